/* eleven_hip.h -- C ABI of the MI355X path-tracing core (libeleven_hip.so).
 *
 * This is the drop-in boundary for ElevenRender's per-sample hot path.  It replaces
 * the SYCL seam of the reference between RenderingManager and the device runtime:
 *
 *   reference interface (file:line under the reference tree)        replaced by
 *   --------------------------------------------------------------  ----------------------
 *   dev_Scene::dev_Scene(Scene*)            src/kernel.cpp:244-266   er_scene_create
 *   copy_scene(dev_Scene*,dev_Scene*,queue) src/SYCLCopy.cpp:3-104   er_scene_create + er_render_begin
 *   renderSetup(q,scene,dev,spp,bs)         src/kernel.cpp:651-678   er_render_begin
 *   kernel_render_enqueue(q,spp,bs,...)     src/kernel.cpp:680-706   er_render_samples
 *   renderingKernel(dev_Scene*,idx,samples) src/kernel.cpp:477-646   (the HIP kernels behind er_render_samples)
 *   RenderingManager::get_pass(string)      src/Managers.cpp:287-302 er_read_pass
 *   RenderingManager::get_render_info()     src/Managers.cpp:211-232 er_samples_done
 *   is_compatible(sycl::device&)            src/kernel.cpp:708-720   er_device_info().compatible
 *   get_sycl_info device enumeration        src/CommandManager.cpp:303-362  er_device_count / er_device_info
 *   NameSelector "name|platform"            src/Managers.cpp:191-208 er_device_find
 *
 * Conventions: plain C, PODs and raw pointers only; every entry point returns
 * ER_OK (0) or a negative ErStatus and never throws; er_last_error() gives the
 * text for the calling thread.  All host pointers in ErSceneDesc stay owned by the
 * caller and are copied during er_scene_create.  The library fails loudly
 * (ER_ERR_NO_DEVICE) when no gfx950 device / HIP runtime is usable: there is no
 * CPU fallback behind this ABI.
 */
#ifndef ELEVEN_HIP_H
#define ELEVEN_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: ErCounters grew the four trace_* fields and ErProfile the empty-launch fields (round 2); a host built against the
 * round-1 header must not pass the version check, since the library fills both caller-allocated structs completely. */
#define ER_ABI_VERSION 2

typedef enum ErStatus {
    ER_OK = 0,
    ER_ERR_INVALID_ARG = -1,
    ER_ERR_NO_DEVICE = -2,
    ER_ERR_HIP = -3,
    ER_ERR_STATE = -4,     /* call order violated (e.g. render before begin) */
    ER_ERR_OOM = -5
} ErStatus;

/* Pass planes, reference enum Passes (src/kernel.h:8). DENOISE is allocated and
 * initialised like the others but never written by the kernel (src/kernel.cpp:604). */
typedef enum ErPass { ER_PASS_BEAUTY = 0, ER_PASS_DENOISE = 1, ER_PASS_NORMAL = 2,
                      ER_PASS_TANGENT = 3, ER_PASS_BITANGENT = 4, ER_PASS_COUNT = 5 } ErPass;

typedef struct ErVec3 { float x, y, z; } ErVec3;

/* reference Camera (src/Camera.h:5-25); rotation in degrees, XYZ Euler. */
typedef struct ErCamera {
    float focal_length, sensor_width, sensor_height, aperture, focus_distance;
    ErVec3 rotation;
    int32_t bokeh;
    ErVec3 position;
} ErCamera;

/* reference Material without its strings (src/Material.h:20-47). Texture ids < 0 = constant. */
typedef struct ErMaterial {
    int32_t albedo_tex, emission_tex, roughness_tex, metallic_tex, normal_tex, opacity_tex,
            transmission_tex;
    int32_t albedo_shader_id;          /* -1 = none; see asl_shade, src/shader.cpp:6-10 */
    ErVec3 albedo, emission;
    float opacity, roughness, metallic, clearcoat_gloss, clearcoat, anisotropic, eta,
          transmission, specular, specular_tint, sheen_tint, subsurface, sheen, ax, ay;
} ErMaterial;

/* reference Texture (src/Texture.h:12-73): interleaved f32, row-major, `channels` per texel.
 * filter: 0 = NO_FILTER, 1 = BILINEAR. */
typedef struct ErTexture {
    int32_t width, height, channels, filter;
    const float* data;
} ErTexture;

/* reference HDRI (src/HDRI.h:9-42). cdf has width*height+1 entries; if NULL the library
 * builds it exactly as HDRI::generateCDF does (src/HDRI.cpp:62-83) and radiance_sum is ignored. */
typedef struct ErHdri {
    ErTexture texture;
    const float* cdf;
    float radiance_sum;
} ErHdri;

/* reference PointLight (src/PointLight.h:4-16). The reference never evaluates point
 * lights (src/kernel.cpp:269-301 has no caller); they are used only when
 * ErRenderParams.flags has ER_FLAG_POINT_LIGHTS (a build-defined extension). */
typedef struct ErPointLight { ErVec3 position, radiance; } ErPointLight;

/* Flattened reference Scene (src/Scene.h:24-73, Tri src/Tri.h:8-21). Triangle arrays are
 * indexed [tri][corner][component]. */
typedef struct ErSceneDesc {
    uint32_t tri_count;
    const float* vertices;       /* [tri_count][3][3] */
    const float* normals;        /* [tri_count][3][3] */
    const float* tangents;       /* [tri_count][3][3] */
    const float* uvs;            /* [tri_count][3][2] */
    const float* tangent_sign;   /* [tri_count] */
    const int32_t* material_id;  /* [tri_count] */
    uint32_t material_count;
    const ErMaterial* materials;
    uint32_t texture_count;
    const ErTexture* textures;
    ErHdri hdri;
    ErCamera camera;
    uint32_t point_light_count;
    const ErPointLight* point_lights;
    uint32_t x_res, y_res;
} ErSceneDesc;

#define ER_FLAG_POINT_LIGHTS 1u   /* extension, default off = reference behaviour: one point-light sample per opaque
                                     bounce after the author's sketch src/kernel.cpp:269-301 (rules: csrc/er_shade.h) */
#define ER_FLAG_MIS          128u /* extension, default off = reference behaviour (NEE and BRDF-sampled environment both
                                     counted in full, src/kernel.cpp:571-577): balance-heuristic weights per direction */
#define ER_FLAG_MESH_LIGHTS  1024u /* extension, default off: next-event estimation of emissive triangles with balance-heuristic
                                     MIS against the BRDF-sampled hits (rules: csrc/er_shade.h).  A scene without emitters renders
                                     as without the flag; with ER_FLAG_POINT_LIGHTS on a scene that has both kinds of light,
                                     er_render_begin returns ER_ERR_INVALID_ARG */
#define ER_FLAG_COUNTERS     2u   /* count node visits / triangle tests (slower kernel variant) */
/* Schedule selection (every schedule computes bit-identical results).  Default: the streaming schedule, at every frame size since
 * round 5 (C1 at 256 x 256: 1 186 Msamples/s against 849 for round 1's fused kernel, which was removed), except for a rank that owns
 * more pixels than the streaming schedule's pixel rings hold (8.4 M): the wavefront schedule.  The flags force one. */
#define ER_FLAG_MEGAKERNEL   4u   /* v0: one wave per 8x8 tile, wave-synchronous bounce loop over the binary BVH */
#define ER_FLAG_FUSED        16u  /* (round 1's lane-asynchronous single kernel, removed in round 5: accepted, means ER_FLAG_STREAM) */
#define ER_FLAG_WAVEFRONT    32u  /* one trace + one shade launch per bounce over compacted ray queues */
#define ER_FLAG_STREAM       256u /* one launch per call, one resident workgroup per CU: tracer waves and shader waves feed each
                                     other through rings in LDS (er_stream.hip) */
#define ER_FLAG_PROFILE      8u   /* bracket every trace / shade launch with HIP events (see er_get_profile) */
/* Acceleration-structure builder.  Default since round 5: the DEVICE build (top-down binned SAH on the GPU, the host builder's own
 * algorithm and tree: 65 ms instead of 0.43 s at 1 M triangles, 0.33 s instead of 5.0 s at 10 M) for scenes of at least
 * ER_GPU_BUILD_MIN_TRIS (20 000; environment variable of that name) triangles, the host build below that; a device build that
 * declines or fails falls back to the host build.  Images do not depend on the builder. */
#define ER_FLAG_GPU_BUILD    64u  /* force the device build whatever the triangle count (an error of it is then the call's error) */
#define ER_FLAG_HOST_BUILD   512u /* force the host build (er_bvh.cpp) */

/* The largest ErRenderParams::max_bounces: every schedule keeps a path's bounce count in 16 bits of a packed word, below its flag bits
 * (csrc/er_wavefront.h ER_SLOT_PENDING).  er_render_begin refuses a larger value. */
#define ER_MAX_BOUNCES 65535u

/* reference RenderParameters (src/kernel.h:51-69) + what the MI355X build adds. */
typedef struct ErRenderParams {
    uint32_t sample_target;   /* informational, as in the reference */
    uint32_t block_size;      /* accepted for protocol compatibility; launch geometry is ours */
    uint32_t max_bounces;     /* 0 -> 5, the literal of src/kernel.cpp:508; at most ER_MAX_BOUNCES (more: ER_ERR_INVALID_ARG) */
    int32_t device;           /* HIP device ordinal */
    uint32_t rank, world;     /* pixel-tile shard: this process renders tiles t with t % world == rank; world 0 -> 1 */
    uint32_t flags;
} ErRenderParams;

typedef struct ErDeviceInfo {
    char name[256];
    char platform[64];        /* "AMD HIP" */
    uint64_t memory_bytes;
    uint32_t compute_units;
    int32_t compatible;       /* 1 iff gcnArchName starts with gfx950 */
    char arch[64];
} ErDeviceInfo;

/* Counters of the work done since er_render_begin (all ranks count only their own pixels). */
typedef struct ErCounters {
    uint64_t paths;            /* pixel-samples finished */
    uint64_t bounce_samples;   /* executed iterations of the bounce loop = the Msamples metric unit */
    uint64_t rays;             /* closest-hit + shadow traversals started */
    uint64_t node_visits;      /* only with ER_FLAG_COUNTERS */
    uint64_t tri_tests;        /* only with ER_FLAG_COUNTERS */
    uint64_t shaded_hits;      /* closest hits shaded */
    uint64_t texel_fetches;    /* only with ER_FLAG_COUNTERS */
    uint64_t hdri_samples;     /* CDF searches */
    /* lane occupancy of the wavefront traversal loop (only with ER_FLAG_COUNTERS): iterations of er_wf_trace's loop summed
     * over its waves, and how many of the 64 lanes held a ray / ran the node part / ran the triangle part in them */
    uint64_t trace_wave_steps, trace_busy_lanes, trace_node_lanes, trace_tri_lanes;
} ErCounters;

typedef struct ErScene ErScene;   /* opaque */

int er_abi_version(void);
const char* er_last_error(void);

int er_device_count(void);
int er_device_info(int index, ErDeviceInfo* out);
/* index of the device whose "name|platform" equals selector, or a negative status. */
int er_device_find(const char* selector);

int er_scene_create(const ErSceneDesc* desc, ErScene** out);
void er_scene_destroy(ErScene* scene);

/* Builds the acceleration structure, uploads, initialises passes/samples/RNG (setupKernel,
 * src/kernel.cpp:176-213, for EVERY pixel). May be called again to restart a render. */
int er_render_begin(ErScene* scene, const ErRenderParams* params);

/* Adds n samples to every owned pixel. Blocking. Equivalent to n launches of renderingKernel. */
int er_render_samples(ErScene* scene, uint32_t n);
/* Non-blocking form + explicit wait; elapsed_ms (may be NULL) = device time of everything
 * enqueued since the previous er_wait, measured with HIP events on the library's stream.
 * (Streaming schedule, the first call of a render with n >= 2: its first sample is a launch of its own that the
 * call waits for -- the library then decides, from the work counted in it, which screen regions go to which XCD --
 * before the other n - 1 samples are enqueued: that one call blocks for one sample pass.) */
int er_render_samples_async(ErScene* scene, uint32_t n);
int er_wait(ErScene* scene, float* elapsed_ms);

/* reference get_render_info semantic: dev_samples[0], i.e. samples added + 1. */
int er_samples_done(ErScene* scene, uint32_t* out);

/* Copies one pass plane (x_res*y_res*4 floats, RGBA, row-major, idx = y*x_res + x) to host memory.
 * With world > 1 only owned pixels are valid; others are left at the setup value (0,0,0,1). */
int er_read_pass(ErScene* scene, int pass, float* dst_rgba);
int er_read_samples(ErScene* scene, uint32_t* dst);

/* Checkpoint / resume (the reference keeps the progressive estimator only in device memory --
 * dev_passes + dev_samples + dev_randstate, src/kernel.h:44-46 -- and these three arrays ARE a complete resumable state).
 * er_state_size: bytes of one snapshot of this scene (5 planes of float4 + 2 u32 per pixel + a 64-byte header).
 * er_state_export: a sample-boundary snapshot into host memory (ordered after everything enqueued, like er_read_pass).
 * er_state_import: after er_render_begin on a scene of the same resolution, continue from a snapshot: the next
 * er_render_samples(n) gives exactly what n more samples would have given in the run that exported it (per-pixel RNG
 * streams; any schedule, any rank/world split -- a rank only ever touches the pixels it owns). */
int er_state_size(ErScene* scene, uint64_t* bytes);
int er_state_export(ErScene* scene, void* dst, uint64_t bytes);
int er_state_import(ErScene* scene, const void* src, uint64_t bytes);

/* Fills the DENOISE plane (which renderingKernel never writes, src/kernel.cpp:604) with an edge-avoiding a-trous
 * wavelet filter of the current BEAUTY plane, guided by colour and by the NORMAL plane: `levels` passes (1..8, 0 -> 5)
 * with stencil holes of 1, 2, 4, ... pixels; colour_sigma > 0 scales the colour edge-stop (0 -> 1).  Stands in for the
 * reference's host-side OIDN call behind `get_pass denoise` (src/Managers.cpp:319-343, CommandManager.cpp:265-274) --
 * a different filter: no parity claim.  On a frame sharded over several ranks (world > 1) it runs on the rank that BEAUTY
 * and NORMAL have been gathered to since the last sample (er_gather_pass, or er_unpack_owned of every other rank), as
 * the reference denoises where the whole pass is; elsewhere ER_ERR_STATE. */
int er_denoise(ErScene* scene, uint32_t levels, float colour_sigma);     /* x_res*y_res */
int er_read_rng(ErScene* scene, uint32_t* dst);         /* x_res*y_res */

/* Multi-GPU framebuffer combine helpers (the collective itself is done by the host with
 * RCCL; these move owned pixels between the full plane and a compact device buffer).
 * er_owned_count: number of pixels this rank owns.
 * er_pack_owned: dev_dst[owned][4] <- owned pixels of `pass`, in owned-pixel order (device pointer).
 * er_unpack_owned: scatters a compact buffer of rank `src_rank` into this scene's full plane. */
int er_owned_count(ErScene* scene, uint32_t rank, uint64_t* out);
int er_pack_owned(ErScene* scene, int pass, void* dev_dst);
int er_unpack_owned(ErScene* scene, int pass, uint32_t src_rank, const void* dev_src);

/* The combine itself, from the C++ side (north_star: "RCCL reduce over xGMI only for the final framebuffer accumulate";
 * reference hook: RenderingManager::get_pass, src/Managers.cpp:287-302).  One process per GPU:
 *   rank 0: er_comm_unique_id(id) -> the host hands the 128 bytes to the other ranks through any channel it has
 *           (the reference's host would use its TCP session; bench.py uses torch.distributed's broadcast)
 *   all:    er_comm_create(id, rank, world, device, &comm)        -- ncclCommInitRank; RCCL is dlopen'ed at this point
 *   all:    er_gather_pass(scene, pass, comm, root)               -- every rank packs the pixels it owns; the non-root
 *           ranks ncclSend, the root ncclRecv's inside ONE group (xGMI is point to point: the seven links carry the
 *           seven buffers side by side) and scatters them into its full plane.  One call per read-back, none per sample.
 *   all:    er_comm_destroy(comm)
 * The scene must have been begun with the communicator's rank / world. */
typedef struct ErComm ErComm;
#define ER_COMM_ID_BYTES 128
int er_comm_unique_id(uint8_t id[ER_COMM_ID_BYTES]);
int er_comm_create(const uint8_t id[ER_COMM_ID_BYTES], uint32_t rank, uint32_t world, int device, ErComm** out);
/* The same for the ranks of ONE process (a host that drives several GPUs itself, reference hook: RenderingManager with N
 * devices; also several ranks on one GPU): `world` communicators over an in-process transport -- a send parks a device copy,
 * the matching receive copies it device to device (peer copy over xGMI between two GPUs); no RCCL involved.  out[world].
 * er_gather_pass may be called by the ranks in any order, from one thread per rank or (non-roots first) from one thread. */
int er_comm_create_local(uint32_t world, ErComm** out);
void er_comm_destroy(ErComm* comm);
int er_gather_pass(ErScene* scene, int pass, ErComm* comm, uint32_t root);

int er_get_counters(ErScene* scene, ErCounters* out);

/* Adaptive sampling (extension, off by default = reference behaviour): owned 8x8 tiles whose noise has fallen below a threshold
 * stop receiving samples.  Tests run when min_samples, min_samples + interval, min_samples + 2 interval, ... samples have been
 * rendered since er_render_begin, whatever the calls' sizes (a call that crosses a test point is split there inside the library,
 * and er_render_samples_async then blocks at each test point inside the call, as the streaming schedule's first call does for its
 * first sample).  A test compares every active tile's BEAUTY plane with a snapshot taken `interval` samples earlier: per pixel the
 * standard error of the running mean, relative to the square root of its brightness; per tile E = the root mean square of those
 * (csrc/er_adaptive.hip gives the exact operations).  A tile stays active iff E >= threshold or it has no testable pixel; a
 * stopped tile never comes back (threshold 0: none stops; +inf: every testable tile stops at the first test).  Every pixel keeps
 * its own RNG stream, so a tile that received k samples equals, bit for bit, the tile of a uniform render of k samples.
 * er_adaptive_set: only between er_render_begin and the first sample (else ER_ERR_STATE); NULL = off; er_render_begin turns it
 * off again.  Threshold negative or NaN, or interval >= min_samples: ER_ERR_INVALID_ARG.  er_state_import of an adaptive render:
 * ER_ERR_STATE (resuming the adaptive state is not supported).  A call once no tile is active returns ER_OK and launches nothing. */
typedef struct ErAdaptiveParams {
    float threshold;
    uint32_t min_samples;        /* 0 -> 16 */
    uint32_t interval;           /* 0 -> 8 */
} ErAdaptiveParams;
typedef struct ErAdaptiveInfo {
    uint32_t enabled, owned_tiles, active_tiles, tests_done;
    uint32_t samples_rendered;   /* samples every still-active tile has received since er_render_begin */
    uint32_t next_test;          /* samples_rendered at which the next test runs (0: not adaptive) */
    uint64_t pixel_samples;      /* samples given, summed over owned pixels: the work spent */
    float max_active_error;      /* largest E among the tiles kept at the last test (-1: none yet) */
} ErAdaptiveInfo;
int er_adaptive_set(ErScene* scene, const ErAdaptiveParams* params);
int er_adaptive_info(ErScene* scene, ErAdaptiveInfo* out);
/* Per tile of the frame (tiles_x * tiles_y each, row-major; either pointer may be NULL): the error E of its last test (-1: untested,
 * untestable or not owned) and the samples it has received since er_render_begin (0: not owned). */
int er_read_tile_state(ErScene* scene, float* error, uint32_t* samples);

/* The emitter table of ER_FLAG_MESH_LIGHTS (csrc/er_shade.h): valid after er_render_begin (before it: ER_ERR_STATE; NULL argument:
 * ER_ERR_INVALID_ARG).  emitters = 0 when the flag is off or the scene has no emitter; total_weight = the sum of area x luminance. */
typedef struct ErLightInfo {
    uint32_t emitters;
    float total_weight;
} ErLightInfo;
int er_light_info(ErScene* scene, ErLightInfo* out);

/* Per-kernel device time of the launches enqueued since the previous er_wait, measured with HIP events on
 * the library's stream (needs ER_FLAG_PROFILE; valid after er_wait). */
typedef struct ErProfile {
    float trace_ms, shade_ms;          /* summed over the launches that had rays to trace */
    uint32_t trace_launches, shade_launches;   /* ... and their number */
    uint32_t schedule;                 /* ER_FLAG_WAVEFRONT / ER_FLAG_FUSED / ER_FLAG_MEGAKERNEL actually in use; for the
                                          two single-kernel schedules trace_ms is that kernel's time and shade_ms is 0 */
    uint32_t concurrency;              /* wavefront schedule: number of slot pools whose launches run side by side on
                                          their own streams (their durations overlap, so trace_ms + shade_ms exceeds the
                                          elapsed time by up to this factor); 1 otherwise */
    uint32_t empty_launches;           /* wavefront schedule: trace + shade pairs that found empty queues (the host loop always
                                          enqueues n * (max_bounces + 1) iterations), and their summed duration */
    float empty_ms;
    uint64_t rays_logged;              /* wavefront schedule: rays the counted trace launches found in their queues */
} ErProfile;
int er_get_profile(ErScene* scene, ErProfile* out);

/* Measured HBM bandwidth of `device`, for the roofline's denominator ("the denominator used is the
 * measured peak from a device-to-device copy / triad kernel run in the same job"): a streaming copy and a streaming
 * read over `bytes` of device memory (0 -> 2 GiB, several times the 256 MB Infinity Cache), best of `iters` (0 -> 5)
 * timed with HIP events.  copy counts bytes read + bytes written. */
int er_measure_hbm_peak(int device, uint64_t bytes, uint32_t iters, float* copy_GBps, float* read_GBps);

/* Description of the built acceleration structure, for roofline accounting. */
typedef struct ErAccelInfo {
    uint32_t node_count, node_bytes;   /* wide nodes */
    uint32_t leaf_count, max_depth;
    uint32_t tri_record_bytes;         /* bytes fetched per triangle test */
    float build_ms, upload_ms;
    float lift_bound;                  /* global bound on |shadingPosition - geomPosition| */
    uint32_t builder;                  /* 0 = host binned-SAH build, 1 = device binned-SAH build, 2 = refit of an earlier build
                                          (er_render_update with ER_UPDATE_GEOMETRY; build_ms then holds the refit's device time) */
} ErAccelInfo;
int er_accel_info(ErScene* scene, ErAccelInfo* out);

/* Edit a begun scene in place: a new camera, moved triangles, or both, without the stages of er_render_begin that the edit does not
 * concern (no build, no texture, material or record upload for a camera; a device refit of the built structure for geometry).
 * After ER_OK every readable output -- the five planes, samples, RNG, er_get_counters, er_samples_done, er_light_info,
 * er_adaptive_info (off again), er_state_* -- equals what er_scene_destroy, er_scene_create of the description with that camera or
 * those arrays replaced, and er_render_begin with the same ErRenderParams would give, bit for bit: the render starts over at sample
 * 0.  The one exception is the acceleration structure after a geometry update: its topology (child references, slot assignment,
 * triangle order) is kept and only the boxes and the triangle records are recomputed, ErAccelInfo.builder reports 2 and build_ms the
 * refit's device time.  Images do not depend on the tree; traversal cost grows with the deformation, and er_render_begin remains the
 * way to a fresh tree.  A camera-only update leaves ErAccelInfo unchanged, field for field.
 * Call order: the scene must be begun (else ER_ERR_STATE); pending asynchronous work is waited for.  NULL arguments, `what` 0 or with
 * unknown bits, NULL vertices with ER_UPDATE_GEOMETRY, or a vertex coordinate that is not finite: ER_ERR_INVALID_ARG, the scene is
 * untouched and still begun.  The scene's host copy (vertices, normals, tangents, camera) is replaced before any device work; if device
 * work then fails, the scene is NO LONGER BEGUN -- every render call returns ER_ERR_STATE -- and a later er_render_begin rebuilds from
 * the edited host copy. */
#define ER_UPDATE_CAMERA   1u
#define ER_UPDATE_GEOMETRY 2u
typedef struct ErSceneUpdate {
    uint32_t what;            /* bits above */
    ErCamera camera;          /* read iff ER_UPDATE_CAMERA */
    const float* vertices;    /* ER_UPDATE_GEOMETRY: [tri_count][3][3], required; tri_count is the scene's */
    const float* normals;     /* [tri_count][3][3] or NULL = keep */
    const float* tangents;    /* [tri_count][3][3] or NULL = keep */
} ErSceneUpdate;
typedef struct ErUpdateInfo {
    uint32_t updates;         /* successful er_render_update calls since er_scene_create */
    uint32_t refits;          /* ... of which refitted the structure */
    float refit_ms;           /* device time of the last refit (HIP events: uploads of the arrays to the last tree level), 0 if none */
    float update_ms;          /* host wall time of the last er_render_update */
} ErUpdateInfo;
int er_render_update(ErScene* scene, const ErSceneUpdate* update);
int er_update_info(ErScene* scene, ErUpdateInfo* out);

/* er_render_update extended to the rest of a look-dev session: materials, textures and the HDRI of a begun scene edited in place.
 * The contract is er_render_update's, word for word, for every bit: after ER_OK every readable output -- the five planes, samples,
 * RNG, er_get_counters, er_samples_done, er_light_info, er_adaptive_info (off again), er_state_* -- equals what er_scene_destroy,
 * er_scene_create of the edited description and er_render_begin with the same ErRenderParams give, bit for bit; the render starts
 * over at sample 0 and the feature planes are invalidated.  What an edit costs is what it touches:
 *   MATERIALS whose texture ids all equal the current list's (same count), without TEXTURES: the materials and their constants are
 *     uploaded (and the triangles' material ids, if given); the texture pool is not touched (texture_stage 0)
 *   MATERIALS with another count or a changed texture id, or TEXTURES: the texture pool is laid out again and rebuilt ON THE DEVICE
 *     (csrc/er_texstage.hip; the layout and every byte are those of er_render_begin's host fill) (texture_stage 2)
 *   HDRI: its CDF (built by the library unless given), the search guide, and the HDRI's texels at the pool's tail, in place if the
 *     allocation holds them (texture_stage 1, unless the pool was rebuilt in the same call)
 * With ER_FLAG_MESH_LIGHTS the emitter table is rebuilt after MATERIALS, TEXTURES or GEOMETRY (an edit may create the first emitter
 * or remove the last).
 * A call with only CAMERA / GEOMETRY is er_render_update and counts in ErUpdateInfo as that; ErUpdateInfo.updates counts successful
 * calls of either entry point and refits the refits of either; ErEditInfo.edits counts the successful calls that named one of the
 * three new bits.
 * ER_ERR_INVALID_ARG, the scene untouched and still begun: NULL arguments; `what` 0 or with unknown bits; a bit without its array
 * (GEOMETRY without vertices, MATERIALS without materials, TEXTURES with a count but no list); material_count 0; a non-finite vertex;
 * texture_count below the scene's; a texture with data == NULL at an index the scene does not have; a texture or an HDRI that
 * er_scene_create refuses; a material_id entry (given, or kept with a shorter list) or a material's texture id beyond the new lists,
 * as er_scene_create refuses them (a negative texture id means "no texture"); a texture pool that would reach 2^32 floats.
 * As for er_render_update the host copy is replaced before any device work, and if device work then fails the scene is no longer
 * begun. */
#define ER_EDIT_CAMERA    1u   /* = ER_UPDATE_CAMERA   */
#define ER_EDIT_GEOMETRY  2u   /* = ER_UPDATE_GEOMETRY */
#define ER_EDIT_MATERIALS 4u
#define ER_EDIT_TEXTURES  8u
#define ER_EDIT_HDRI      16u
typedef struct ErSceneEdit {
    uint32_t what;
    ErCamera camera;                                   /* as in ErSceneUpdate */
    const float *vertices, *normals, *tangents;        /* as in ErSceneUpdate */
    uint32_t material_count; const ErMaterial* materials;   /* MATERIALS: the complete new list, count >= 1 */
    const int32_t* material_id;                        /* MATERIALS: [tri_count] or NULL = keep */
    uint32_t texture_count; const ErTexture* textures; /* TEXTURES: the complete new list; data == NULL = keep texture i as it is */
    ErHdri hdri;                                       /* HDRI: as in ErSceneDesc (cdf NULL = built by the library) */
} ErSceneEdit;
int er_render_edit(ErScene* scene, const ErSceneEdit* edit);
typedef struct ErEditInfo {
    uint32_t edits;            /* successful er_render_edit calls with MATERIALS, TEXTURES or HDRI since er_scene_create */
    uint32_t texture_stage;    /* the last of them: 0 the pool was not touched, 1 only the HDRI's tail was rewritten, 2 rebuilt on the device */
    float texture_stage_ms;    /* device time of that pool work (HIP events), 0 if none */
    float edit_ms;             /* host wall time of the last of them */
    uint64_t pool_floats;      /* the texture pool after it */
} ErEditInfo;
int er_edit_info(ErScene* scene, ErEditInfo* out);

/* A measured cost of the acceleration structure as it lies in device memory, whichever builder or refit left it (csrc/er_cost.h gives
 * every operation): the areas of the boxes a traversal tests, weighted by the bytes fetched for each, over the areas of the triangles'
 * own boxes --
 *   cost = (ErAccelInfo.node_bytes x node_area + ErAccelInfo.tri_record_bytes x leaf_area) / tri_area
 *   node_area = the root's box + every inner child box; leaf_area = every leaf child box x its triangles; tri_area = every triangle's box
 * (0 for a scene without triangles or without area).  Translation and scale do not change it; it rises when a refit has grown node
 * boxes around triangles that moved apart.  Only the RATIO of two costs of one scene means anything.  Bitwise reproducible.
 * The scene must be begun (else ER_ERR_STATE); pending asynchronous work is waited for; planes, RNG and counters are neither read nor
 * written.  The result is kept until the next build or refit, so a second call launches nothing (ms is then the first call's). */
typedef struct ErAccelCost {
    double node_area, leaf_area, tri_area, cost;
    float ms;                  /* device time of the measurement (HIP events) */
    uint32_t builder;          /* ErAccelInfo.builder of the structure measured */
} ErAccelCost;
int er_accel_cost(ErScene* scene, ErAccelCost* out);

/* What the geometry bit of er_render_update / er_render_edit does to the structure.  ER_REBUILD_NEVER (a fresh scene's policy): the
 * refit described above, always.  ER_REBUILD_ALWAYS: the structure stage of er_render_begin runs again on the edited arrays -- the
 * builder chosen by the same flags, environment and thresholds -- and nothing else of er_render_begin does.  ER_REBUILD_AUTO: the refit,
 * then er_accel_cost of the refitted tree; if that exceeds max_cost_ratio x the cost of the last BUILT tree, the structure is built
 * fresh in the same call.  (The built tree's cost is measured before the refit unless it is known; a scene whose structure is already a
 * refit of unknown ancestry -- earlier updates ran under NEVER -- is rebuilt once, which gives the baseline.  A built tree of cost 0 is
 * never rebuilt by ratio.)  After an update that ended in a rebuild the exception of er_render_update's contract is gone: the
 * structure is, byte for byte, that of a fresh er_scene_create + er_render_begin, ErAccelInfo.builder is 0 or 1, and
 * ErUpdateInfo.refits does not count the call.  There is no library default for the ratio; DESIGN.md 3g has the measurements to choose one by.
 * er_update_policy_set needs only a created scene; the policy lasts until er_scene_destroy.  An unknown mode, or AUTO with a ratio
 * that is not finite or below 1: ER_ERR_INVALID_ARG, the policy unchanged. */
#define ER_REBUILD_NEVER  0u
#define ER_REBUILD_ALWAYS 1u
#define ER_REBUILD_AUTO   2u
typedef struct ErUpdatePolicy {
    uint32_t mode;
    float max_cost_ratio;      /* read iff ER_REBUILD_AUTO */
} ErUpdatePolicy;
typedef struct ErRebuildInfo {
    uint32_t mode; float max_cost_ratio;   /* the policy in force */
    uint32_t rebuilds;         /* geometry updates since er_scene_create that ended in a rebuild */
    uint32_t last_decision;    /* of the last geometry update under ALWAYS or AUTO: 0 none yet, 1 refit kept, 2 rebuilt: ratio exceeded,
                                  3 rebuilt: ALWAYS, 4 rebuilt: no baseline */
    double cost_built;         /* AUTO: the baseline the last decision used (0 if it had none) */
    double cost_refit;         /*       the refitted tree's cost (0 if no refit ran) */
    double cost_after;         /*       the rebuilt tree's cost = the next baseline (0 if the refit was kept) */
    float cost_ms;             /* device time of that update's measurements */
    float rebuild_ms;          /* host wall time of its structure stage, 0 if the refit was kept */
} ErRebuildInfo;
int er_update_policy_set(ErScene* scene, const ErUpdatePolicy* policy);
int er_rebuild_info(ErScene* scene, ErRebuildInfo* out);

/* er_render_update for an edit that moves FEW triangles: the listed ones are given, the others stay.  After ER_OK everything
 * observable -- planes, samples, RNG, counters, er_state_*, er_light_info, the structure byte for byte (er_debug_read_accel),
 * ErAccelInfo except build_ms, ErUpdateInfo.updates / .refits, and every decision of er_update_policy_set with its ErRebuildInfo --
 * equals what er_render_update with the same `what` and camera and the COMPLETE arrays (the scene's current ones with the listed
 * triangles replaced) would leave.  What differs is the cost: nothing of the geometry stage is proportional to tri_count on the host
 * or over PCIe.  The listed records are scattered on the device; if the scene's largest |coordinate| kept its bits, only the nodes above
 * the moved triangles are recomputed, from boxes kept on the device since the last refit (path 1).  If it changed -- it sets the
 * absolute padding of EVERY box -- or if no refit has run on this topology yet (after er_render_begin or a rebuild the kept boxes do
 * not exist), the whole refit runs from the records on the device (path 2); still nothing but the listed triangles is uploaded.
 * ER_ERR_STATE unless the scene is begun.  ER_ERR_INVALID_ARG, the scene untouched and still begun: NULL arguments; `what` 0 or with
 * unknown bits; GEOMETRY with count 0 or without tri_ids or vertices; an id >= tri_count; an id listed twice; a listed vertex
 * coordinate that is not finite.  The checks cost O(count) time and memory. */
typedef struct ErSparseUpdate {
    uint32_t what;            /* ER_UPDATE_CAMERA | ER_UPDATE_GEOMETRY, as ErSceneUpdate */
    ErCamera camera;          /* read iff ER_UPDATE_CAMERA */
    uint32_t count;           /* ER_UPDATE_GEOMETRY: number of listed triangles, >= 1 */
    const uint32_t* tri_ids;  /* [count], each < tri_count, no id twice */
    const float* vertices;    /* [count][3][3], required */
    const float* normals;     /* [count][3][3] or NULL = keep */
    const float* tangents;    /* [count][3][3] or NULL = keep */
} ErSparseUpdate;
int er_render_update_sparse(ErScene* scene, const ErSparseUpdate* update);

typedef struct ErSparseInfo {
    uint32_t calls;           /* successful sparse geometry updates since er_scene_create */
    uint32_t path;            /* the last one: 1 = dirty ancestors only, 2 = whole refit from device-resident data,
                                 3 = ended in a rebuild (policy) */
    uint32_t why_full;        /* path 2: 1 = no kept boxes for this topology yet, 2 = the largest |coordinate| changed */
    uint32_t moved;           /* = count */
    uint32_t dirty_nodes2, dirty_nodes8;   /* binary / wide nodes rewritten (path 1; the node counts on path 2) */
    uint64_t bytes_uploaded;  /* host-to-device bytes of the geometry stage */
    float refit_ms;           /* device time, HIP events, as ErUpdateInfo.refit_ms */
} ErSparseInfo;
int er_sparse_info(ErScene* scene, ErSparseInfo* out);

/* Object transforms: registered objects posed ON THE DEVICE by matrix (csrc/er_xform.h gives every operation).
 * er_objects_set: disjoint lists of triangle ids in CSR form -- object o = tri_ids[first[o] .. first[o + 1]) -- become the scene's object
 * table.  Legal any time after er_scene_create.  The REST POSE of every listed triangle -- vertices, normals, tangents -- is taken from
 * the scene's current arrays; an earlier table is replaced, object_count 0 clears it (neither array is then read).  The table belongs to
 * the scene: it survives rebuilds and a second er_render_begin.  Triangles in no object are allowed, and so are empty objects.
 * ER_ERR_INVALID_ARG, the scene and its table untouched: NULL arguments; a `first` that does not start at 0 or that decreases; an id that
 * is not below tri_count; an id in two objects or twice in one.
 * er_render_transform: every listed object takes the pose pose(rest, m): x' = L x + t for m = [L | t], row-major 3x4; normals by the
 * cofactor matrix of L, tangents by L, both normalised (unit or zero).  The pose is ABSOLUTE, from the rest copy: a second transform of
 * an object does not compose with the first and nothing drifts.  Objects not listed keep their current pose.  After ER_OK everything
 * observable -- planes, samples, RNG, counters, er_state_*, er_light_info, the structure byte for byte (er_debug_read_accel), ErAccelInfo
 * except its timings, ErUpdateInfo's counts, and every decision of er_update_policy_set with its ErRebuildInfo -- equals what
 * er_render_update_sparse would leave when given the listed objects' ids with pose(rest, m) as vertices, normals and tangents, the same
 * `what` and the same camera.  tangent_sign and the records' sign stay, as in every refit.  What differs is the cost: the host touches
 * no triangle and 128 bytes per listed OBJECT go to the device (ErTransformInfo.bytes_uploaded = 128 x count + 64, + 64 on path 2); the
 * rest copy lies on the device (112 bytes per listed triangle, uploaded by the first transform after er_objects_set or er_render_begin).
 * The scene's host copy takes a pose lazily, when something reads it (a rebuild, er_render_begin, a sparse or partial update).  A direct
 * edit (er_render_update, er_render_update_sparse, er_render_edit) of a triangle in an object moves its current pose only: the rest copy
 * stays what er_objects_set saw, and the object's next transform poses it from there.
 * ER_ERR_STATE: the scene is not begun, or ER_UPDATE_GEOMETRY without an object table.  ER_ERR_INVALID_ARG, the scene untouched and
 * still begun: NULL arguments; `what` 0 or with unknown bits; GEOMETRY with count 0, without transforms, or with listed objects that
 * hold no triangle; an object index not below the object count; an object listed twice; a matrix entry that is not finite; det(L) not
 * > 0 (a mirror would have to flip the records' sign, which no refit does); a matrix with |m_i0| Bx + |m_i1| By + |m_i2| Bz + |m_i3| >
 * 1e37 in some row, B being the object's largest rest |coordinate| per axis (what keeps every posed vertex finite).  The checks cost
 * O(count) time and memory. */
int er_objects_set(ErScene* scene, uint32_t object_count, const uint32_t* first /*[object_count + 1]*/, const uint32_t* tri_ids);
typedef struct ErObjectTransform { uint32_t object; float m[12]; } ErObjectTransform;   /* row-major 3x4, x' = L x + t */
typedef struct ErTransformUpdate {
    uint32_t what;            /* ER_UPDATE_CAMERA | ER_UPDATE_GEOMETRY, as ErSparseUpdate */
    ErCamera camera;          /* read iff ER_UPDATE_CAMERA */
    uint32_t count;           /* ER_UPDATE_GEOMETRY: listed objects, each at most once */
    const ErObjectTransform* transforms;
} ErTransformUpdate;
int er_render_transform(ErScene* scene, const ErTransformUpdate* update);
typedef struct ErTransformInfo {
    uint32_t calls;           /* successful er_render_transform calls with ER_UPDATE_GEOMETRY since er_scene_create */
    uint32_t objects;         /* the last one: listed objects ... */
    uint32_t moved;           /* ... and their triangles */
    uint32_t path, why_full;  /* as ErSparseInfo */
    uint32_t dirty_nodes2, dirty_nodes8;
    uint32_t reserved;
    uint64_t bytes_uploaded;  /* host-to-device bytes of the geometry stage: the entries and the refit's counter words */
    float refit_ms;           /* device time, HIP events, as ErUpdateInfo.refit_ms */
} ErTransformInfo;
int er_transform_info(ErScene* scene, ErTransformInfo* out);

/* Skinning: registered objects DEFORMED on the device by linear-blend skinning from bone matrices (csrc/er_skin.h gives every operation;
 * DESIGN.md 3p).  Geometry is a triangle soup, so influences are per corner: ER_SKIN_INFLUENCES pairs (bone index, weight) for each of a
 * triangle's three corners, in the order of the object's tri_ids.
 * er_skin_set: gives object `object` of the er_objects_set table a skin of bone_count bones, or with bone_count 0 removes it (the arrays
 * are then not read).  Legal any time after er_scene_create, once a table exists.  The influences are copied and belong to the scene:
 * they survive rebuilds and a second er_render_begin.  er_objects_set and er_render_topology DROP EVERY SKIN (a pending skin pose is
 * flushed into the host copy first, as pending matrices are; ErSkinInfo.skinned is then 0): carrying skins through a renumbering is not
 * done.  ER_ERR_STATE without an object table.  ER_ERR_INVALID_ARG, the scene and every skin untouched: NULL arguments; an object index
 * not below the object count; an empty object; bone_count above ER_SKIN_MAX_BONES; a bone index not below bone_count, also where its
 * weight is 0; a weight that is not finite or outside [0, 1].  Weights are used as given: they are not renormalised.
 * er_render_skin: every listed object takes the pose of csrc/er_skin.h from its REST copy and the given palette of row-major 3x4 bone
 * matrices: per corner the blended matrix M = ((w0 P[b0] + w1 P[b1]) + w2 P[b2]) + w3 P[b3]; the position by M, the normal by the
 * cofactor matrix of M's 3x3 part, the tangent by that part, both normalised (unit or zero).  The pose is ABSOLUTE: nothing composes and
 * nothing drifts.  Objects not listed keep their current pose.  A later er_render_transform of the same object poses it by matrix from
 * the same rest copy, and the other way round: the last call wins.  After ER_OK everything observable -- planes, samples, RNG, counters,
 * er_state_*, er_light_info, the structure byte for byte (er_debug_read_accel), ErAccelInfo except its timings, ErUpdateInfo's counts,
 * every decision of er_update_policy_set with its ErRebuildInfo, and what feature planes, id planes, the history (dropped: a deformation
 * has no back matrix) and the variance state do -- equals what er_render_update_sparse would leave when given the listed objects' ids
 * with that pose as vertices, normals and tangents, the same `what` and the same camera.  tangent_sign and the records' sign stay.
 * What differs is the cost: the host touches no triangle, and what goes to the device follows the objects and bones listed, never their
 * triangle counts:
 *   ErSkinInfo.bytes_uploaded = 32 x objects + 48 x bones + 64   (+ 64 on path 2)
 * -- one entry per listed object, the palettes, the refit's sixteen counter words.  The influences lie on the device beside the rest
 * copy, 72 bytes per triangle of a skinned object (3 x 4 x (2 + 4)); they are uploaded with the rest copy by the first er_render_skin
 * after an er_skin_set or an er_render_begin and counted by themselves in ErSkinInfo.influence_bytes (0 in every other call).  The
 * scene's host copy takes a pose lazily, as after er_render_transform.
 * ER_ERR_STATE: the scene is not begun, or ER_UPDATE_GEOMETRY names an object without a skin.  ER_ERR_INVALID_ARG, the scene untouched
 * and still begun: NULL arguments; `what` 0 or with unknown bits; GEOMETRY with count 0; an object index not below the object count; an
 * object listed twice; a bone_count different from the skin's; a matrix entry that is not finite; a bone whose det(L) is not > 0; a bone
 * that fails er_render_transform's bound 1e37 against the object's largest rest |coordinate|; a bone with a linear entry |L_ij| > 16384
 * (2^14: blended entries then stay below 2^16 and their float32 cofactors below 2^33).  The checks cost O(objects listed + bones
 * listed) time and memory. */
#define ER_SKIN_INFLUENCES 4
#define ER_SKIN_MAX_BONES  1024u
typedef struct ErSkin {
    uint32_t object;          /* index into the er_objects_set table */
    uint32_t bone_count;      /* 1..ER_SKIN_MAX_BONES; 0 removes the object's skin (arrays not read) */
    const uint16_t* bones;    /* [size_of(object)][3][ER_SKIN_INFLUENCES], the object's tri_ids order */
    const float* weights;     /* same shape */
} ErSkin;
int er_skin_set(ErScene* scene, const ErSkin* skin);
typedef struct ErSkinPose { uint32_t object, bone_count; const float* palette; /* [bone_count][12] */ } ErSkinPose;
typedef struct ErSkinUpdate {
    uint32_t what;            /* ER_UPDATE_CAMERA | ER_UPDATE_GEOMETRY, as ErSparseUpdate */
    ErCamera camera;          /* read iff ER_UPDATE_CAMERA */
    uint32_t count;           /* ER_UPDATE_GEOMETRY: listed objects, each at most once */
    const ErSkinPose* poses;
} ErSkinUpdate;
int er_render_skin(ErScene* scene, const ErSkinUpdate* update);
typedef struct ErSkinInfo {
    uint32_t calls;           /* successful er_render_skin calls with ER_UPDATE_GEOMETRY since er_scene_create */
    uint32_t skinned;         /* objects that have a skin now */
    uint32_t objects;         /* the last call: listed objects ... */
    uint32_t bones;           /* ... their bones ... */
    uint32_t moved;           /* ... and their triangles */
    uint32_t path, why_full;  /* as ErSparseInfo */
    uint32_t dirty_nodes2, dirty_nodes8;
    float refit_ms;           /* device time, HIP events, as ErUpdateInfo.refit_ms */
    uint64_t bytes_uploaded;  /* host-to-device bytes of the geometry stage: entries, palettes and the refit's counter words */
    uint64_t influence_bytes; /* the influences, where this call uploaded them (72 x the triangles of the skinned objects), else 0 */
} ErSkinInfo;
int er_skin_info(ErScene* scene, ErSkinInfo* out);

/* Add and remove triangles of a begun scene in place (csrc/er_topology_host.h states the numbering once).
 * The edit is applied in this order: the listed triangles are removed, the given ones appended, then `rest` -- an er_render_edit of the
 * RESULT, so a rest.material_id has the new tri_count entries and overrides the appended ones.  Survivors keep their relative order:
 *   new_id(old) = old - |{r in remove_ids : r < old}|;   appended triangle j gets id survivors + j.
 * A result of 0 triangles is legal.  The contract is er_render_update's: after ER_OK every readable output -- the five planes, samples,
 * RNG, er_get_counters, er_samples_done, er_light_info, er_adaptive_info (off again), er_state_* -- equals, bit for bit, what
 * er_scene_destroy, er_scene_create of the edited description (the current host copy with pending poses flushed, then the three steps
 * above), the same er_update_policy_set and er_render_begin with the same ErRenderParams would give.  The structure equals the fresh
 * one byte for byte (er_debug_read_accel) and ErAccelInfo equals the fresh one except its timings: builder is 0 or 1, never 2, chosen as
 * er_render_begin chooses it.  The render starts over at sample 0; feature planes and id planes are invalidated; the sparse refit's kept
 * boxes are released and the rebuild baseline is forgotten, as after any build; with ER_FLAG_MESH_LIGHTS the emitter table is rebuilt.
 * The counts of ErUpdateInfo, ErEditInfo, ErSparseInfo, ErTransformInfo and ErRebuildInfo do not move: the call has ErTopologyInfo.
 * The object table survives, renumbered: removed ids leave their objects (an object may become empty), the rest copy keeps the surviving
 * rows as er_objects_set saw them, per-object bounds are recomputed from them, and appended triangles are in no object -- unless
 * append_as_object is set and a table is present: they then become a new last object whose rest pose is the arrays given.  A later
 * er_render_transform gives the outputs of the same absolute poses on a fresh scene made from the edited rest arrays with the
 * renumbered table.
 * The geometry store: where the device builder builds, the call keeps the scene's six arrays on the device in id order (140 bytes per
 * triangle) and the next topology edit compacts them there (csrc/er_topology.hip) instead of uploading them again -- path 1, with
 *   bytes_uploaded = 4 x remove_count + 140 x append_count,
 * whatever tri_count is.  Every other call that writes vertices, normals, tangents or material ids (er_render_update,
 * er_render_update_sparse, er_render_transform with GEOMETRY, er_render_edit with GEOMETRY or a material_id, a rest.material_id here),
 * er_render_begin and a failed topology edit release the store; the next topology edit fills it from the host copy (path 2,
 * bytes_uploaded = 140 x tri_count).  Path 0: no store was used -- the host builder built (by size or flag, or because the device builder
 * declined or failed without ER_FLAG_GPU_BUILD), or the store could not be allocated.
 * ER_ERR_STATE unless the scene is begun.  ER_ERR_INVALID_ARG, the scene untouched and still begun: NULL arguments; `what` without a
 * TOPO bit or with unknown bits; a bit with count 0 or without its arrays; a removed id not below tri_count, or listed twice; an
 * appended vertex coordinate that is not finite; ER_EDIT_GEOMETRY in rest.what; anything er_render_edit refuses in `rest`; a material_id
 * (appended, kept, or given in rest) beyond the resulting material list; a resulting triangle count that does not fit 32 bits or that
 * er_scene_create refuses (2^28 and more).  The checks cost O(remove_count log remove_count + append_count) plus what `rest` costs.
 * As in every edit path the host copy is replaced before any device work; if device work then fails the scene is no longer begun and a
 * later er_render_begin builds from the edited copy. */
#define ER_TOPO_REMOVE 1u
#define ER_TOPO_APPEND 2u
typedef struct ErTopologyEdit {
    uint32_t what;                  /* ER_TOPO_* bits, at least one */
    uint32_t remove_count; const uint32_t* remove_ids;    /* REMOVE: ids in the CURRENT numbering, each < tri_count, none twice */
    uint32_t append_count;                                /* APPEND: >= 1 */
    const float *vertices, *normals, *tangents;           /* [append_count][3][3], all required */
    const float *uvs; const float* tangent_sign;          /* [append_count][3][2], [append_count], required */
    const int32_t* material_id;                           /* [append_count], required */
    uint32_t append_as_object;      /* != 0 with an object table present: the appended triangles become a new last object */
    ErSceneEdit rest;               /* what = 0, or any of CAMERA | MATERIALS | TEXTURES | HDRI with er_render_edit's meaning */
} ErTopologyEdit;
typedef struct ErTopologyInfo {
    uint32_t calls;            /* successful er_render_topology calls since er_scene_create */
    uint32_t removed, appended, tri_count;   /* the last one: its two counts and the triangle count it left */
    uint32_t path;             /* 1 = the store was resident, 2 = it was filled from the host copy in this call, 0 = no store used */
    uint32_t texture_stage;    /* of the `rest` part, as ErEditInfo */
    uint64_t bytes_uploaded;   /* host-to-device bytes of the geometry stage (path 0: not counted, 0) */
    float build_ms;            /* the builder's own figure (ErAccelInfo.build_ms) */
    float store_ms;            /* device time of the compaction (HIP events), 0 unless path 1 */
    float edit_ms;             /* host wall time of the call */
    float texture_stage_ms;    /* as ErEditInfo */
} ErTopologyInfo;
int er_render_topology(ErScene* scene, const ErTopologyEdit* edit);
int er_topology_info(ErScene* scene, ErTopologyInfo* out);

/* First-hit feature planes and the denoise guided by them (extension; csrc/er_features.hip gives every float32 operation).
 * er_render_features: a stateless primary-visibility pass over the pixels this rank owns -- n camera rays per pixel (0 -> 4, at most
 * 64; more: ER_ERR_INVALID_ARG) through the production traversal, drawn from the pixel's RNG stream as er_render_begin seeds it, so
 * ray 0 is the camera ray of the render's first sample.  It overwrites two float4 planes (row-major like er_read_pass):
 *   ER_FEATURE_ALBEDO  xyz = mean of the first-hit albedo as the shading step sees it (a miss counts as (1, 1, 1)), w = hits / n
 *   ER_FEATURE_DEPTH   x = y = z = mean distance from the ray origin to Hit.position over the rays that hit (0 if none), w = hits / n
 * The pass reads neither the planes, the sample counts nor the RNG state of the render and writes none of them; its rays are not
 * in ErCounters but in ErFeatureInfo.  Opacity is not drawn: the first hit counts whatever its opacity.  Pending asynchronous work is
 * waited for.  The planes are allocated by the first call (32 bytes per pixel), freed with the scene and not part of er_state_*.
 * er_render_begin and every successful er_render_update invalidate them: er_read_feature, er_gather_feature and er_denoise_guided
 * return ER_ERR_STATE until the pass has run again.  Before er_render_begin all five entry points return ER_ERR_STATE.
 * er_read_feature / er_gather_feature: er_read_pass / er_gather_pass for a feature plane.
 * er_denoise_guided: fills the DENOISE plane like er_denoise, but filters BEAUTY divided by (albedo + 0.01) -- the irradiance, which
 * carries the noise but not the texture detail -- with the colour and NORMAL stops of er_denoise and two more on albedo and depth,
 * and multiplies back.  levels 1..8 (0 -> 5); colour_sigma (0 -> 4: the demodulated signal is several times the radiance),
 * albedo_sigma (0 -> 0.3), depth_sigma (0 -> 0.2, relative).  Negative or NaN: ER_ERR_INVALID_ARG.  On a sharded frame it runs on
 * the rank that BEAUTY, NORMAL and both features have been gathered to since the last sample / feature pass; elsewhere ER_ERR_STATE. */
typedef enum ErFeature { ER_FEATURE_ALBEDO = 0, ER_FEATURE_DEPTH = 1, ER_FEATURE_COUNT = 2 } ErFeature;
typedef struct ErFeatureInfo {
    uint32_t valid;           /* 1 between a feature pass and the next er_render_begin / er_render_update */
    uint32_t samples;         /* n of the last pass */
    uint64_t rays;            /* camera rays it traced: n x the owned pixels inside the frame */
    float ms;                 /* its device time (HIP events) */
} ErFeatureInfo;
typedef struct ErDenoiseGuided {
    uint32_t levels;
    float colour_sigma, albedo_sigma, depth_sigma;
} ErDenoiseGuided;
int er_render_features(ErScene* scene, uint32_t n);
int er_feature_info(ErScene* scene, ErFeatureInfo* out);
int er_read_feature(ErScene* scene, int feature, float* dst_rgba);
int er_gather_feature(ErScene* scene, int feature, ErComm* comm, uint32_t root);
int er_denoise_guided(ErScene* scene, const ErDenoiseGuided* params);

/* Id planes, coverage mattes and picking from a first-hit id pass (extension; csrc/er_ids.h and er_ids.hip).
 * er_render_ids: the rays of er_render_features -- n camera rays per owned pixel (0 -> 4, more than 64: ER_ERR_INVALID_ARG), ray 0 the
 * camera ray of the render's first sample, no opacity draw -- but the ids of what they hit are kept instead of shaded.  The id of a ray
 * that hits, per kind:
 *   ER_ID_TRIANGLE  the scene index of the triangle
 *   ER_ID_OBJECT    the index of the object of the scene's current table (er_objects_set) that lists it; ER_ID_NONE if none does, or
 *                   if the scene has no table
 *   ER_ID_MATERIAL  the triangle's current material_id
 * Per pixel and kind the distinct ids of the rays that hit are ordered by (count descending, id ascending as unsigned); the first
 * ER_ID_SLOTS become the pixel's slots (id, count), unused slots are (ER_ID_NONE, 0).  A hit on geometry in no object is an entry like
 * any other: id ER_ID_NONE, count > 0, last among equal counts.  Misses contribute nothing.  Ids beyond the fourth are dropped and the
 * pixel counts in ErIdInfo.overflow_pixels[kind].  Pixels of other ranks read as empty slots until gathered.
 * Like the feature pass it reads neither planes, sample counts, RNG nor counters of the render and writes none of them; its rays are
 * in ErIdInfo, not in ErCounters.  Pending asynchronous work is waited for.  The planes are allocated by the first call (96 bytes per
 * pixel), freed with the scene and not part of er_state_*.  er_render_begin, every successful er_render_update, er_render_edit,
 * er_render_update_sparse and er_render_transform, and a successful er_objects_set invalidate them: er_read_ids, er_gather_ids,
 * er_id_matte and er_pick_rect return ER_ERR_STATE until the pass has run again.  Before er_render_begin all seven entry points return
 * ER_ERR_STATE; NULL arguments and a kind out of range are ER_ERR_INVALID_ARG.
 * er_read_ids: both planes of one kind, row-major, [y_res * x_res][ER_ID_SLOTS] each; either destination may be NULL, not both.
 * er_gather_ids: er_gather_feature for both planes of one kind.
 * er_id_matte: dst[p] = (float)(sum of the counts of pixel p's slots whose id is in the list) / (float)n, computed on the device.  The
 * list is a set: duplicates are allowed and ER_ID_NONE is a legal member; count 0 or a NULL list: ER_ERR_INVALID_ARG.  It reads the
 * planes as they lie: ungathered pixels give 0.
 * er_pick_rect: the distinct ids with count > 0 in any slot of any pixel of the half-open rectangle [x0, x1) x [y0, y1), ascending as
 * unsigned, reduced on the device; at most `capacity` of them are written, *count is the number found (ids may be NULL with capacity
 * 0 to ask for it).  x0 >= x1, y0 >= y1, x1 > x_res or y1 > y_res: ER_ERR_INVALID_ARG.
 * er_pick: needs a begun scene only, no id pass.  It traces ray 0 of pixel (x, y) -- any pixel of the frame, whichever rank owns it
 * -- and reports what it hits; the object comes from the current table, also right after er_render_transform.  It leaves the render's
 * state, its counters and the id planes alone.  x or y outside the frame: ER_ERR_INVALID_ARG. */
#define ER_ID_NONE  0xFFFFFFFFu
#define ER_ID_SLOTS 4
typedef enum ErIdKind { ER_ID_TRIANGLE = 0, ER_ID_OBJECT = 1, ER_ID_MATERIAL = 2, ER_ID_KIND_COUNT = 3 } ErIdKind;
typedef struct ErIdInfo {
    uint32_t valid;           /* 1 between an id pass and whatever invalidates it (above) */
    uint32_t samples;         /* n of the last pass */
    uint64_t rays;            /* camera rays it traced: n x the owned pixels inside the frame */
    float ms;                 /* its device time (HIP events) */
    uint32_t objects;         /* object count of the table the OBJECT plane was made with (0: none) */
    uint32_t overflow_pixels[ER_ID_KIND_COUNT];   /* owned pixels with more than ER_ID_SLOTS distinct ids of that kind */
} ErIdInfo;
typedef struct ErPick {
    uint32_t hit, triangle, object, material;     /* a miss: 0, ER_ID_NONE x 3, every float 0 */
    float distance;           /* length(Hit.position - ray.o): the operations of ER_FEATURE_DEPTH */
    float position[3];        /* Hit.position */
    float uv[2];              /* the texture coordinates the shading step sees */
} ErPick;
int er_render_ids(ErScene* scene, uint32_t n);
int er_id_info(ErScene* scene, ErIdInfo* out);
int er_read_ids(ErScene* scene, int kind, uint32_t* ids /*[y_res * x_res][ER_ID_SLOTS]*/, uint32_t* counts /*the same shape*/);
int er_gather_ids(ErScene* scene, int kind, ErComm* comm, uint32_t root);
int er_id_matte(ErScene* scene, int kind, const uint32_t* ids, uint32_t count, float* dst /*[y_res * x_res]*/);
int er_pick_rect(ErScene* scene, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, int kind, uint32_t* ids, uint32_t capacity, uint32_t* count);
int er_pick(ErScene* scene, uint32_t x, uint32_t y, ErPick* out);

/* Keeping the image across camera moves and object poses by temporal reprojection (extension; csrc/er_reproject.h and er_history.hip;
 * DESIGN.md 3l).  A display-side aid like the DENOISE plane: the render's planes, sample counts, RNG and counters are neither read for
 * anything but the colour nor written, so a render with these calls in between is, bit for bit, the render without them.
 * A KEY PLANE holds one pinhole ray per pixel through the production traversal -- camera_ray with r1 = r2 = 0.5 and bokeh taken as 0, so
 * pixel x samples continuous coordinate x exactly --: a hit flag, the object of the current table (ER_ID_NONE if the triangle is in no
 * object or there is no table), the distance length(Hit.position - ray.o), Hit.position, and for a miss the ray's direction.
 * er_history_capture (before an edit): makes the key plane of the scene as it is now unless the previous resolve left one that is still
 * current (same camera and poses, bit for bit), stores the camera and every object's pose, and per pixel a colour C and a weight W: with
 * n = samples - 1 and m = BEAUTY.rgb * ((float)samples / (float)n) for n > 0,  C = (w H + n m) / (w + n)  where (H, w) is the pixel's
 * resolved history if one is valid (else w = 0), C = 0 if w + n = 0;  W = min(w + n, max_weight).  History therefore accumulates over
 * a sequence of edits.  params may name 0 for a default (depth_tolerance 0.02, relative; max_weight 32).
 * er_history_resolve (after it): makes the key plane of the scene as it is now and keeps it for the next capture.  For a pixel that
 * hits, P_old = B_o P_new with B_o = M_capture o M_now^-1 of the pixel's object (computed on the host in double, rounded to float once);
 * objects whose two poses are bitwise equal, and ER_ID_NONE, take P_old = P_new bit for bit.  For a pixel that misses, P_old = the old
 * camera position + the ray's direction.  P_old is projected through the captured camera to continuous pixel coordinates (invalid if
 * the point is not in front of the camera or a coordinate is not finite), and four bilinear taps are taken around them.  A tap is valid
 * if it is inside the frame, the captured key there has the same hit flag and, for hits, the same object and
 * |d_exp - d_old| <= depth_tolerance * d_exp, d_exp = |P_old - old camera position|.  History rgb and w are the bilinear means of C and
 * W over the valid taps, weights renormalised; w = 0 if no tap is valid.  Every pixel is in exactly one class of ErHistoryInfo: sky (it
 * misses), valid (four valid taps), partial (one to three), offscreen (no tap inside the frame), rejected (the rest).
 * er_read_history: rgb = the reprojected colour, a = the carried weight w (0: none).
 * er_read_blended: (w H + n m) / (w + n) per pixel from the current BEAUTY and sample counts, alpha 1; the setup colour where w + n = 0.
 * A changed camera keeps a capture, through any edit path; so do er_render_transform and er_render_samples.  er_render_begin,
 * er_render_topology, er_objects_set, er_state_import, every direct geometry edit (er_render_update / _sparse / er_render_edit with the
 * geometry bit) and every materials, textures or HDRI edit drop the capture and the resolved history: er_history_resolve and the two
 * reads then return ER_ERR_STATE.
 * ER_ERR_STATE: the scene is not begun; resolve without a capture; a read without a resolve; world > 1 (a sharded frame would need the
 * old pixels of other ranks: not built).  ER_ERR_INVALID_ARG: NULL arguments; negative or NaN parameters.
 * Stated limits: view-dependent shading and moved shadows go stale, bounded by max_weight; the first hit counts regardless of opacity,
 * as in the feature pass.  The planes (80 bytes per pixel) are allocated by the first capture, freed with the scene and not part of
 * er_state_*. */
typedef struct ErHistoryParams {
    float depth_tolerance;    /* 0 -> 0.02: relative */
    float max_weight;         /* 0 -> 32: cap on the carried sample weight */
} ErHistoryParams;
typedef struct ErHistoryInfo {
    uint32_t captured, resolved;      /* a capture is held / a history plane is valid */
    uint32_t moved_objects;           /* objects whose pose differs between capture and resolve */
    uint64_t pixels_valid, pixels_partial, pixels_offscreen, pixels_rejected, pixels_sky;   /* of the last resolve */
    float capture_ms, resolve_ms;     /* device time of the last capture / resolve (HIP events) */
} ErHistoryInfo;
int er_history_capture(ErScene* scene, const ErHistoryParams* params);
int er_history_resolve(ErScene* scene);
int er_history_info(ErScene* scene, ErHistoryInfo* out);
int er_read_history(ErScene* scene, float* dst_rgba);
int er_read_blended(ErScene* scene, float* dst_rgba);

/* A variance plane by batch means and the denoise guided by it (extension; csrc/er_variance.h gives every float32 operation, csrc/
 * er_variance.hip the kernels).  Stateless with respect to the render like the feature, id and history passes: the render's
 * planes, sample counts, RNG and ErCounters are read and never written; only DENOISE is written, as the other two filters do.
 * A pixel's BEAUTY is a running mean with a known count, so the mean of the samples between two read points follows from the two plane
 * values, and the scatter of those batch means estimates the variance.  Per pixel the library keeps 12 words (48 bytes): a snapshot S
 * (rgb) with its count m, the weighted mean mu (rgb) of the batch means with the total weight W, M2 (rgb) and the batch count K.
 * RESET: S, m = the pixel's BEAUTY rgb and sample count as they stand -- (0, 0, 0) and 1 right after er_render_begin or an edit, so the
 * first fold's batch is everything since the start --, mu = M2 = 0, W = 0, K = 0.  er_render_begin, every successful er_render_update,
 * er_render_update_sparse, er_render_edit, er_render_transform and er_render_topology, and er_state_import (the snapshot is taken from
 * the imported planes) reset every pixel and `folds`.  er_render_samples, er_render_features, er_render_ids and the history calls leave
 * the state alone.
 * er_variance_fold: waits for pending asynchronous work, then per pixel with I = BEAUTY rgb, M = its sample count, n = M - m:
 *   n == 0 (a tile the adaptive sampler stopped, a pixel whose samples were all gated): all 12 words stay.  Otherwise per channel
 *     J = (I * (float)M - S * (float)m) / (float)n;   W' = W + (float)n;   d = J - mu;   mu' = mu + d * ((float)n / W');
 *     M2' = M2 + (float)n * (d * (J - mu'));   then K' = K + 1, S = I, m = M         (West's weighted update: E[M2] = (K - 1) sigma^2)
 * er_read_variance: xyz = the variance of BEAUTY as stored, at the current count M: (0, 0, 0) if K < 2, else
 *   max(0, ((M2 / (float)(K - 1)) * (float)(M - 1)) / ((float)M * (float)M));  w = (float)K.  Row-major like er_read_pass.  Samples
 *   rendered after the last fold change M but not the moments.
 * er_denoise_variance: er_denoise_guided's demodulation, stencil, normal, albedo and depth stops, with the colour stop normalised per
 *   pixel: the squared difference of each channel is divided by the 3 x 3 binomial mean of the demodulated variance v / (albedo + 0.01)^2
 *   around the centre (+ 1e-8), wc = 1 / (1 + d2 / colour_sigma^2) -- colour_sigma counts standard errors and is not tightened per level,
 *   because the variance is propagated through the levels instead: ve' = sum(wgt^2 ve_q) / (sum wgt)^2.  A centre with K < 2 takes
 *   wc = 1.  levels 1..8 (0 -> 5); colour_sigma (0 -> 6), albedo_sigma (0 -> 0.3), depth_sigma (0 -> 0.2, relative).  It needs valid
 *   feature planes, exactly as er_denoise_guided does, and folds >= 2 since the last reset; otherwise ER_ERR_STATE.
 * ER_ERR_STATE from all four: the scene is not begun; world > 1 (variance on a sharded frame is not built).  ER_ERR_INVALID_ARG: NULL
 * arguments; more than 8 levels; a negative or NaN sigma.  Adaptive sampling may be on: the arithmetic is per pixel with per-pixel counts.
 * Stated limit: J is a difference of two products, its rounding error relative to I about 2^-23 * M / n -- harmless at interactive
 * counts; a render of thousands of samples should fold in batches that grow with M.  The state is allocated by the first use (48 bytes
 * per pixel), freed with the scene and not part of er_state_*. */
typedef struct ErVarianceInfo {
    uint32_t folds;               /* since the last reset */
    uint32_t reserved;
    uint64_t pixels_folded;       /* by the last fold: pixels with n > 0 */
    uint64_t pixels_known;        /* pixels with K >= 2 after it */
    float fold_ms, filter_ms;     /* device time of the last fold / er_denoise_variance (HIP events) */
} ErVarianceInfo;
typedef struct ErDenoiseVariance {
    uint32_t levels;
    float colour_sigma, albedo_sigma, depth_sigma;
} ErDenoiseVariance;
int er_variance_fold(ErScene* scene);
int er_variance_info(ErScene* scene, ErVarianceInfo* out);
int er_read_variance(ErScene* scene, float* dst_rgba);
int er_denoise_variance(ErScene* scene, const ErDenoiseVariance* params);

/* The variance carried through the history, the variance of the blend and the denoise of the blended frame (extension; csrc/
 * er_history_variance.h gives every float32 operation, csrc/er_history_variance.hip the kernels).  Display-side like both
 * parents: the render's planes, sample counts, RNG and ErCounters are read and never written; only DENOISE is written.  Every output of
 * every other entry point is, bit for bit, what it is without these calls.
 * West's moments give the variance of ONE sample of a pixel, s2 = M2 / (float)(K - 1) per channel (values not > 0, a NaN too, become 0),
 * known where K >= 2; a pending reset of the variance state or a state that was never allocated is K = 0 everywhere.
 * POOL of (s2_H, k_H, w) and (s2_C, k_C, n), n = (float)(samples - 1):  useH = k_H && w > 0, useC = k_C && n > 0;  both:
 * (w * s2_H + n * s2_C) / (w + n) per channel;  one: that one, bit for bit;  none: 0 and flag 0.
 * er_history_capture also writes, if the scene's variance state is allocated (an er_variance_fold or er_read_variance has run), a plane
 * SV = (pool.rgb, flag) per pixel: the pixel's resolved history variance HV with the history weight w, pooled with its current variance
 * with n; without a resolved history w = 0 and k_H = 0.  er_history_resolve, when the held capture carries SV, takes the colour's four
 * taps once and also writes HV = (rgb, flag): the mean of SV.rgb over the taps that are valid and whose SV flag is set, with the
 * colour's tap weights renormalised over those taps (a plain mean, accumulated in the colour's order); flag 1 if their weights sum to
 * more than 0, else all four words 0.  The history plane and the five class counts are the same bits with and without SV.
 * er_read_history_variance: HV; a plane of zeros if the capture carried nothing.
 * er_read_blended_variance: VB, the variance of er_read_blended's colour:  (s2, k) = pool(HV, w, current, n);  VB.rgb = s2 / (w + n)
 *   where k is set and w + n > 0, else 0;  a = k.
 * er_denoise_blended: fills DENOISE from the blend.  e = blend.rgb / (albedo + 0.01), ve = VB.rgb / ((albedo + 0.01) * (albedo + 0.01))
 *   with ve.w = VB's flag, then er_denoise_variance's levels unchanged and its join with the blend's alpha (1).  It needs a resolved
 *   history and valid feature planes of the current scene state, NOT two folds: a pixel whose flag is 0 is filtered with wc = 1.
 *   Parameters, defaults and argument checks are er_denoise_variance's.
 * The two planes (32 bytes per pixel) live and die with the capture: whatever drops a capture drops them.  They are allocated by the
 * first capture that carries variance, freed with the scene and not part of er_state_*.
 * ER_ERR_STATE: the scene is not begun; world > 1; a read or the filter without a resolved history; the filter without feature planes.
 * ER_ERR_INVALID_ARG: NULL arguments; more than 8 levels; a negative or NaN sigma.
 * Stated limits: the cap W = min(w + n, max_weight) makes s2 / w overstate the variance of a long history, and bilinear taps average up
 * to four pixels, which the carried variance ignores: both err towards smoothing.  A per-sample variance is view-dependent and goes stale
 * as the colour does. */
typedef struct ErHistoryVarianceInfo {
    uint32_t captured, resolved;          /* the held capture carries SV / the resolved history carries HV */
    uint64_t pixels_known_captured;       /* SV flag set, last capture */
    uint64_t pixels_known_history;        /* HV flag set, last resolve */
    uint64_t pixels_known_blended;        /* VB flag set, last er_denoise_blended or er_read_blended_variance */
    float filter_ms;                      /* device time of the last er_denoise_blended (HIP events) */
} ErHistoryVarianceInfo;
int er_history_variance_info(ErScene* scene, ErHistoryVarianceInfo* out);
int er_read_history_variance(ErScene* scene, float* dst_rgba);
int er_read_blended_variance(ErScene* scene, float* dst_rgba);
int er_denoise_blended(ErScene* scene, const ErDenoiseVariance* params);

/* ---- Seeing through cut-outs in the first-hit passes.  The render passes a path straight through a hit that fails its
 * opacity draw and shades what lies behind; the first-hit camera pass (er_render_features, er_render_ids, er_pick, the key plane of
 * er_history_capture / er_history_resolve) by default reports the first hit whatever its opacity.  With `cutouts` set a camera ray of
 * these four goes on through hits the render would mostly pass through and reports the first surface that stops it:
 *   along the ray take the closest hit; its opacity is the material's constant or the first channel of the opacity texture through its
 *   filter at the hit's uv (what the render shades with); the hit STOPS the ray iff opacity >= threshold (a NaN opacity passes);
 *   otherwise the ray goes on as the render's does, from position + d * 0.001 along d, with no self-exclusion.  At most max_bounces
 *   hits are examined (a path of the render ends there): if all of them pass, the ray is a miss (rays_capped).  A ray that passes and
 *   then leaves the scene is a miss (rays_through_to_miss).  Distances (DEPTH, the key's dist, ErPick::distance) are measured from the
 *   CAMERA ray's origin.  Each consumer does with the surviving hit what it does with the first hit otherwise.
 * The rule is deterministic -- a threshold, not the render's draw, because a guide plane must be free of noise -- and takes no RNG
 * draw: binary cut-outs are exact under it, a semi-transparent sheet goes to the majority.
 * opacity_threshold: 0 means 0.5; otherwise in (0, 1].  cutouts: 0 (the default: every output is bit for bit what it is without this
 * call) or 1; any other value is refused.
 * A successful er_first_hit_set that changes either field invalidates the feature planes, the id planes and the history (a capture
 * keyed under one rule cannot be resolved under the other); one that changes nothing invalidates nothing.  The setting survives
 * er_render_update, _edit, _transform, _topology and a second er_render_begin.  The render itself (BEAUTY, samples, RNG, ErCounters) is
 * the same with and without the mode.
 * ErFirstHitInfo: the setting (the threshold as resolved: 0.5 for 0) and five counters of the last whole-frame pass run in this mode
 * (features, ids or key, whichever ran last; on a sharded frame the rank's own rays): rays traced; rays_through, those that passed at
 * least one hit; layers_skipped, the hits passed, summed; rays_capped; rays_through_to_miss.  All five are 0 while the mode is off.
 * ER_ERR_STATE: the scene is not begun.  ER_ERR_INVALID_ARG: NULL arguments; cutouts > 1; a NaN, negative or > 1 threshold (the scene
 * is left untouched). */
typedef struct ErFirstHitParams {
    uint32_t cutouts;
    float opacity_threshold;
} ErFirstHitParams;
typedef struct ErFirstHitInfo {
    uint32_t cutouts;
    float opacity_threshold;
    uint64_t rays, rays_through, layers_skipped, rays_capped, rays_through_to_miss;
} ErFirstHitInfo;
int er_first_hit_set(ErScene* scene, const ErFirstHitParams* params);
int er_first_hit_info(ErScene* scene, ErFirstHitInfo* out);

#ifdef __cplusplus
}
#endif
#endif /* ELEVEN_HIP_H */
