/* eleven_hip_debug.h -- host-only inspection hooks of libeleven_hip.so (no GPU needed).
 * Not part of the drop-in boundary; used by the CPU test-suite to validate the library's own
 * acceleration-structure builder, which replaces Scene::buildBVH / BVH::build
 * (reference src/Scene.cpp:122-143, src/BVH.cpp:132-415). */
#ifndef ELEVEN_HIP_DEBUG_H
#define ELEVEN_HIP_DEBUG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ErBvhCheck {
    uint32_t node_count, leaf_count, max_depth, max_leaf_size;
    uint32_t tris_in_leaves;       /* must equal tri_count */
    uint32_t duplicate_tris;       /* triangles referenced more than once: must be 0 */
    uint32_t uncontained;          /* vertices outside their leaf's box, or child boxes outside the parent's: must be 0 */
    uint32_t unreachable_nodes;    /* must be 0 */
    float lift_bound;
    float build_ms;
    double sah_cost;               /* sum over inner nodes of child-area * child-count / root area */
} ErBvhCheck;

/* Builds the BVH for [tri_count][3][3] vertices/normals exactly as er_render_begin does and checks its invariants. */
int er_debug_bvh_check(const float* vertices, const float* normals, uint32_t tri_count, int threads, ErBvhCheck* out);

/* The acceleration structure itself, byte for byte, for a checker outside the library (tests/accel_check.py).  Both hooks below
 * only copy: they judge nothing.  Layouts (elevenrender_amd/csrc/er_bvh.h): binary nodes ErNode, 64 bytes each, root = node 0; wide
 * nodes ErNode8, 80 bytes at the start of every node8_pieces x 16 bytes; intersection records ErTriIsect, 48 bytes, tri_count + 1 of them
 * (the last one is the zero record the paired triangle fetch of the wide traversal may read); attribute records ErTriAttr at the
 * start of every attr_pieces x 16 bytes. */
typedef struct ErAccelDump {
    uint32_t tri_count;
    uint32_t node_count;           /* binary nodes */
    uint32_t node8_count;          /* wide nodes */
    uint32_t node8_pieces;         /* stride of the wide nodes in 16-byte pieces (ER_NODE8_PIECES) */
    uint32_t attr_pieces;          /* stride of the attribute records in 16-byte pieces (ER_ATTR_PIECES); 0: no records (er_debug_bvh_dump) */
    uint32_t max_depth;            /* levels of inner nodes of the binary tree (what ER_BVH_MAX_DEPTH bounds) */
    uint32_t max_depth8;           /* levels of the wide tree (what ER_STACK8 bounds; ErAccelInfo::max_depth) */
    uint32_t builder;              /* 0 = host build, 1 = device build */
    float lo[3], hi[3];            /* scene bounds as the builder reported them */
    float lift_bound;              /* the builder's bound on |shadingPosition - geomPosition| over all triangles */
    float max_lift;                /* the same bound as the kernels' scene descriptor carries it */
} ErAccelDump;

/* The structure as it lies in DEVICE memory after er_render_begin, whichever builder made it (before: ER_ERR_STATE).  `info` is always
 * filled.  With all four buffers NULL that is all (the size query: nodes need node_count * 64 bytes, nodes8 node8_count * node8_pieces * 16,
 * isect (tri_count + 1) * 48, attr tri_count * attr_pieces * 16); otherwise every non-NULL buffer receives its array, and a capacity
 * (in bytes) smaller than the array is ER_ERR_INVALID_ARG.  A copy made on request: nothing is kept for it by er_render_begin. */
struct ErScene;
int er_debug_read_accel(struct ErScene* scene, ErAccelDump* info, void* nodes, uint64_t nodes_cap, void* nodes8, uint64_t nodes8_cap,
                        void* isect, uint64_t isect_cap, void* attr, uint64_t attr_cap);

/* The HOST builder's output for [tri_count][3][3] vertices / normals (er_build_bvh, run exactly as er_debug_bvh_check runs it; no device
 * needed): nodes, packed wide nodes (node8_pieces = 5), slot_to_tri[tri_count] and tri_lift[tri_count] (per ORIGINAL triangle id) in place
 * of the records.  Same protocol: all four buffers NULL = size query; capacities in bytes. */
int er_debug_bvh_dump(const float* vertices, const float* normals, uint32_t tri_count, int threads, ErAccelDump* info, void* nodes, uint64_t nodes_cap,
                      void* nodes8, uint64_t nodes8_cap, uint32_t* slot_to_tri, uint64_t slot_cap, float* tri_lift, uint64_t lift_cap);

/* The terms behind er_accel_cost (csrc/er_cost.h).  The sums of either hook are in `sums` (node_area, leaf_area, tri_area,
 * cost; ms = device time, 0 on the host); node_terms receives 2 doubles per wide node (node_i, leaf_i), tri_terms one float per
 * triangle record (tri_k); either may be NULL, capacities in bytes, a capacity smaller than the array is ER_ERR_INVALID_ARG.
 * er_debug_accel_cost_terms: a measurement of the begun scene's structure in device memory, run for this call (er_accel_cost's kept
 * result is neither used nor replaced; the arithmetic is bitwise reproducible, so the sums equal its).  Before er_render_begin: ER_ERR_STATE.
 * er_debug_accel_cost_host: the host compilation of the same header over caller-supplied arrays in the layouts of er_debug_bvh_dump /
 * er_debug_read_accel -- wide nodes at a stride of node8_pieces x 16 bytes, tri_count intersection records; no device needed.  The
 * terms are the device's bit for bit; the sums are added sequentially, ascending. */
typedef struct ErCostSumsDebug {
    double node_area, leaf_area, tri_area, cost;
    float ms; uint32_t reserved;
} ErCostSumsDebug;
int er_debug_accel_cost_terms(struct ErScene* scene, ErCostSumsDebug* sums, double* node_terms, uint64_t node_cap, float* tri_terms, uint64_t tri_cap);
int er_debug_accel_cost_host(const void* nodes8, uint32_t node8_count, uint32_t node8_pieces, const void* isect, uint32_t tri_count, ErCostSumsDebug* sums,
                             double* node_terms, uint64_t node_cap, float* tri_terms, uint64_t tri_cap);

/* Runs the library's HDRI CDF search (elevenrender_amd/csrc/er_cdf.h, the replacement of the 21-level
 * HDRI::binarySearch, reference src/HDRI.cpp:85-98) on the host for `count` values. */
int er_debug_cdf_search(const float* cdf, int length, const float* values, int32_t* out, int count);

/* Closest hit of `n` arbitrary rays (origins/dirs [n][3]; directions taken as given) through the library's exact
 * traversal routine on the GPU, under the reference's metric (src/BVH.cpp:105-120): original triangle id (-1 = miss),
 * Hit.position and |Hit.position - origin|.  Needs a scene on which er_render_begin has succeeded.  Used by the
 * function-level parity test against the oracle's throwRay. */
struct ErScene;
int er_debug_closest_hit(struct ErScene* scene, const float* origins, const float* dirs, uint32_t n, int32_t* tri_ids, float* positions, float* distances);

/* The same query through the PRODUCTION traversal -- the 8-wide interval traversal of er_wf_trace / the streaming tracer waves
 * (csrc/er_trav.h: trav_choose / trav_fetch / trav_apply) followed by resolve_closest / resolve_shadow -- for `n`
 * arbitrary rays (directions taken as given).
 *   self_slots == NULL: closest-hit queries.  tri_ids = original triangle id (-1 miss), slots = the library's internal
 *     triangle handle (feed it back as self_slots), positions = Hit.position, distances = |Hit.position - origin|
 *     (inf on a miss), info = 0 one surviving candidate, 1 two survivors decided by the exact metric, 2 more than two:
 *     exact re-trace.
 *   self_slots != NULL: shadow queries, the reference's "occluded iff the closest hit is a triangle other than the one
 *     the ray leaves" (src/kernel.cpp:555-562) in the form the kernels use: occluded iff some triangle other than
 *     self_slots[i] (-1: none is exempt) is hit nearer than limits[i].  tri_ids = 1 occluded / 0 not; info = 0 / 1
 *     decided by the t-intervals, 2 exact metric of the candidates, 3 exact re-trace. */
int er_debug_trace_rays(struct ErScene* scene, const float* origins, const float* dirs, uint32_t n, const int32_t* self_slots,
                        const float* limits, int32_t* tri_ids, int32_t* slots, float* positions, float* distances, int32_t* info);

/* er_debug_trace_rays, and what the queries left in the traversal's HBM spill area.  A lane's stack keeps its first *lds_levels entries
 * (WF_LDS_STACK as compiled) in LDS and the deeper ones in its own column of the spill area, *stack_levels (ER_STACK8 as compiled)
 * levels in all.  The call fills the area with 0xFF bytes before the launch (no entry has that value) and reads it back after it:
 * spill_levels[i] = the leading levels of ray i's column that were written, so ray i's stack reached *lds_levels + spill_levels[i]
 * entries.  ER_ERR_STATE (the rays' results are delivered all the same) if an entry lies above an unwritten level of its column, at
 * level (wide depth - *lds_levels) or above, or in the column of a lane that had no ray. */
int er_debug_trace_rays_levels(struct ErScene* scene, const float* origins, const float* dirs, uint32_t n, const int32_t* self_slots,
                               const float* limits, int32_t* tri_ids, int32_t* slots, float* positions, float* distances, int32_t* info,
                               uint32_t* spill_levels, uint32_t* lds_levels, uint32_t* stack_levels);

/* The judgement er_debug_trace_rays_levels passes on the spill area it read back, on a caller's buffer (host code, no device): `spilled`
 * holds ceil(n / 64) regions of *stack_levels levels x 64 lanes x 2 words, filled with 0xFF bytes where nothing was written; `usable` is
 * the wide depth minus *lds_levels.  levels[i] = the leading written levels of ray i's column; ER_ERR_STATE as described above. */
int er_debug_spill_levels(const void* spilled, uint64_t spilled_bytes, uint32_t n, uint32_t usable, uint32_t* levels);

/* One record per executed bounce-loop iteration (reference src/kernel.cpp:508-592); the same fields, in the same order, as the oracle's
 * OracleTraceRec begins with (oracle/er_oracle.h; the oracle's record goes on with fields of its own). */
typedef struct ErTraceRec {
    int32_t bounce;
    int32_t tri;            /* ORIGINAL triangle id of the closest hit, -1 = miss */
    int32_t shadow_tri;     /* original id of the HDRI shadow ray's closest hit, -1 = none / not traced */
    int32_t opaque;         /* 1 if the opacity test passed */
    float position[3];      /* Hit.position */
    float wi[3];            /* next ray direction */
    float light[3];         /* accumulated radiance after this iteration */
    float reduction[3];     /* throughput after this iteration */
    int32_t shadow_occ;     /* HDRI shadow query: 1 occluded, 0 visible, -1 not traced */
    int32_t light_occ;      /* point-light / emitter query (ER_FLAG_POINT_LIGHTS / ER_FLAG_MESH_LIGHTS): 1 occluded, 0 visible, -1 none */
} ErTraceRec;

/* Runs ONE more sample of pixel idx -- bounce_step (csrc/er_shade.h) over the production traversal, every query traced
 * at once -- and records up to max_recs iterations.  The pixel's planes, sample count and RNG advance exactly as by
 * er_render_samples(scene, 1) restricted to that pixel.  *count = records written. */
int er_debug_trace_pixel(struct ErScene* scene, uint32_t idx, ErTraceRec* recs, int max_recs, int* count);

/* The emitter table of ER_FLAG_MESH_LIGHTS (er_light_info gives its length): for the first min(emitters, cap) entries, in table
 * order (ascending triangle slot), the emitter's INPUT triangle index (ErSceneDesc order, mapped back through the BVH builder's
 * permutation) and its CDF entry.  Either output may be NULL.  Before er_render_begin: ER_ERR_STATE. */
int er_debug_read_light_table(struct ErScene* scene, int32_t* tri_index, float* cdf, uint32_t cap);
/* The same, and in `prob` P of each entry: the value the table holds at the emitter's triangle slot (w / W), which the shading step
 * reads for p_L of an emitter sample and of a BRDF-sampled hit (csrc/er_shade.h rules 5 and 7).  Any output may be NULL. */
int er_debug_read_light_table_prob(struct ErScene* scene, int32_t* tri_index, float* cdf, float* prob, uint32_t cap);

/* The row and column tables of the HDRI's next-event sample directions (csrc/er_hdri_trig.h), copied as they lie on the device:
 * `cols` receives 4 words per column -- px, pz, bits(ix), iu --, `rows` 6 words per row -- py, a, bits(iy), sin_pdf, iv, sin_row --
 * for the first min(width, col_cap) columns and min(height, row_cap) rows of the begun scene's HDRI.  Either output may be NULL.
 * The tables are there whether or not ER_HDRI_TRIG_ON_DEVICE kept the kernels from reading them.  Before er_render_begin: ER_ERR_STATE. */
int er_debug_read_hdri_trig(struct ErScene* scene, uint32_t* cols, uint32_t col_cap, uint32_t* rows, uint32_t row_cap);
/* The same entries evaluated on the HOST for a width x height HDRI (the fill kernel's twin: one implementation of every function for
 * both sides): `cols` holds 4 * width words, `rows` 6 * height words.  Needs no device. */
int er_debug_hdri_trig_host(int32_t width, int32_t height, uint32_t* cols, uint32_t* rows);

/* The DEVICE functions of the path, one call per item, for known-answer tests against the oracle's function-level entry
 * points (SURVEY.md section 4 level 1: a1 RNG, a3 camera, a5 Tri::hit record, a6-a8 textures and mappings, a9 HDRI search /
 * pdf, a10-a12 Disney sample / eval / pdf, the transcendentals).  `in` holds n items of in_stride floats, `out` receives n
 * items of out_stride floats (integers travel as float BITS).  Needs a scene on which er_render_begin has succeeded (the
 * camera, textures, HDRI and triangles are the scene's).  Kinds and layouts:
 *   ER_FN_RNG            in [bits(pixel idx)]                          out [16 x next(), 16 x bits(state)]        (32)
 *   ER_FN_CAMERA_RAY     in [x, y, r1, r2, r3, r4, r5]                 out [origin(3), dir(3)]                    (6)
 *   ER_FN_TRI_HIT        in [bits(original tri id), origin(3), dir(3)] out [valid, position(3), normal(3), gnormal(3),
 *                                                                           tangent(3), bitangent(3), tu, tv]     (18)
 *   ER_FN_DISNEY_EVAL    in [hd(20), V(3), N(3), L(3)]                 out [rgb]                                  (3)
 *   ER_FN_DISNEY_PDF     in [hd(20), V(3), N(3), L(3)]                 out [pdf]                                  (1)
 *   ER_FN_DISNEY_SAMPLE  in [hd(20), V(3), N(3), r1, r2, r3]           out [dir(3)]                               (3)
 *     hd = metallic, roughness, clearcoatGloss, clearcoat, anisotropic, transmission, specular, specularTint, sheenTint,
 *          subsurface, sheen, albedo(3), tangent(3), bitangent(3)   -- the oracle's layout (oracle/er_oracle.h)
 *   ER_FN_SPHERICAL      in [p(3)]                                     out [u, v]                                 (2)
 *   ER_FN_REV_SPHERICAL  in [u, v]                                     out [p(3)]                                 (3)
 *   ER_FN_TEXTURE        in [bits(texture id, -1 = the HDRI), u, v, filtered(0/1)]   out [rgb]                    (3)
 *                        (ER_ERR_STATE for a texture the library keeps compacted on the device -- one channel, possibly to the
 *                        power 2.2, er_render_begin -- since a fetch from that entry is not a fetch from the scene's texture;
 *                        begin the render with ER_TEX_COMPACT=0 in the environment to evaluate such a texture)
 *   ER_FN_HDRI_SEARCH    in [value]                                    out [bits(index)]                          (1)
 *   ER_FN_HDRI_PDF       in [bits(x), bits(y)]                         out [pdf]                                  (1)
 *   ER_FN_MATH           in [bits(op: 0 sin 1 cos 2 acos 3 log 4 pow 5 atan2), x, y]   out [value]                (1)
 *   ER_FN_MESH_PICK      in [r]                                        out [bits(table index), bits(input triangle)] (2)
 *                        (mesh_pick and mesh_slot of csrc/er_shade.h on the begun scene's emitter table; ER_ERR_STATE unless the
 *                        render was begun with ER_FLAG_MESH_LIGHTS and the table is non-empty) */
enum { ER_FN_RNG = 0, ER_FN_CAMERA_RAY, ER_FN_TRI_HIT, ER_FN_DISNEY_EVAL, ER_FN_DISNEY_PDF, ER_FN_DISNEY_SAMPLE, ER_FN_SPHERICAL,
       ER_FN_REV_SPHERICAL, ER_FN_TEXTURE, ER_FN_HDRI_SEARCH, ER_FN_HDRI_PDF, ER_FN_MATH, ER_FN_MESH_PICK, ER_FN_COUNT };
int er_debug_eval(struct ErScene* scene, int kind, const float* in, uint32_t n, uint32_t in_stride, float* out, uint32_t out_stride);

/* Loopback transport for er_gather_pass: `world` communicators that live in ONE process and move the packed buffers
 * through device-to-device copies, so that pack -> exchange -> unpack can be driven on a one-GPU box without RCCL (which
 * refuses two ranks on one GPU).  out[world].  Call er_gather_pass for the non-root ranks first, then for the root. */
struct ErComm;
int er_debug_comm_create_local(uint32_t world, struct ErComm** out);

/* What the streaming schedule ran the last completed call with, and what it read from it (er_stream_host.cpp stream_adapt): for bench.py's
 * `projected` block and the tests.  Valid after er_wait / a read-back; all zero for the other schedules. */
typedef struct ErStreamInfo {
    uint32_t waves, tracers;       /* waves per workgroup (16 or 12) and how many of them trace */
    uint32_t large_regions;        /* 1: the deal of 16 x 16-tile screen regions per XCD is in use; 0: the default 8 x 8 one */
    uint32_t deal_pending;         /* 1: the deal is still to be decided (no call has completed) */
    uint32_t launches;             /* kernel launches of this render so far */
    uint32_t pixels_per_cu;        /* owned pixels per workgroup (tiles x 64 / workgroups) */
    double lanes_busy;             /* share of the tracer waves' lanes that held a ray, last completed launch */
    double launch_ms;              /* device time of that launch */
    double cost_spread;            /* (max - min) / mean of the XCDs' counted work under the large deal; < 0: not decided */
    uint64_t spec_started, spec_right, spec_wrong;   /* speculative samples (small shares) started / whose guessed RNG state was right / wrong, completed launches of this render */
    uint32_t form;                 /* the kernel's form this share is launched in: 0 plain (whole frames), 1 pixels that are behind keep their slots, 2 that and speculative samples */
    uint32_t reserved;
} ErStreamInfo;
int er_debug_stream_info(struct ErScene* s, ErStreamInfo* out);

/* The buffers er_gather_pass keeps on a scene (round 5: allocated by the first gather, reused by every later one): the receive
 * buffer for `peer`'s pixels on the root (*in_ptr, *in_bytes; NULL / 0 before the first gather or for peer == own rank) and the
 * packed send buffer of a non-root rank (*mine_ptr, *mine_bytes).  Device pointers, for identity comparison only. */
int er_debug_gather_buffers(struct ErScene* s, uint32_t peer, void** in_ptr, uint64_t* in_bytes, void** mine_ptr, uint64_t* mine_bytes);

/* `bytes` of a known pattern from this rank to ITSELF through the communicator's transport table -- group start, send(self),
 * recv(self), group end on a stream of the library's own -- and compared after the stream has drained: the one exchange RCCL
 * allows on a one-GPU box (it refuses two ranks on one device), so that ncclSend / ncclRecv of the dlopen'd library have carried
 * bytes from the C++ side before the first multi-GPU run.  *ms = wall time of the exchange.  ER_ERR_STATE if the bytes differ. */
int er_debug_comm_loopback(struct ErComm* c, uint64_t bytes, double* ms);

/* The streaming schedule's deal of a rank's owned 8 x 8 tiles (`owned`: tile indices ty * tiles_x + tx) to `blocks` workgroups, as
 * er_render_begin makes it (host code, no device needed): out[b + k * blocks] = the k-th tile of workgroup b or 0xFFFFFFFF, for
 * k < *most; workgroups b and b + 8 share an XCD.  edge = side of a super-tile in tiles, 0 = the library's default.  out_cap >= blocks * *most
 * (a first call with out_cap = 0 fails with ER_ERR_INVALID_ARG after setting *most). */
int er_debug_stream_deal(const uint32_t* owned, uint32_t count, uint32_t tiles_x, uint32_t blocks, int xcd_aware, uint32_t edge, uint32_t* out, uint32_t out_cap,
                         uint32_t* most);

/* A deal in the layout of er_debug_stream_deal (`deal`, deal_n = blocks * its most entries) levelled by counted cost, as the streaming schedule
 * does it after a render's first sample and again after its first call (host code, no device needed): cost[t] = counted work of tile t of
 * the frame (tiles >= cost_n count 0), cap = the most tiles one workgroup may get.  First the XCDs (workgroup b is on XCD b % 8 if blocks is
 * a multiple of 8): while the costliest exceeds the cheapest by more than twice the cost of the costliest one's LAST tile, that tile moves to
 * the cheapest; then, inside each XCD, heaviest tile first to the workgroup of the smallest summed cost that is under the cap.  Integer
 * arithmetic: the same costs give the same bytes; a total cost of 0 gives `deal` back.  out / out_cap / most as in er_debug_stream_deal. */
int er_debug_stream_level(const uint32_t* deal, uint32_t deal_n, uint32_t tiles_x, uint32_t blocks, const uint32_t* cost, uint32_t cost_n, uint32_t cap,
                          uint32_t* out, uint32_t out_cap, uint32_t* most);

/* How the deal in use spreads the work over the workgroups, and when they finished (streaming schedule; after er_wait / a read-back).
 * Every pointer may be NULL (nothing is copied there); a first call with info alone gives the sizes. */
typedef struct ErStreamBalance {
    uint32_t blocks;               /* workgroups */
    uint32_t most;                 /* the deal in use has blocks * most entries (layout of er_debug_stream_deal) */
    uint32_t levelled;             /* 1: the deal in use was levelled by counted cost; 0: it is dealt by tile count */
    uint32_t counting;             /* 1: the kernel is still counting tile costs (the render's first call has not completed) */
    uint32_t cost_tiles;           /* entries of the tile costs last read: tiles of the frame, 0 = none were counted */
    uint32_t cap;                  /* the most tiles one workgroup may get (pixel ring cells / 64) */
    uint64_t launch_ticks;         /* last completed launch: the latest XCD's end stamp minus the launch's start stamp, 100 MHz ticks (0: none) */
} ErStreamBalance;
/* wg_ticks[b]: workgroup b's end stamp minus the launch's start (0: it ran no wave), wg_tiles[b]: its tiles, wg_cost[b]: their summed cost
 * (tile costs last read), each `blocks` entries if wg_cap >= blocks; deal: the deal in use (deal_cap >= blocks * most); tile_cost: the
 * costs last read (cost_cap >= cost_tiles).  Measured times are for printing and logging: the library decides nothing on them. */
int er_debug_stream_balance(struct ErScene* s, ErStreamBalance* info, uint64_t* wg_ticks, uint32_t* wg_tiles, uint64_t* wg_cost, uint32_t wg_cap,
                            uint32_t* deal, uint32_t deal_cap, uint32_t* tile_cost, uint32_t cost_cap);

/* The streaming kernel's form for a share of `tiles` tiles on `blocks` workgroups, as er_render_begin and an adaptive re-deal choose
 * it (host code, no device needed; the A/B knobs of the environment are honoured): light_query = the slots carry a point-light or
 * emitter query; flags: the render's (ER_FLAG_COUNTERS matters). */
typedef struct ErStreamForm {
    uint32_t waves, tracers;       /* waves per workgroup (16 or 12) and how many of them trace at the start */
    uint32_t adapt;                /* 1: the split follows the tracer lanes' occupancy */
    uint32_t keep, spec;           /* 1: the share asks for the keep rule / for speculative samples */
    uint32_t reserved;
} ErStreamForm;
int er_debug_stream_form(uint32_t tiles, uint32_t blocks, int light_query, uint32_t tri_count, uint32_t flags, ErStreamForm* out);

/* The texture pool (er_render_begin fills it on the host, er_render_edit on the device: csrc/er_texplan.h, csrc/er_texstage.hip).  Both
 * hooks below only copy.  Entries: ErTexEntry = the device table's record of a texture (csrc/er_device.h DevTex; channels 1 and filter
 * 0 / 1 / 2 for a texture kept by its first channel, 2 = already to the power 2.2), ErFusedEntry = a material's fused record block
 * (DevFused; width 0 = not fused).  Buffers follow er_debug_read_accel's protocol: NULL = not wanted, capacities in bytes, a capacity
 * smaller than the array is ER_ERR_INVALID_ARG, all NULL queries the sizes. */
typedef struct ErTexEntry { int32_t width, height, channels, filter; uint32_t offset; } ErTexEntry;
typedef struct ErFusedEntry { int32_t width, height, filter; uint32_t offset; } ErFusedEntry;
typedef struct ErTexturePlan {
    uint32_t texture_count;        /* modes: texture_count bytes (0 as it came, 1 first channel alone, 2 that to the power 2.2); table: as many ErTexEntry */
    uint32_t fused_count;          /* fused: max(1, material_count) ErFusedEntry */
    uint32_t fused_any, reserved;
    ErTexEntry hdri;               /* the HDRI's texels lie last in the pool */
    uint64_t pool_floats;          /* >= 2^32: er_render_begin and er_render_edit refuse the scene */
} ErTexturePlan;
/* The texture plan of a scene description, as er_render_begin and er_render_edit make it (host code, no device needed; the
 * ER_TEX_COMPACT, ER_TEX_FUSE and ER_MAT_PRE_ON_DEVICE knobs of the environment are honoured).  Only the sizes, channels and filters of
 * desc->textures and desc->hdri.texture and the texture ids of desc->materials are read: no texel, no triangle array. */
struct ErSceneDesc;
int er_debug_texture_plan(const struct ErSceneDesc* desc, ErTexturePlan* plan, uint8_t* modes, uint64_t modes_cap, ErTexEntry* table, uint64_t table_cap,
                          ErFusedEntry* fused, uint64_t fused_cap);

/* What the texture, material and HDRI stages left in DEVICE memory (after er_render_begin; before: ER_ERR_STATE): the table, the pool
 * (pool_floats floats), the fused descriptors, mat_pre (material_count x 4 floats), the materials (material_count ErMaterial), the
 * HDRI's CDF (cdf_count floats) and its search guide (guide_count uint32), and the fields of the kernels' scene descriptor that
 * follow from them. */
typedef struct ErTextureDump {
    uint32_t texture_count, material_count, fused_count, cdf_count, guide_count;
    uint32_t tex_pow2, fused_any;  /* the descriptor's */
    int32_t hdri_buckets;
    float hdri_radiance_sum;
    ErTexEntry hdri_tex;           /* the descriptor's */
    uint64_t pool_floats;
} ErTextureDump;
int er_debug_read_textures(struct ErScene* scene, ErTextureDump* info, void* table, uint64_t table_cap, void* pool, uint64_t pool_cap, void* fused, uint64_t fused_cap,
                           void* mat_pre, uint64_t mat_pre_cap, void* materials, uint64_t materials_cap, void* cdf, uint64_t cdf_cap, void* guide, uint64_t guide_cap);

/* Test hook for the out-of-memory path of the boundary: while `bytes` is non-zero, any single large host allocation the
 * library announces (scene copy in er_scene_create, build staging in er_render_begin) larger than `bytes` fails as
 * std::bad_alloc would, which the entry point must turn into ER_ERR_OOM (no exception crosses the C ABI).  0 = off. */
void er_debug_set_host_alloc_limit(uint64_t bytes);

/* Test hook for er_render_begin's handling of a device BVH build that does not deliver: 0 = off; 1 = every device build fails as a
 * fault inside the builder would (default builder: one line on stderr and the host builder takes over; ER_FLAG_GPU_BUILD: ER_ERR_HIP);
 * 2 = as running out of device memory would (default builder: silent host fallback; ER_FLAG_GPU_BUILD: ER_ERR_OOM); 3 = every device
 * build delivers but reports a wide tree of ER_STACK8 + 1 levels (either way ER_ERR_STATE: the host builder makes the same tree). */
void er_debug_set_gpu_build_failure(int kind);

/* The host form of er_render_transform's arithmetic (csrc/er_xform.h) on caller arrays, no device needed: `count` triangles,
 * [count][3][3] rest vertices, normals and tangents -> pose(rest, m) in the three outputs (which must not overlap the inputs).
 * ER_ERR_INVALID_ARG: a NULL argument, a matrix entry that is not finite, det(L) not > 0.  The overflow bound is not applied here. */
int er_debug_transform_apply(const float m[12], uint32_t count, const float* vertices, const float* normals, const float* tangents,
                             float* out_vertices, float* out_normals, float* out_tangents);

/* The host form of er_render_skin's arithmetic (csrc/er_skin.h) on caller arrays, no device needed: a palette of bone_count row-major 3x4
 * matrices, `count` triangles with [count][3][ER_SKIN_INFLUENCES] bones and weights and [count][3][3] rest vertices, normals and tangents
 * -> the skinned ones in the three outputs (which must not overlap the inputs).  ER_ERR_INVALID_ARG: a NULL argument, or influences that
 * er_skin_set would refuse (bone_count, a bone index, a weight).  The palette's own checks (er_render_skin's) are not applied here. */
int er_debug_skin_apply(const float* palette, uint32_t bone_count, uint32_t count, const uint16_t* bones, const float* weights, const float* vertices,
                        const float* normals, const float* tangents, float* out_vertices, float* out_normals, float* out_tangents);

/* The ranking er_render_ids gives every pixel (csrc/er_ids.h er_id_rank, the function the kernel calls), on caller arrays, no device
 * needed: `count` <= 64 ids of the rays that hit (NULL with count 0) -> out_ids / out_counts [ER_ID_SLOTS] by (count descending, id
 * ascending as unsigned), unused slots (ER_ID_NONE, 0); *distinct = the number of distinct ids.  ER_ERR_INVALID_ARG: a NULL argument,
 * count > 64. */
int er_debug_id_rank(const uint32_t* ids, uint32_t count, uint32_t* out_ids, uint32_t* out_counts, uint32_t* distinct);

/* The arithmetic of the temporal reprojection (csrc/er_reproject.h, the functions the kernels call), on caller arrays, no device needed.
 * A projection camera is 12 floats: position[3], sensor_width, sensor_height, focal_length, then cos and sin of the rotation about x,
 * y and z as the library evaluates them (cx, sx, cy, sy, cz, sz).
 * er_debug_history_camera: the 12 floats of an ErCamera.
 * er_debug_history_project: `count` world points [count][3] -> out_xy [count][2] continuous pixel coordinates and out_ok [count]
 *   (0: not in front of the camera, or a coordinate not finite; the coordinates are then 0).
 * er_debug_history_back_matrix: B = M_capture o M_now^-1 of two row-major 3x4 poses; ER_ERR_INVALID_ARG if an entry is not finite or
 *   det(L_now) is not > 0.
 * er_debug_history_taps: one resolve of `count` pixels against a captured frame of x_res x y_res pixels.  Per pixel i: the new key --
 *   hit[i], object[i], P[i][3] (Hit.position, or the ray's direction of a miss) -- and moved[i] != 0 with back[i][12] if its object's
 *   pose changed.  The captured frame: old_hit, old_object, old_dist [y_res * x_res] and old_cw [y_res * x_res][4] = (C.rgb, W).
 *   Out: out_rgbw [count][4] = (H.rgb, w), out_state [count][4] = the four taps' states (0 valid, 1 outside the frame, 2 hit flag, 3
 *   object, 4 depth), out_class [count] (0 valid, 1 partial, 2 offscreen, 3 rejected, 4 sky).
 * er_debug_history_capture / _blend: `count` pixels of a capture (hist may be NULL: no resolved history) or of er_read_blended:
 *   beauty [count][4], samples [count], hist [count][4] -> out [count][4]. */
int er_debug_history_camera(const void* camera /* an ErCamera of eleven_hip.h */, float out[12]);
int er_debug_history_project(const float cam[12], uint32_t x_res, uint32_t y_res, uint32_t count, const float* points, float* out_xy, uint32_t* out_ok);
int er_debug_history_back_matrix(const float m_capture[12], const float m_now[12], float out[12]);
int er_debug_history_taps(const float cam[12], uint32_t x_res, uint32_t y_res, float depth_tolerance, uint32_t count, const uint32_t* hit, const uint32_t* object,
                          const float* P, const uint32_t* moved, const float* back, const uint32_t* old_hit, const uint32_t* old_object, const float* old_dist,
                          const float* old_cw, float* out_rgbw, uint32_t* out_state, uint32_t* out_class);
int er_debug_history_capture(uint32_t count, const float* beauty, const uint32_t* samples, const float* hist, float max_weight, float* out);
int er_debug_history_blend(uint32_t count, const float* beauty, const uint32_t* samples, const float* hist, float* out);

/* The arithmetic of the variance plane and of its filter (csrc/er_variance.h, the functions the kernels call), on caller arrays, no
 * device needed.  A pixel's state is 12 words: S.rgb, m (uint32), mu.rgb, W, M2.rgb, K (uint32).
 * er_debug_variance_mark / _fold: `count` pixels: beauty [count][4], samples [count], state [count][12] written / updated in place;
 *   folded [count] (may be NULL): 1 where the pixel had n > 0.
 * er_debug_variance_value: state [count][12], samples [count] -> out [count][4] = er_read_variance's pixel.
 * er_debug_variance_split: value [count][4], albedo [count][4] -> ve [count][4], the demodulated variance and the K >= 2 flag.
 * er_debug_variance_level_px: one level of er_denoise_variance over a whole frame of w x h pixels: planes e, ve, normal, albedo, depth
 *   [h * w][4] -> out_e, out_ve [h * w][4]; kc = 1 / colour_sigma^2, ka, kz as er_denoise_guided's.  step 1 .. 128. */
int er_debug_variance_mark(uint32_t count, const float* beauty, const uint32_t* samples, float* state);
int er_debug_variance_fold(uint32_t count, const float* beauty, const uint32_t* samples, float* state, uint32_t* folded);
int er_debug_variance_value(uint32_t count, const float* state, const uint32_t* samples, float* out);
int er_debug_variance_split(uint32_t count, const float* value, const float* albedo, float* ve);
int er_debug_variance_level_px(uint32_t w, uint32_t h, uint32_t step, float kc, float ka, float kz, const float* e, const float* ve, const float* normal, const float* albedo,
                               const float* depth, float* out_e, float* out_ve);

/* The arithmetic of the variance carried through the history (csrc/er_history_variance.h, the functions the kernels call), on caller
 * arrays, no device needed.  Planes are [count][4]: rgb and a flag word (0.0 or 1.0).
 * er_debug_history_variance_current: state [count][12] (er_debug_variance_*'s) -> out = (M2 / (K - 1) clamped at 0, K >= 2).
 * er_debug_history_variance_pool: (s_h, w [count]) and (s_c, n [count]) -> out = (pool.rgb, flag).
 * er_debug_history_variance_capture: state [count][12] (NULL: K = 0), samples [count], hist [count][4] = (H.rgb, w) (NULL: w = 0), hv
 *   (NULL: none) -> out = SV.
 * er_debug_history_variance_mean: tap states [count][4] (er_debug_history_taps's), tap weights [count][4], the taps' SV [count][4][4]
 *   -> out = HV.
 * er_debug_history_variance_taps: er_debug_history_taps with the captured SV plane old_sv [y_res * x_res][4] beside old_cw: out_rgbw is
 *   the colour's, out_hv = HV.
 * er_debug_history_variance_blend: as _capture -> out = VB.
 * er_debug_history_variance_split: blend (er_debug_history_blend's), vb, albedo [count][4] -> e, ve [count][4]. */
int er_debug_history_variance_current(uint32_t count, const float* state, float* out);
int er_debug_history_variance_pool(uint32_t count, const float* s_h, const float* w, const float* s_c, const float* n, float* out);
int er_debug_history_variance_capture(uint32_t count, const float* state, const uint32_t* samples, const float* hist, const float* hv, float* out);
int er_debug_history_variance_mean(uint32_t count, const uint32_t* tap_state, const float* tap_w, const float* tap_sv, float* out);
int er_debug_history_variance_taps(const float cam[12], uint32_t x_res, uint32_t y_res, float depth_tolerance, uint32_t count, const uint32_t* hit, const uint32_t* object,
                                   const float* P, const uint32_t* moved, const float* back, const uint32_t* old_hit, const uint32_t* old_object, const float* old_dist,
                                   const float* old_cw, const float* old_sv, float* out_rgbw, float* out_hv, uint32_t* out_state, uint32_t* out_class);
int er_debug_history_variance_blend(uint32_t count, const float* state, const uint32_t* samples, const float* hist, const float* hv, float* out);
int er_debug_history_variance_split(uint32_t count, const float* blend, const float* vb, const float* albedo, float* e, float* ve);

/* The cut-out rule of the first-hit pass (csrc/er_cutout.h, the functions the kernels call), on caller arrays, no device needed.
 * er_debug_cutout_threshold: t [count] -> ok [count] (1: er_first_hit_set takes it) and resolved [count] (0 -> 0.5).
 * er_debug_cutout_stops: opacity [count], threshold [count] -> out [count] (1: the hit stops the ray).
 * er_debug_cutout_continue: position, d [count][3] -> the continuation ray's origin and direction [count][3]. */
int er_debug_cutout_threshold(uint32_t count, const float* t, uint32_t* ok, float* resolved);
int er_debug_cutout_stops(uint32_t count, const float* opacity, const float* threshold, uint32_t* out);
int er_debug_cutout_continue(uint32_t count, const float* position, const float* d, float* o_out, float* d_out);
/* FirstHit::visible (csrc/er_first_hit.h) for n arbitrary rays of a begun scene, whatever its er_first_hit_set: `threshold` as
 * er_first_hit_set takes it, at most max_bounces hits examined.  tri_out: the triangle id of the hit that stopped the ray, or -1;
 * layers_out: the hits passed (of a capped ray: max_bounces); dist_out: length(position - origin), 0 of a miss; pos_out [n][3]: the
 * hit's position, zeros of a miss.  The directions are taken as given (normalise them as the camera does). */
int er_debug_first_hit_rays(struct ErScene* scene, const float* origins, const float* dirs, uint32_t n, float threshold, int32_t* tri_out, uint32_t* layers_out,
                            float* dist_out, float* pos_out);

#ifdef __cplusplus
}
#endif
#endif
