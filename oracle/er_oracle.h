/* er_oracle.h -- C entry points of the CPU oracle (liberoracle.so).
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the product (elevenrender_amd/, include/) may
 * include, link or call this.  Only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg load it -- as the checker / CPU baseline, never as the thing shipped.
 *
 * The reference (101001000/ElevenRender) has no tests, golden vectors or fixtures for this
 * path.  This oracle is a line-by-line restatement of the reference algorithm from reading
 * its source.  On the default path (flags 0) it is PINNED to the reference's own code: the
 * reference's per-sample sources, compiled on the host (`make ref`, ref_driver.cpp, stand-in
 * third-party headers in ref_shim/), recorded tests/golden/reference_*.npz, and
 * tests/test_reference_kat_cpu.py requires every function-level entry point below and whole
 * renders of two scenes to equal them bit for bit in both math modes.  PARITY UNPINNED
 * remains: the build-defined extensions (flags), SYCL device math versus libm, scene and
 * texture loading; see DESIGN.md "Oracle".
 */
#ifndef ER_ORACLE_H
#define ER_ORACLE_H
#include "../include/eleven_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OracleOpts {
    int32_t math_mode;    /* 0 = glibc libm (what a CPU build of the reference gets), 1 = er_math.h */
    int32_t max_bounces;  /* 0 -> 5 (src/kernel.cpp:508) */
    int32_t traversal;    /* 0 = reference BVH (fixed depth 18, src/BVH.cpp), 1 = brute force over all tris */
    int32_t threads;      /* worker threads over pixel rows; <=0 -> 1 */
    uint32_t flags;       /* ER_FLAG_POINT_LIGHTS | ER_FLAG_MIS | ER_FLAG_MESH_LIGHTS: the three build-defined extensions, mirrored
                             operation for operation from elevenrender_amd/csrc/er_shade.h (the reference defines no result for any).
                             ER_FLAG_MESH_LIGHTS takes effect after oracle_set_emitters has made a non-empty table */
} OracleOpts;

typedef struct OracleCounters {
    uint64_t paths, bounce_samples, rays;
    uint64_t node_visits;   /* inner-node iterations of BVH::transverse (two box tests each) */
    uint64_t tri_tests, tri_hits, shaded_hits, texel_fetches, hdri_samples;
} OracleCounters;

/* one record per executed bounce-loop iteration */
typedef struct OracleTraceRec {
    int32_t bounce;
    int32_t tri;            /* ORIGINAL triangle id of the closest hit, -1 = miss */
    int32_t shadow_tri;     /* original id of the shadow ray's closest hit, -1 = none / not traced */
    int32_t opaque;         /* 1 if the opacity test passed */
    float position[3];
    float wi[3];            /* next ray direction */
    float light[3];
    float reduction[3];
    int32_t shadow_occ;     /* HDRI shadow query: 1 if shadowHit.valid && shadowHit.triIdx != hitdata.triIdx, 0 if not, -1 not traced */
    int32_t light_occ;      /* point-light / emitter query (extensions): 1 occluded, 0 visible, -1 none */
    /* ER_FLAG_MESH_LIGHTS, the oracle's own (the library's ErTraceRec ends above): what the bounce did, for counting what a scene exercises */
    int32_t mesh_sample;    /* -1 no opaque bounce with a table; 0 emitter sample evaluated and its shadow query traced; 1 skipped: k is the
                               shaded triangle; 2 skipped: the last bounce; 3 skipped: cos_l == 0; 4 skipped: DisneyEval exactly zero */
    int32_t mesh_k;         /* the picked emitter's input triangle, -1 none */
    int32_t mesh_le_tex;    /* mesh_sample 0: the texture Le came from, -1 a constant */
    float mesh_opacity;     /* mesh_sample 0: the opacity at the sampled point BEFORE the clamp */
    int32_t mesh_hit;       /* a table triangle reached with prev_pdf >= 0 (rule 7): 1 reached directly, its emission weighted by w_bsdf;
                               2 reached after at least one opacity pass-through, weight 1 */
    float mesh_d;           /* mesh_hit 1: mesh_d at the hit (0.001f: the ray left that far from the bounce) */
} OracleTraceRec;

typedef struct Oracle Oracle;

Oracle* oracle_create(const ErSceneDesc* desc, const OracleOpts* opts);
void oracle_destroy(Oracle* o);

/* ER_FLAG_MESH_LIGHTS: hands the oracle the emitter ORDER -- input triangle ids in the library's table order (ascending triangle slot of
 * ITS acceleration structure; the oracle's tree has another leaf order, and the order decides which emitter a draw picks).  From it the
 * oracle builds weights, CDF and P itself, in the float order the header of elevenrender_amd/csrc/er_lights.hip documents.  Returns 0, or
 * -1 (and an empty table) if the list is not exactly the oracle's own set of emitters, each once.  n = 0: an empty table. */
int oracle_set_emitters(Oracle* o, const int32_t* tri_ids, uint32_t n);
/* the table as built: per entry the input triangle, weight, CDF entry and P; *total = W.  Any output may be NULL; returns the entry count. */
uint32_t oracle_read_emitters(const Oracle* o, int32_t* tri_ids, float* weight, float* cdf, float* prob, float* total, uint32_t cap);
/* the mean luminance of a texture in the texture-mean kernel's summation order */
float oracle_texture_mean_luminance(const ErTexture* tex);
/* mesh_pick on the oracle's table (0xFFFFFFFF for an empty one) */
uint32_t oracle_mesh_pick(const Oracle* o, float r);
double oracle_build_seconds(const Oracle* o);

/* n_samples calls of renderingKernel for every pixel idx in [idx0, idx1) (idx1 = 0 -> all). */
void oracle_render(Oracle* o, uint32_t n_samples, uint32_t idx0, uint32_t idx1);
void oracle_read_pass(const Oracle* o, int pass, float* dst_rgba);
void oracle_read_samples(const Oracle* o, uint32_t* dst);
void oracle_read_rng(const Oracle* o, uint32_t* dst);
void oracle_counters(const Oracle* o, OracleCounters* out);

/* Runs ONE more sample of pixel idx and records up to max_recs bounce records; returns count. */
int oracle_trace_pixel(Oracle* o, uint32_t idx, OracleTraceRec* recs, int max_recs);

/* closest hit of the reference traversal for arbitrary rays: out_tri = original tri id or -1,
 * out_pos[3] = Hit.position */
void oracle_closest_hit(Oracle* o, const float* origins, const float* dirs, int n,
                        int32_t* out_tri, float* out_pos);

/* ---- function-level entry points (for known-answer tests) ---- */
uint32_t oracle_jenkins_oaat_u32(uint32_t seed);
uint32_t oracle_jenkins_oaat_bytes(const uint8_t* key, size_t len);   /* the published general form */
void oracle_rng_stream(uint32_t pixel_idx, int n, uint32_t* states, float* values);
void oracle_xorshift32(uint32_t* state);
void oracle_camera_ray(const ErCamera* cam, uint32_t x_res, uint32_t y_res, int x, int y,
                       const float r[5], int math_mode, float out_origin[3], float out_dir[3]);
/* tri = 9 verts, 9 normals, 9 tangents, 6 uvs, sign; returns hit flag and fills
 * out[0..2]=position, [3..5]=normal, [6..8]=gnormal, [9..11]=tangent, [12..14]=bitangent, [15]=tu, [16]=tv */
int oracle_tri_hit(const float* verts, const float* normals, const float* tangents, const float* uvs,
                   float tangent_sign, const float origin[3], const float dir[3], float out[17]);
int oracle_box_hit(const float origin[3], const float dir[3], const float b1[3], const float b2[3]);
/* hd[]: metallic, roughness, clearcoatGloss, clearcoat, anisotropic, transmission, specular,
 * specularTint, sheenTint, subsurface, sheen, albedo[3], tangent[3], bitangent[3]  (20 floats) */
void oracle_disney_eval(const float hd[20], const float V[3], const float N[3], const float L[3],
                        int math_mode, float out[3]);
float oracle_disney_pdf(const float hd[20], const float V[3], const float N[3], const float L[3], int math_mode);
void oracle_disney_sample(const float hd[20], const float V[3], const float N[3], float r1, float r2, float r3,
                          int math_mode, float out[3]);
void oracle_spherical_mapping(const float p[3], int math_mode, float* u, float* v);
void oracle_reverse_spherical_mapping(float u, float v, int math_mode, float out[3]);
void oracle_texture_fetch(const ErTexture* tex, float u, float v, int filtered, float out[3]);
void oracle_hdri_cdf(const ErTexture* tex, float* cdf, float* radiance_sum);
int oracle_hdri_binary_search(const float* cdf, float value, int length);
float oracle_hdri_pdf(const ErTexture* tex, float radiance_sum, int x, int y, int math_mode);
/* math: kind 0 sin,1 cos,2 acos,3 log,4 pow(x,y),5 atan2(x=y_arg,y=x_arg) ; mode as above */
void oracle_math(int kind, int math_mode, const float* x, const float* y, float* out, int n);

#ifdef __cplusplus
}
#endif
#endif
