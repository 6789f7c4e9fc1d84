// er_lights.h -- the emitter table of ER_FLAG_MESH_LIGHTS (rules: er_shade.h), built on the device by er_lights.hip during
// er_render_begin.  The shading step reads it through er_shade.h (mesh_pick, mesh_prob, mesh_tri).
//
// ONE device buffer of floats, in three parts (tri_count = T slots, n emitters):
//   [0, T)          P per triangle slot: w_slot / W for an emitter, 0 for every other slot (the BRDF-hit weight, er_bounce.inc)
//   [T, T + n)      the normalised CDF over the emitters, in ascending slot order
//   [T + n, T + 2n) the emitters' slots (uint32 bits), in the same order
// DevScene::mesh_lights points at it and DevScene::emitter_count holds n (er_device.h: they share their words with the point lights,
// which a render with a non-empty table never samples).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

struct ErMaterial;
struct DevTex;

// Builds the table of the triangles in `isect` (3 float4 per slot) / `attr` (ER_ATTR_PIECES float4 per slot); `emission_textures`
// (device, `n_etex` entries) lists the texture ids some material uses as emission_tex.  Enqueues everything on `stream`; waits for it
// twice (the emitter count sizes the table; W is reported).  On success *table holds the buffer described above (hipMalloc'd, the caller
// frees it; NULL when there is no emitter), *count the emitter count and *total the sum of the weights W.  Returns a hipError_t.
hipError_t er_lights_build(const float4* isect, const float4* attr, uint32_t tri_count, const ErMaterial* materials, const DevTex* textures,
                           const float* tex_pool, const int32_t* emission_textures, uint32_t n_etex, uint32_t texture_count,
                           float** table, uint32_t* count, float* total, hipStream_t stream);
// out[i] <- the input triangle index of the i-th emitter (the builder's permutation is in the triangle records), cdf_out[i] <- its CDF
// entry, prob_out[i] (may be NULL) <- P at its slot, for i < min(count, cap)
void er_launch_light_table_read(const float4* isect, const float* table, uint32_t tri_count, uint32_t count, uint32_t cap,
                                int32_t* out, float* cdf_out, float* prob_out, hipStream_t stream);
