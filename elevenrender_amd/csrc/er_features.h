// er_features.h -- launch wrappers of the feature pass and of the guided filter (er_features.hip; include/eleven_hip.h
// er_render_features, er_read_feature, er_gather_feature, er_denoise_guided).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

struct DevScene;

hipError_t er_probe_features(const char** which);
// n camera rays per owned pixel of S through the production traversal: albedo and depth (row-major float4 planes of the frame) of the
// owned pixels are overwritten.  `blocks`, `spill`: the first-hit pass's grid and spill area (er_first_hit_blocks, er_first_hit.h).
void er_launch_features(const DevScene& S, uint32_t n, float4* albedo, float4* depth, uint32_t blocks, uint2* spill, hipStream_t stream);
// ... with the pass seeing through cut-outs (er_first_hit_set): the resolved threshold and the mode's counter words (er_first_hit.h)
void er_launch_features_cutouts(const DevScene& S, uint32_t n, float4* albedo, float4* depth, uint32_t blocks, uint2* spill, float threshold, unsigned long long* counts,
                                hipStream_t stream);
hipError_t er_probe_first_hit(const char** which);      // er_first_hit.hip; er_render_begin asks it beside er_probe_ids
// pixels of the listed tiles <-> compact buffer [tile][64] float4 of a row-major plane (lanes outside the frame: zero / skipped)
void er_launch_pack_plane(const DevScene& S, const uint32_t* tiles, uint32_t ntiles, const float4* plane, void* dst, hipStream_t stream);
void er_launch_unpack_plane(const DevScene& S, const uint32_t* tiles, uint32_t ntiles, float4* plane, const void* src, hipStream_t stream);
// the guided filter's three steps (er_features.hip gives the arithmetic): e0 = beauty / (albedo + 0.01); one a-trous level; out = e * (albedo + 0.01)
void er_launch_guided_split(const float4* beauty, int beauty_stride, const float4* albedo, float4* e, int w, int h, hipStream_t stream);
void er_launch_guided_level(const float4* src, const float4* normal, int normal_stride, const float4* albedo, const float4* depth, float4* dst, int w, int h,
                            int step, float kc, float ka, float kz, hipStream_t stream);
void er_launch_guided_join(const float4* e, const float4* albedo, const float4* beauty, int beauty_stride, float4* out, int w, int h, hipStream_t stream);
