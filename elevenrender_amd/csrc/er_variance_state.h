// er_variance_state.h -- what a scene keeps for the variance plane (include/eleven_hip.h er_variance_*; er_variance.h has the arithmetic,
// er_variance.hip the kernels and entry points).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/eleven_hip.h"
#include "er_devbuf.h"

// d_state: three float4 planes of the frame back to back -- (S, m), (mu, W), (M2, K) -- 48 bytes per pixel, allocated by the first fold
// (or by an er_state_import, which has to snapshot the planes it brought).  A restart of the render (er_render_begin, every edit) only
// sets `restarted`: the planes are then (0, 0, 0) with count 1 in every pixel, which is what the next use writes into the snapshot before
// anything else -- and what a batch measured from the start of the render needs whether or not that restart went through.
struct ErVarianceState {
    erh::DevBuf<float4> d_state;
    erh::DevBuf<uint32_t> d_counts;      // pixels folded and, 64 bytes on, pixels with K >= 2: written by a fold
    bool restarted = true;
    uint32_t folds = 0;
    uint64_t pixels_folded = 0, pixels_known = 0;
    float fold_ms = 0, filter_ms = 0;
    void reset() noexcept { restarted = true; folds = 0; pixels_folded = pixels_known = 0; fold_ms = filter_ms = 0; }
    void release() {
        d_state.release(); d_counts.release();
        reset();
    }
};

struct ErScene;
// er_denoise_variance's argument checks and defaults, for every filter of this family: levels, kc = 1 / colour_sigma^2, ka, kz
int er_variance_filter_params(const ErDenoiseVariance* p, const char* who, uint32_t* levels, float* kc, float* ka, float* kz);
// the a-trous levels on demodulated planes: bufs[0] / vbufs[0] hold (e, ve) of er_variance.h; the result is in bufs[levels & 1]
void er_launch_variance_levels(float4* const bufs[2], float4* const vbufs[2], const float4* normal, int normal_stride, const float4* albedo, const float4* depth, int w, int h,
                               uint32_t levels, float kc, float ka, float kz, hipStream_t stream);
hipError_t er_probe_variance(const char** which);      // see er_kernels.h; er_render_begin asks it beside er_probe_history
// er_state_import's reset: the snapshot is taken from the planes as they lie now (the stream is idle, the scene's mutex held)
int er_variance_mark_imported(ErScene* s);
