// er_history.h -- what a scene keeps for the temporal reprojection (include/eleven_hip.h er_history_*; er_reproject.h has the arithmetic,
// er_history.hip the kernels and entry points).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/eleven_hip.h"
#include "er_devbuf.h"
#include "er_history_variance.h"
#include "er_reproject.h"

// Two key planes of 6 words per pixel, plane after plane (hit, object, dist, then P as [npx][3]): key[now] is made by a resolve (or by a
// capture that finds none current), key[1 - now] is the captured one -- a capture swaps the two instead of copying.  d_cw: the captured
// (C.rgb, W); d_hist: the resolved (H.rgb, w).  80 bytes per pixel, allocated by the first capture.  A key plane is CURRENT while the
// camera and every pose are, bit for bit, what it was made with: everything else that changes what a pinhole ray hits drops the whole
// history (invalidate).
// d_sv: the captured per-sample variance and its flag, d_hv: the resolved one (er_history_variance.h) -- 32 more bytes per
// pixel, allocated by the first capture of a scene whose variance state exists.  sv_captured / hv_resolved say whether the held capture /
// the resolved history carries them; they fall with the capture.
struct ErHistoryState {
    erh::DevBuf<uint32_t> d_key[2];
    erh::DevBuf<float4> d_cw, d_hist;
    erh::DevBuf<float> d_back;                 // per object 12 floats of B_o and a `moved` word: 13 words, one small table per resolve
    erh::DevBuf<unsigned long long> d_counts;  // the five class counts of a resolve
    int now = 0;
    bool captured = false, resolved = false, key_valid = false;
    ErCamera cap_cam{}, key_cam{};
    std::vector<float> cap_m, key_m;           // [objects][12]
    float tol = 0.02f, max_weight = 32.0f;
    uint32_t moved_objects = 0;
    uint64_t classes[ER_HC_COUNT] = {0, 0, 0, 0, 0};
    float capture_ms = 0, resolve_ms = 0;
    erh::DevBuf<float4> d_sv, d_hv;
    erh::DevBuf<uint32_t> d_known;             // three counts of pixels whose flag is set, ER_HV_COUNT_STRIDE words apart: SV, HV, VB
    bool sv_captured = false, hv_resolved = false;
    uint64_t known_captured = 0, known_history = 0, known_blended = 0;
    float blended_filter_ms = 0;
    void invalidate() noexcept {
        captured = resolved = key_valid = false;
        sv_captured = hv_resolved = false;
        known_captured = known_history = known_blended = 0;
    }
    void release() {
        d_key[0].release(); d_key[1].release(); d_cw.release(); d_hist.release(); d_back.release(); d_counts.release();
        d_sv.release(); d_hv.release(); d_known.release();
        invalidate();
    }
};

#define ER_HV_COUNT_STRIDE 16      // (64 bytes between two counters)
enum { ER_HV_KNOWN_CAPTURED = 0, ER_HV_KNOWN_HISTORY = 1, ER_HV_KNOWN_BLENDED = 2, ER_HV_KNOWN_COUNT = 3 };

// er_history_variance.hip: the kernels that carry the variance beside the colour, launched by er_history_capture / er_history_resolve.
// `blocks`: a bounded grid (four workgroups per CU), the kernels walk the frame with a grid stride; known: one counter of d_known, zeroed.
hipError_t er_probe_history_variance(const char** which);      // er_render_begin asks it beside er_probe_history
// m2k: the third plane of the variance state or NULL (a restart is pending: K = 0); hist / hv: the resolved planes or NULL
void er_launch_history_variance_capture(const float4* m2k, const uint32_t* samples, const float4* hist, const float4* hv, size_t npx, float4* sv, uint32_t* known,
                                        unsigned blocks, hipStream_t stream);
// k_history_resolve's arguments and the captured SV: the taps are taken once, hist and hv written, the five classes and the known pixels counted
void er_launch_history_resolve_variance(const uint32_t* key_now, const uint32_t* key_old, const float4* cw, const float4* sv, const float* back, uint32_t objects,
                                        const ErReprojCam& cam, uint32_t x_res, uint32_t y_res, float tol, float4* hist, float4* hv, unsigned long long* counts,
                                        uint32_t* known, unsigned blocks, hipStream_t stream);

hipError_t er_probe_history(const char** which);      // see er_kernels.h; er_render_begin asks it beside er_probe_ids
