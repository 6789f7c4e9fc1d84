// er_history.h -- what a scene keeps for the temporal reprojection (include/eleven_hip.h er_history_*; er_reproject.h has the arithmetic,
// er_history.hip the kernels and entry points).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/eleven_hip.h"
#include "er_devbuf.h"
#include "er_reproject.h"

// Two key planes of 6 words per pixel, plane after plane (hit, object, dist, then P as [npx][3]): key[now] is made by a resolve (or by a
// capture that finds none current), key[1 - now] is the captured one -- a capture swaps the two instead of copying.  d_cw: the captured
// (C.rgb, W); d_hist: the resolved (H.rgb, w).  80 bytes per pixel, allocated by the first capture.  A key plane is CURRENT while the
// camera and every pose are, bit for bit, what it was made with: everything else that changes what a pinhole ray hits drops the whole
// history (invalidate).
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
    void invalidate() noexcept { captured = resolved = key_valid = false; }
    void release() {
        d_key[0].release(); d_key[1].release(); d_cw.release(); d_hist.release(); d_back.release(); d_counts.release();
        invalidate();
    }
};

hipError_t er_probe_history(const char** which);      // see er_kernels.h; er_render_begin asks it beside er_probe_ids
