// er_history_variance.h -- the per-sample variance carried through the reprojection history, the variance of the blended colour and the
// planes the a-trous filter takes of the blend (include/eleven_hip.h er_history_variance_info, er_read_history_variance,
// er_read_blended_variance, er_denoise_blended; er_history_variance.hip has the kernels and entry points).  Every float32
// operation is stated ONCE here, for the device kernels, for the tests (er_debug_history_variance_*; elevenrender_amd/
// history_variance.py restates it in numpy) and for tests/native/history_variance_host.cpp, which compiles this file alone under
// ASan + UBSan.  Plain C++ plus __host__ __device__, without a HIP or library header.  Nothing is contracted (-ffp-contract=off): every
// product, quotient and sum is rounded by itself in the written order.
//
// West's moments (er_variance.h) give the variance of ONE sample of a pixel, s2 = M2 / (K - 1): a property of the surface point, which
// reprojects as the colour does.  A history weight w is an effective sample count, so the history colour has the variance s2_H / w.
//   current (M2.rgb, K):  K < 2: (0, 0, 0), flag 0.  Otherwise per channel s2 = M2 / (float)(K - 1), values that are not > 0 (a NaN too)
//                         become 0; flag 1.  A pending restart or an unallocated state is K = 0.
//   pool ((s2_H, k_H, w), (s2_C, k_C, n)):  useH = k_H && w > 0;  useC = k_C && n > 0.
//                         both: sum = w + n, per channel (w * s2_H + n * s2_C) / sum;  one: that one, bit for bit;  none: (0, 0, 0).
//                         flag = useH || useC.
//   capture:              SV = (pool(HV.rgb, HV.w != 0, w, current, n), flag) with (HV, w) the pixel's resolved history variance and
//                         weight (none resolved, or a capture that carried nothing: k_H = 0, w = 0), n = (float)(samples - 1) (0 for
//                         samples = 0): er_history_render_mean's n, the weights of er_history_capture_px.
//   resolve:              the colour's four taps, states and weights (er_history_tap_set).  A tap counts if it is ER_TAP_VALID and its
//                         SV.w != 0.  In er_history_mean's loop order: ws = ws + (counts ? tap_w : 0); acc_c = acc_c + (counts ?
//                         tap_w * SV_c : 0);  ws > 0: HV = (acc / ws, 1), else (0, 0, 0, 0).  A plain weighted mean: the carried value is
//                         the variance of a sample of the surface point, not of the interpolated colour.
//   blend variance:       (s2, k) = pool(HV, w, current, n);  sum = w + n;  VB_c = (k && sum > 0) ? s2_c / sum : 0;  VB.w = k.
//   split:                a_c = albedo_c + 0.01;  e = (blend_c / a_c, blend.w) with the blend of er_history_blend_px;
//                         ve = (VB_c / (a_c * a_c), VB.w)        (er_variance_split_px's shape; ve.w is the filter's "known" flag)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "er_reproject.h"      // the taps, er_history_render_mean, er_history_blend_px

#define ER_HV_HD ER_RP_HD

ER_HV_HD inline uint32_t er_hv_word(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

// m2k: the third float4 of a pixel's variance state (M2.rgb, K as a uint32 word), or NULL (K = 0) -> s2[3]; returns the flag
ER_HV_HD inline uint32_t er_hv_current_px(const float* m2k, float* s2) {
    const uint32_t K = m2k ? er_hv_word(m2k[3]) : 0u;
    if (K < 2u) { s2[0] = s2[1] = s2[2] = 0.0f; return 0u; }
    const float fk = (float)(K - 1u);
    for (int c = 0; c < 3; c++) {
        const float v = m2k[c] / fk;
        s2[c] = v > 0.0f ? v : 0.0f;      // (a NaN becomes 0 too)
    }
    return 1u;
}

ER_HV_HD inline float er_hv_samples_n(uint32_t samples) { return (float)(samples > 0u ? samples - 1u : 0u); }      // er_history_render_mean's nf

ER_HV_HD inline uint32_t er_hv_pool_px(const float* sH, uint32_t kH, float w, const float* sC, uint32_t kC, float n, float* out /*[3]*/) {
    const bool useH = kH != 0u && w > 0.0f, useC = kC != 0u && n > 0.0f;
    if (useH && useC) {
        const float sum = w + n;
        for (int c = 0; c < 3; c++) out[c] = (w * sH[c] + n * sC[c]) / sum;
    } else if (useH) {
        for (int c = 0; c < 3; c++) out[c] = sH[c];
    } else if (useC) {
        for (int c = 0; c < 3; c++) out[c] = sC[c];
    } else {
        for (int c = 0; c < 3; c++) out[c] = 0.0f;
    }
    return (useH || useC) ? 1u : 0u;
}

// One pixel of a capture: hist_w = the resolved history's weight (0: none), hv = (s2_H.rgb, flag) or NULL -> sv = (s2.rgb, flag)
ER_HV_HD inline uint32_t er_hv_capture_px(const float* m2k, uint32_t samples, float hist_w, const float* hv, float* sv) {
    float cur[3];
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const uint32_t kC = er_hv_current_px(m2k, cur);
    const uint32_t kH = hv ? (hv[3] != 0.0f ? 1u : 0u) : 0u;
    const uint32_t k = er_hv_pool_px(hv ? hv : zero, kH, hist_w, cur, kC, er_hv_samples_n(samples), sv);
    sv[3] = k ? 1.0f : 0.0f;
    return k;
}

// The mean of the carried variance over the taps that are valid and known: sv[k] = the captured SV at tap k (read only where state[k] is
// ER_TAP_VALID) -> out = (s2_H.rgb, flag)
ER_HV_HD inline uint32_t er_hv_mean(const int* state, const float* tap_w, const float (*sv)[4], float* out) {
    float ws = 0.0f, acc[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 4; k++) {
        const bool v = state[k] == ER_TAP_VALID && sv[k][3] != 0.0f;
        ws = ws + (v ? tap_w[k] : 0.0f);
        for (int c = 0; c < 3; c++) acc[c] = acc[c] + (v ? tap_w[k] * sv[k][c] : 0.0f);
    }
    const bool any = ws > 0.0f;
    for (int c = 0; c < 3; c++) out[c] = any ? acc[c] / ws : 0.0f;
    out[3] = any ? 1.0f : 0.0f;
    return any ? 1u : 0u;
}

// One pixel of a resolve that carries the variance: er_history_resolve_px's taps taken once -> hist = (H.rgb, w), hv = (s2_H.rgb, flag);
// returns the pixel's class.  old_sv: the captured SV plane [npx][4].
ER_HV_HD inline int er_hv_resolve_px(const ErHistoryKey& k, const float* back, uint32_t moved, const ErReprojCam& cam, uint32_t x_res, uint32_t y_res, float tol,
                                     const uint32_t* old_hit, const uint32_t* old_object, const float* old_dist, const float* old_cw, const float* old_sv, float* hist,
                                     float* hv, int* state_out /*[4] or NULL*/) {
    int state[4];
    float tw[4], cw[4][4], sv[4][4];
    size_t q[4];
    er_history_tap_set(k, back, moved, cam, x_res, y_res, tol, old_hit, old_object, old_dist, state, tw, q);
    for (int t = 0; t < 4; t++) {
        const bool v = state[t] == ER_TAP_VALID;
        for (int c = 0; c < 4; c++) { cw[t][c] = v ? old_cw[q[t] * 4 + c] : 0.0f; sv[t][c] = v ? old_sv[q[t] * 4 + c] : 0.0f; }
        if (state_out) state_out[t] = state[t];
    }
    er_history_mean(state, tw, cw, hist);
    er_hv_mean(state, tw, sv, hv);
    return er_history_class(k.hit, state);
}

// One pixel of er_read_blended_variance: hist_w = the resolved history's weight, hv = (s2_H.rgb, flag) or NULL -> vb = (VB.rgb, flag)
ER_HV_HD inline uint32_t er_hv_blend_px(const float* m2k, uint32_t samples, float hist_w, const float* hv, float* vb) {
    float cur[3], s2[3];
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const uint32_t kC = er_hv_current_px(m2k, cur);
    const uint32_t kH = hv ? (hv[3] != 0.0f ? 1u : 0u) : 0u;
    const float w = hist_w, n = er_hv_samples_n(samples);
    const uint32_t k = er_hv_pool_px(hv ? hv : zero, kH, w, cur, kC, n, s2);
    const float sum = w + n;
    const bool any = k != 0u && sum > 0.0f;
    for (int c = 0; c < 3; c++) vb[c] = any ? s2[c] / sum : 0.0f;
    vb[3] = k ? 1.0f : 0.0f;
    return k;
}

// The filter's two planes of one pixel: blend = er_history_blend_px's (rgb, 1), vb = er_hv_blend_px's
ER_HV_HD inline void er_hv_split_px(const float* blend, const float* vb, const float* albedo, float* e, float* ve) {
    for (int c = 0; c < 3; c++) {
        const float a = albedo[c] + 0.01f;
        e[c] = blend[c] / a;
        ve[c] = vb[c] / (a * a);
    }
    e[3] = blend[3];
    ve[3] = vb[3];
}
