// er_reproject.h -- temporal reprojection (include/eleven_hip.h er_history_capture, er_history_resolve, er_history_info, er_read_history,
// er_read_blended; er_history.hip has the kernels and entry points).  Every float32 operation of the projection, the tap
// test, the bilinear mean, the capture and the blend is stated ONCE here, for the device kernels, for the tests
// (er_debug_history_project / _back_matrix / _taps; elevenrender_amd/history.py restates it in numpy) and for
// tests/native/history_host.cpp, which compiles this file alone under ASan + UBSan.  Plain C++ plus __host__ __device__, without a HIP
// or library header.  Nothing is contracted (-ffp-contract=off): every product and every sum is rounded by itself in the written order.
#pragma once
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "er_xform.h"      // er_xform_point: how a back matrix is applied

#if defined(__HIPCC__)
#define ER_RP_HD __host__ __device__
#else
#define ER_RP_HD
#endif

#define ER_HISTORY_NONE 0xFFFFFFFFu      // (= ER_ID_NONE: a triangle in no object, or no table)

// A camera as the projection needs it, 12 floats: position, sensor width and height, focal length, and the six sines and cosines of
// camera_trig (er_device.h) -- the values camera_ray rotates by, so that the projection undoes the same rotation.
struct ErReprojCam {
    float pos[3];
    float sensor_w, sensor_h, focal;
    float cx, sx, cy, sy, cz, sz;
};
static_assert(sizeof(ErReprojCam) == 48, "a projection camera is 12 floats");

// One pixel of a key plane: P = Hit.position of a hit, the ray's direction of a miss; dist = length(Hit.position - ray.o), 0 of a miss.
struct ErHistoryKey {
    uint32_t hit, object;
    float dist;
    float P[3];
};

// tap states (er_history_taps): why a tap does not count, in the order the tests are made
enum { ER_TAP_VALID = 0, ER_TAP_OUTSIDE = 1, ER_TAP_FLAG = 2, ER_TAP_OBJECT = 3, ER_TAP_DEPTH = 4 };
// pixel classes (ErHistoryInfo): exclusive, every pixel of the frame is in exactly one
enum { ER_HC_VALID = 0, ER_HC_PARTIAL = 1, ER_HC_OFFSCREEN = 2, ER_HC_REJECTED = 3, ER_HC_SKY = 4, ER_HC_COUNT = 5 };

ER_RP_HD inline float er_rp_length(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }
ER_RP_HD inline bool er_rp_finite(float v) { return v - v == 0.0f; }      // (false for NaN and both infinities)

// World point p -> continuous pixel coordinates of camera c on an x_res x y_res frame: pixel x's pinhole ray (r1 = r2 = 0.5) goes through
// coordinate x exactly.  v = p - position; camera_ray's three rotations undone in reverse order (Z, Y, X: each the transpose, with the
// same six values); then the sensor plane at z = focal_length:
//   s = focal / d.z,   fx = ((d.x * s) / sensor_w + 0.5) * x_res,   fy = ((d.y * s) / sensor_h + 0.5) * y_res
// false (fx = fy = 0): the point is not in front of the camera (!(d.z > 0): behind, at the camera, NaN) or a coordinate is not finite.
ER_RP_HD inline bool er_history_project(const ErReprojCam& c, uint32_t x_res, uint32_t y_res, const float* p, float* fx, float* fy) {
    const float vx = p[0] - c.pos[0], vy = p[1] - c.pos[1], vz = p[2] - c.pos[2];
    const float yx = vx * c.cz + vy * c.sz, yy = vy * c.cz - vx * c.sz, yz = vz;            // Z undone
    const float xx = yx * c.cy - yz * c.sy, xy = yy, xz = yx * c.sy + yz * c.cy;            // Y undone
    const float dx = xx, dy = xy * c.cx + xz * c.sx, dz = xz * c.cx - xy * c.sx;            // X undone
    *fx = 0.0f; *fy = 0.0f;
    if (!(dz > 0.0f)) return false;
    const float s = c.focal / dz;
    const float gx = ((dx * s) / c.sensor_w + 0.5f) * (float)x_res;
    const float gy = ((dy * s) / c.sensor_h + 0.5f) * (float)y_res;
    if (!er_rp_finite(gx) || !er_rp_finite(gy)) return false;
    *fx = gx; *fy = gy;
    return true;
}

// Where the surface point under a pixel was at the capture.  A hit: B P if its object moved (B = the object's back matrix, applied with
// er_xform_point), P bit for bit if it did not (`moved` 0: the two poses are bitwise equal, or the object is ER_HISTORY_NONE).  A miss:
// the captured camera's position + the ray's direction -- a point one unit along the same direction, which is where sky stays.
ER_RP_HD inline void er_history_old_point(const ErHistoryKey& k, const float* back /*[12] or NULL*/, uint32_t moved, const float* old_cam_pos, float* out) {
    if (!k.hit) { for (int i = 0; i < 3; i++) out[i] = old_cam_pos[i] + k.P[i]; return; }
    if (moved && back) { er_xform_point(back, k.P, out); return; }
    for (int i = 0; i < 3; i++) out[i] = k.P[i];
}

// One tap: the captured key at an integer pixel against what the new pixel expects there.  d_exp = |P_old - old camera position|.
ER_RP_HD inline int er_history_tap_state(bool inside, uint32_t new_hit, uint32_t new_object, float d_exp, float tol, uint32_t old_hit, uint32_t old_object, float old_dist) {
    if (!inside) return ER_TAP_OUTSIDE;
    if ((new_hit != 0u) != (old_hit != 0u)) return ER_TAP_FLAG;
    if (!new_hit) return ER_TAP_VALID;
    if (new_object != old_object) return ER_TAP_OBJECT;
    if (!(fabsf(d_exp - old_dist) <= tol * d_exp)) return ER_TAP_DEPTH;
    return ER_TAP_VALID;
}

// The four bilinear taps around (fx, fy), in the order (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), x0 = floor(fx), with the
// weights (1 - tx)(1 - ty), tx (1 - ty), (1 - tx) ty, tx ty, tx = fx - x0.  Returns false -- every tap ER_TAP_OUTSIDE, x = y = 0, weight
// 0 -- if `projected` is false or no tap can lie inside the frame (!(fx > -1 && fx < x_res), the same for y); else tap_x / tap_y [4] are
// the taps' pixels (each in [-1, res]) and inside[4] says which are pixels of the frame.
ER_RP_HD inline bool er_history_tap_geometry(bool projected, float fx, float fy, uint32_t x_res, uint32_t y_res, int* tap_x, int* tap_y, float* tap_w, bool* inside) {
    const bool near = projected && fx > -1.0f && fx < (float)x_res && fy > -1.0f && fy < (float)y_res;
    if (!near) {
        for (int k = 0; k < 4; k++) { tap_x[k] = 0; tap_y[k] = 0; tap_w[k] = 0.0f; inside[k] = false; }
        return false;
    }
    const float flx = floorf(fx), fly = floorf(fy);
    const float tx = fx - flx, ty = fy - fly;
    const float ux = 1.0f - tx, uy = 1.0f - ty;
    const int x0 = (int)flx, y0 = (int)fly;
    tap_w[0] = ux * uy; tap_w[1] = tx * uy; tap_w[2] = ux * ty; tap_w[3] = tx * ty;
    for (int k = 0; k < 4; k++) {
        tap_x[k] = x0 + (k & 1); tap_y[k] = y0 + (k >> 1);
        inside[k] = tap_x[k] >= 0 && tap_x[k] < (int)x_res && tap_y[k] >= 0 && tap_y[k] < (int)y_res;
    }
    return true;
}

// The class of a pixel from its four tap states.
ER_RP_HD inline int er_history_class(uint32_t new_hit, const int* state) {
    if (!new_hit) return ER_HC_SKY;
    int valid = 0, outside = 0;
    for (int k = 0; k < 4; k++) { valid += state[k] == ER_TAP_VALID; outside += state[k] == ER_TAP_OUTSIDE; }
    if (valid == 4) return ER_HC_VALID;
    if (valid > 0) return ER_HC_PARTIAL;
    return outside == 4 ? ER_HC_OFFSCREEN : ER_HC_REJECTED;
}

// The bilinear mean over the valid taps, weights renormalised: cw[k] = the captured (C.rgb, W) at tap k (read only where state[k] is
// ER_TAP_VALID).  out = (rgb, w); all four 0 if no tap is valid or the valid taps' weights sum to 0.
ER_RP_HD inline void er_history_mean(const int* state, const float* tap_w, const float (*cw)[4], float* out) {
    float ws = 0.0f, acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 4; k++) {
        const bool v = state[k] == ER_TAP_VALID;
        ws = ws + (v ? tap_w[k] : 0.0f);
        for (int c = 0; c < 4; c++) acc[c] = acc[c] + (v ? tap_w[k] * cw[k][c] : 0.0f);
    }
    const bool any = ws > 0.0f;
    for (int c = 0; c < 4; c++) out[c] = any ? acc[c] / ws : 0.0f;
}

// The render's mean of a pixel without the setup sample: the planes hold sum / (n + 1) (accumulate_sample, er_shade.h), n = samples - 1.
ER_RP_HD inline void er_history_render_mean(const float* beauty_rgb, uint32_t samples, float* m, float* nf) {
    const uint32_t n = samples > 0u ? samples - 1u : 0u;
    *nf = (float)n;
    const float scale = n > 0u ? (float)samples / (float)n : 0.0f;
    for (int c = 0; c < 3; c++) m[c] = n > 0u ? beauty_rgb[c] * scale : 0.0f;
}

// (w H + n m) / (w + n); false (out = 0) where w + n = 0
ER_RP_HD inline bool er_history_mix(const float* H, float w, const float* m, float nf, float* out) {
    const float sum = w + nf;
    const bool any = sum > 0.0f;
    for (int c = 0; c < 3; c++) out[c] = any ? (w * H[c] + nf * m[c]) / sum : 0.0f;
    return any;
}

// One pixel of a capture: hist = the pixel's resolved (H.rgb, w) or NULL (none valid: w = 0) -> out = (C.rgb, W)
ER_RP_HD inline void er_history_capture_px(const float* beauty_rgb, uint32_t samples, const float* hist, float max_weight, float* out) {
    float m[3], nf;
    er_history_render_mean(beauty_rgb, samples, m, &nf);
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const float w = hist ? hist[3] : 0.0f;
    er_history_mix(hist ? hist : zero, w, m, nf, out);
    const float sum = w + nf;
    out[3] = sum < max_weight ? sum : max_weight;
}

// One pixel of er_read_blended: hist = (H.rgb, w) -> out = (rgb, 1); the setup colour (BEAUTY as it lies) where w + n = 0
ER_RP_HD inline void er_history_blend_px(const float* beauty_rgb, uint32_t samples, const float* hist, float* out) {
    float m[3], nf;
    er_history_render_mean(beauty_rgb, samples, m, &nf);
    if (!er_history_mix(hist, hist[3], m, nf, out))
        for (int c = 0; c < 3; c++) out[c] = beauty_rgb[c];
    out[3] = 1.0f;
}

// The four taps of one pixel of a resolve: their states, their bilinear weights and their pixels in the captured frame (q: 0 for a tap
// outside it, which is never read).  What every plane carried beside the colour is gathered through (er_history_variance.h).
ER_RP_HD inline void er_history_tap_set(const ErHistoryKey& k, const float* back, uint32_t moved, const ErReprojCam& cam, uint32_t x_res, uint32_t y_res, float tol,
                                        const uint32_t* old_hit, const uint32_t* old_object, const float* old_dist, int* state /*[4]*/, float* tw /*[4]*/, size_t* q /*[4]*/) {
    float Po[3], fx, fy;
    er_history_old_point(k, back, moved, cam.pos, Po);
    const bool projected = er_history_project(cam, x_res, y_res, Po, &fx, &fy);
    const float d_exp = er_rp_length(Po[0] - cam.pos[0], Po[1] - cam.pos[1], Po[2] - cam.pos[2]);
    int tx[4], ty[4];
    bool inside[4];
    er_history_tap_geometry(projected, fx, fy, x_res, y_res, tx, ty, tw, inside);
    for (int t = 0; t < 4; t++) {
        q[t] = inside[t] ? (size_t)ty[t] * x_res + (size_t)tx[t] : 0;
        state[t] = er_history_tap_state(inside[t], k.hit, k.object, d_exp, tol, inside[t] ? old_hit[q[t]] : 0u, inside[t] ? old_object[q[t]] : 0u, inside[t] ? old_dist[q[t]] : 0.0f);
    }
}

// One pixel of a resolve, from plain arrays: the new key k, the object's back matrix, the captured camera, the captured key plane
// (old_hit / old_object / old_dist, row-major) and the captured (C, W) plane.  out = (H.rgb, w); returns the pixel's class.  What the
// device kernel runs per work item and what er_debug_history_taps runs per query.
ER_RP_HD inline int er_history_resolve_px(const ErHistoryKey& k, const float* back, uint32_t moved, const ErReprojCam& cam, uint32_t x_res, uint32_t y_res, float tol,
                                          const uint32_t* old_hit, const uint32_t* old_object, const float* old_dist, const float* old_cw /*[npx][4]*/, float* out,
                                          int* state_out /*[4] or NULL*/) {
    int state[4];
    float tw[4], cw[4][4];
    size_t q[4];
    er_history_tap_set(k, back, moved, cam, x_res, y_res, tol, old_hit, old_object, old_dist, state, tw, q);
    for (int t = 0; t < 4; t++) {
        for (int c = 0; c < 4; c++) cw[t][c] = state[t] == ER_TAP_VALID ? old_cw[q[t] * 4 + c] : 0.0f;
        if (state_out) state_out[t] = state[t];
    }
    er_history_mean(state, tw, cw, out);
    return er_history_class(k.hit, state);
}

// ---- host only from here on ----

// B = M_capture o M_now^-1 as a row-major 3x4 matrix: in double, from the cofactor form er_xform_derive uses (L_now^-1 = C^T / det),
// every product and sum rounded by itself in the written order, rounded to float once.  false: an entry is not finite or det(L_now) is
// not > 0 (cannot happen for poses er_render_transform accepted).
inline bool er_history_back_matrix(const float* m_cap, const float* m_now, float* out) {
    for (int k = 0; k < 12; k++) if (!std::isfinite(m_cap[k]) || !std::isfinite(m_now[k])) return false;
    double L[9], C[9], A[9], I[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { L[3 * i + j] = (double)m_now[4 * i + j]; A[3 * i + j] = (double)m_cap[4 * i + j]; }
    C[0] = L[4] * L[8] - L[5] * L[7];
    C[1] = L[5] * L[6] - L[3] * L[8];
    C[2] = L[3] * L[7] - L[4] * L[6];
    C[3] = L[2] * L[7] - L[1] * L[8];
    C[4] = L[0] * L[8] - L[2] * L[6];
    C[5] = L[1] * L[6] - L[0] * L[7];
    C[6] = L[1] * L[5] - L[2] * L[4];
    C[7] = L[2] * L[3] - L[0] * L[5];
    C[8] = L[0] * L[4] - L[1] * L[3];
    const double det = (L[0] * C[0] + L[1] * C[1]) + L[2] * C[2];
    if (!(det > 0)) return false;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) I[3 * i + j] = C[3 * j + i] / det;      // L_now^-1
    for (int i = 0; i < 3; i++) {
        double R[3];
        for (int j = 0; j < 3; j++) R[j] = (A[3 * i] * I[j] + A[3 * i + 1] * I[3 + j]) + A[3 * i + 2] * I[6 + j];
        const double t = (double)m_cap[4 * i + 3] - ((R[0] * (double)m_now[3] + R[1] * (double)m_now[7]) + R[2] * (double)m_now[11]);
        for (int j = 0; j < 3; j++) out[4 * i + j] = (float)R[j];
        out[4 * i + 3] = (float)t;
    }
    return true;
}

inline bool er_history_same_pose(const float* a, const float* b) { return memcmp(a, b, 12 * sizeof(float)) == 0; }      // bitwise
