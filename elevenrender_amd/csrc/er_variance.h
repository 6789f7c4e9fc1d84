// er_variance.h -- the per-pixel variance of BEAUTY by batch means, and the colour stop it gives the a-trous filter (include/eleven_hip.h
// er_variance_fold, er_variance_info, er_read_variance, er_denoise_variance; er_variance.hip has the kernels and entry points).
// Every float32 operation is stated ONCE here, for the device kernels, for the tests (er_debug_variance_fold / _value / _level_px;
// elevenrender_amd/variance.py restates it in numpy) and for tests/native/variance_host.cpp, which compiles this file alone under
// ASan + UBSan.  Plain C++ plus __host__ __device__, without a HIP or library header.  Nothing is contracted (-ffp-contract=off): every
// product, quotient and sum is rounded by itself in the written order.
//
// A pixel's BEAUTY is a running mean with a known count: I <- I * sa / (sa + 1) + L / (sa + 1), sa starting at 1, so I * M is the sum of
// its samples and the mean J of the samples between two read points follows from the two plane values.  The scatter of those batch means
// estimates the variance (West's weighted update: E[M2] = (K - 1) * sigma^2 of the per-sample variance sigma^2, whatever the batch sizes).
//
// State of a pixel, 12 words (three float4): { S.r, S.g, S.b, m } { mu.r, mu.g, mu.b, W } { M2.r, M2.g, M2.b, K } -- m and K are uint32
// words, the others float32.
//   mark  (I, M):  S = I, m = M, mu = M2 = 0, W = 0, K = 0
//   fold  (I, M):  n = M - m (uint32).  n == 0: all 12 words stay.  Otherwise, per channel c, with fM = (float)M, fm = (float)m, fn = (float)n:
//                    J   = (I * fM - S * fm) / fn
//                    W'  = W + fn
//                    d   = J - mu
//                    mu' = mu + d * (fn / W')
//                    M2' = M2 + fn * (d * (J - mu'))
//                  then K' = K + 1, S = I, m = M.
//   value (M):     K < 2: (0, 0, 0).  Otherwise v = max(0, ((M2 / (float)(K - 1)) * (float)(M - 1)) / ((float)M * (float)M)); w = (float)K.
//                  This is the variance of BEAUTY as stored at the count M (the setup sample counts in M and adds no scatter).
// J is a difference of two products: its rounding error relative to I is about 2^-23 * M / n, harmless at interactive counts; renders of
// thousands of samples should fold in batches that grow with M.  A first batch's mu' = 0 + J * (fn / fn) is J exactly, so M2 stays 0;
// later fn / W' < 1 and mu' stays between mu and J (rounding is monotone), so every term of M2 is >= 0.  Only a first batch onto a mean
// that is not 0 -- which no reset leaves -- can land mu + d beyond J and give a negative term: the max(0, .) keeps the value total.
//
// The filter (er_variance_level_px): er_guided_level_kernel's 5 x 5 B3 stencil, tap order, normal, albedo and depth stops, with the colour
// stop normalised by the centre's variance and the variance carried to the next level.  On demodulated planes e (colour) and ve
// (variance; ve.w = 1 where the pixel's K >= 2, else 0), per centre p:
//     vb_c = the 3 x 3 (1,2,1)/4 x (1,2,1)/4 mean of ve_c at unit offsets, clamped coordinates, rows j = -1..1 then columns i = -1..1:
//            vb_c = vb_c + ve_q,c * (k3[i] * k3[j]), k3 = {0.25, 0.5, 0.25}
//     per tap q (j = -2..2 rows, i = -2..2, offsets i * step, j * step, clamped):
//         flag 0: wc = 1.  Otherwise d = e - e_q,
//             d2 = ((dx * dx) / (vb_x + 1e-8f) + (dy * dy) / (vb_y + 1e-8f)) + (dz * dz) / (vb_z + 1e-8f);   wc = 1 / (1 + kc * d2)
//         nd, wa, wz: er_guided_level_kernel's
//         wgt = ((((kernel[i] * kernel[j]) * wc) * (nd * nd)) * wa) * wz
//         s_c = s_c + e_q,c * wgt;  sw = sw + wgt;  t_c = t_c + (wgt * wgt) * ve_q,c
//     e' = (sx / sw, sy / sw, sz / sw, e.w);   ve' = (tx / (sw * sw), ty / (sw * sw), tz / (sw * sw), ve.w)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ER_VAR_HD __host__ __device__
#else
#define ER_VAR_HD
#endif

#define ER_VARIANCE_WORDS 12

// every plane is an array of float4: on the device a pixel's three or four floats come in one 16-byte load
#if defined(__HIP_DEVICE_COMPILE__)
#define ER_VAR_PX(ptr) ((const float*)__builtin_assume_aligned((ptr), 16))
#else
#define ER_VAR_PX(ptr) (ptr)
#endif

ER_VAR_HD inline uint32_t er_var_u(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
ER_VAR_HD inline float er_var_f(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

// st: the pixel's 12 words as floats (m at [3] and K at [11] are uint32 bit patterns)
ER_VAR_HD inline void er_variance_mark_px(const float* rgb, uint32_t M, float* st) {
    st[0] = rgb[0]; st[1] = rgb[1]; st[2] = rgb[2]; st[3] = er_var_f(M);
    for (int i = 4; i < 11; i++) st[i] = 0.0f;
    st[11] = er_var_f(0u);
}

// true if the pixel was folded (n != 0)
ER_VAR_HD inline bool er_variance_fold_px(const float* rgb, uint32_t M, float* st) {
    const uint32_t m = er_var_u(st[3]);
    const uint32_t n = M - m;
    if (n == 0u) return false;
    const float fM = (float)M, fm = (float)m, fn = (float)n;
    const float W1 = st[7] + fn;
    const float r = fn / W1;
    for (int c = 0; c < 3; c++) {
        const float J = (rgb[c] * fM - st[c] * fm) / fn;
        const float d = J - st[4 + c];
        const float mu = st[4 + c] + d * r;
        st[8 + c] = st[8 + c] + fn * (d * (J - mu));
        st[4 + c] = mu;
        st[c] = rgb[c];
    }
    st[7] = W1;
    st[11] = er_var_f(er_var_u(st[11]) + 1u);
    st[3] = er_var_f(M);
    return true;
}

ER_VAR_HD inline void er_variance_value_px(const float* st, uint32_t M, float* out) {
    const uint32_t K = er_var_u(st[11]);
    out[3] = (float)K;
    if (K < 2u) { out[0] = out[1] = out[2] = 0.0f; return; }
    const float fk = (float)(K - 1u), fm1 = (float)(M - 1u), fM = (float)M;
    const float mm = fM * fM;
    for (int c = 0; c < 3; c++) {
        const float v = ((st[8 + c] / fk) * fm1) / mm;
        out[c] = v > 0.0f ? v : 0.0f;      // (a NaN becomes 0 too)
    }
}

// the split's second plane: v over (albedo + 0.01)^2 per channel, and the flag
ER_VAR_HD inline void er_variance_split_px(const float* v /*[4]: value_px*/, const float* albedo, float* ve) {
    for (int c = 0; c < 3; c++) {
        const float a = albedo[c] + 0.01f;
        ve[c] = v[c] / (a * a);
    }
    ve[3] = v[3] >= 2.0f ? 1.0f : 0.0f;
}

// One pixel of one level.  Planes are float4 arrays given as float pointers with a stride in floats per pixel (e, ve, albedo, depth: 4;
// normal: 4 on a plane, 16 in the interleaved passes).  `depth` is read at .x.
ER_VAR_HD inline void er_variance_level_px(const float* e, const float* ve, const float* normal, size_t normal_stride, const float* albedo, const float* depth, int w, int h, int x,
                                           int y, int step, float kc, float ka, float kz, float* out_e, float* out_ve) {
    const float kernel[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const float k3[3] = {0.25f, 0.5f, 0.25f};
    const size_t p = (size_t)y * w + x;
    const float *c = ER_VAR_PX(e + p * 4), *n = ER_VAR_PX(normal + p * normal_stride), *a = ER_VAR_PX(albedo + p * 4);
    const float z = depth[p * 4];
    const bool known = ve[p * 4 + 3] != 0.0f;
    float vbx = 0.0f, vby = 0.0f, vbz = 0.0f;
    if (known) {
        for (int j = -1; j <= 1; j++)
            for (int i = -1; i <= 1; i++) {
                int qx = x + i, qy = y + j;
                qx = qx < 0 ? 0 : (qx >= w ? w - 1 : qx);
                qy = qy < 0 ? 0 : (qy >= h ? h - 1 : qy);
                const float* vq = ER_VAR_PX(ve + ((size_t)qy * w + qx) * 4);
                const float k = k3[i + 1] * k3[j + 1];
                vbx = vbx + vq[0] * k; vby = vby + vq[1] * k; vbz = vbz + vq[2] * k;
            }
    }
    const float ex = vbx + 1e-8f, ey = vby + 1e-8f, ez = vbz + 1e-8f;
    float sx = 0, sy = 0, sz = 0, sw = 0, tx = 0, ty = 0, tz = 0;
    for (int j = -2; j <= 2; j++)
        for (int i = -2; i <= 2; i++) {
            int qx = x + i * step, qy = y + j * step;
            qx = qx < 0 ? 0 : (qx >= w ? w - 1 : qx);
            qy = qy < 0 ? 0 : (qy >= h ? h - 1 : qy);
            const size_t q = (size_t)qy * w + qx;
            const float *cq = ER_VAR_PX(e + q * 4), *vq = ER_VAR_PX(ve + q * 4), *nq = ER_VAR_PX(normal + q * normal_stride), *aq = ER_VAR_PX(albedo + q * 4);
            const float zq = depth[q * 4];
            float wc = 1.0f;
            if (known) {
                const float dx = c[0] - cq[0], dy = c[1] - cq[1], dz = c[2] - cq[2];
                const float d2 = ((dx * dx) / ex + (dy * dy) / ey) + (dz * dz) / ez;
                wc = 1.0f / (1.0f + kc * d2);
            }
            float nd = n[0] * nq[0] + n[1] * nq[1] + n[2] * nq[2];
            const bool none = (n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f), noneq = (nq[0] == 0.0f && nq[1] == 0.0f && nq[2] == 0.0f);
            nd = (none && noneq) ? 1.0f : (nd < 0.0f ? 0.0f : nd);
            const float ax = a[0] - aq[0], ay = a[1] - aq[1], az = a[2] - aq[2];
            const float a2 = ax * ax + ay * ay + az * az;
            const float wa = 1.0f / (1.0f + a2 * ka);
            const float r = (z - zq) / (__builtin_fmaxf(z, zq) + 1e-6f);
            const float wz = 1.0f / (1.0f + (r * r) * kz);
            const float wgt = kernel[i + 2] * kernel[j + 2] * wc * (nd * nd) * wa * wz;
            const float w2 = wgt * wgt;
            sx = sx + cq[0] * wgt; sy = sy + cq[1] * wgt; sz = sz + cq[2] * wgt; sw = sw + wgt;
            tx = tx + w2 * vq[0]; ty = ty + w2 * vq[1]; tz = tz + w2 * vq[2];
        }
    const float ss = sw * sw;
    out_e[0] = sx / sw; out_e[1] = sy / sw; out_e[2] = sz / sw; out_e[3] = c[3];
    out_ve[0] = tx / ss; out_ve[1] = ty / ss; out_ve[2] = tz / ss; out_ve[3] = ve[p * 4 + 3];
}
