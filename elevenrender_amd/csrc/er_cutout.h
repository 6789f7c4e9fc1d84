// er_cutout.h -- the rule by which the first-hit camera pass sees through cut-outs (include/eleven_hip.h er_first_hit_set; FirstHit::visible
// in er_first_hit.h walks with it).  Every float32 operation is stated ONCE here, for the device kernels, for the tests
// (er_debug_cutout_*; elevenrender_amd/first_hit.py restates it in numpy) and for tests/native/cutout_host.cpp, which compiles this file
// alone under ASan + UBSan.  Plain C++ plus __host__ __device__, without a HIP or library header.  Nothing is contracted
// (-ffp-contract=off): every product, quotient and sum is rounded by itself in the written order.
//
//   parameter:     a threshold of 0 (+0 or -0) means 0.5; otherwise it must lie in (0, 1].  NaN, a negative value and a value > 1 are refused.
//   stop:          a hit of opacity `a` stops the ray iff a >= threshold.  A NaN opacity passes (it fails the render's u <= opacity too);
//                  opacities below 0 pass and opacities above 1 stop whatever the threshold, as they do under every draw of the render.
//   continuation:  the render's own ray past a hit it passes through (er_bounce.inc: make_ray(hit.position + ray.d * 0.001f, ray.d)):
//                  o'_c = position_c + d_c * 0.001f;  l = sqrt((d_x * d_x + d_y * d_y) + d_z * d_z);  d'_c = l != 0 ? d_c / l : d_c
//                  (make_ray normalises again; the quotient is kept because it is not always the identity on a unit vector's bits).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ER_CO_HD __host__ __device__
#else
#define ER_CO_HD
#endif

#define ER_CUTOUT_DEFAULT_THRESHOLD 0.5f
#define ER_CUTOUT_STEP 0.001f      // er_bounce.inc's offset along the ray

ER_CO_HD inline bool er_cutout_threshold_ok(float t) { return t >= 0.0f && t <= 1.0f; }      // (false for NaN; -0 is 0)
ER_CO_HD inline float er_cutout_threshold(float t) { return t == 0.0f ? ER_CUTOUT_DEFAULT_THRESHOLD : t; }

ER_CO_HD inline bool er_cutout_stops(float opacity, float threshold) { return opacity >= threshold; }

ER_CO_HD inline void er_cutout_continue(const float* position, const float* d, float* o_out, float* d_out) {
    for (int c = 0; c < 3; c++) o_out[c] = position[c] + d[c] * ER_CUTOUT_STEP;
    const float l = __builtin_sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    for (int c = 0; c < 3; c++) d_out[c] = l != 0.0f ? d[c] / l : d[c];
}
