// er_build_dev.h -- the device arithmetic that the builder (er_gpu_build.hip) and the refit (er_refit.hip) share: the scene's largest
// coordinate, a triangle's padded box and lift bound, the scene bounds, and a wide node's origin, exponents and outward-quantised child
// boxes.  One implementation, so that a refitted structure holds exactly what a fresh build of the same arrays would compute for these.
// Include from a .hip file only; everything here has internal linkage (each translation unit carries its own kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "er_bvh.h"

namespace {

struct Box3 { float lo[3], hi[3]; };

__device__ __forceinline__ unsigned f2ord(float f) {   // order-preserving map float -> unsigned
    unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
inline float er_ord2f_host(unsigned u) {               // the host side of ord2f
    const unsigned b = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}

// pass 1: largest |coordinate| (the absolute part of the box padding, as er_build_bvh)
__global__ __launch_bounds__(256) void k_scene_bounds(const float* __restrict__ v, uint32_t n, unsigned* g /* [0] vmax bits */) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    float vm = 0;
    if (i < n) {
        const float* p = v + (size_t)i * 9;
        for (int k = 0; k < 9; k++) vm = fmaxf(vm, fabsf(p[k]));
    }
    for (int off = 32; off >= 1; off >>= 1) vm = fmaxf(vm, __shfl_xor(vm, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(&g[0], __float_as_uint(vm));     // vm >= 0: the bit pattern orders like the value
}

// One triangle's padded box and the term of the scene's lift maximum (er_build_bvh's arithmetic, reference src/Tri.h:106-112): p = its
// [3][3] vertices, nn = its [3][3] normals, pad_abs = the scene's largest |coordinate| x 1e-6.  k_prims and the sparse refit
// (er_refit.hip) both call these: one implementation.
__device__ __forceinline__ void prim_padded_box(const float* p, float pad_abs, Box3* b) {
    for (int a = 0; a < 3; a++) {
        float lo = fminf(fminf(p[a], p[3 + a]), p[6 + a]), hi = fmaxf(fmaxf(p[a], p[3 + a]), p[6 + a]);
        float m = fmaxf(fabsf(lo), fabsf(hi));
        float pad = fmaxf(m * 4e-7f + 1e-37f, pad_abs);
        float bl = lo - pad, bh = hi + pad;      // rounded outward, as er_build_bvh does
        if ((double)bl > (double)lo - (double)pad) bl = nextafterf(bl, -INFINITY);
        if ((double)bh < (double)hi + (double)pad) bh = nextafterf(bh, INFINITY);
        b->lo[a] = bl;
        b->hi[a] = bh;
    }
}
// (float)(tl * 1.01); the record's lift is that + 1e-30f
__device__ __forceinline__ float prim_lift(const float* p, const float* nn) {
    double tl = 0;
    for (int j = 0; j < 3; j++) {
        double nx = nn[3 * j], ny = nn[3 * j + 1], nz = nn[3 * j + 2];
        double nl = sqrt(nx * nx + ny * ny + nz * nz);
        for (int k = 0; k < 3; k++) {
            if (k == j) continue;
            double dx = (double)p[3 * k] - p[3 * j], dy = (double)p[3 * k + 1] - p[3 * j + 1], dz = (double)p[3 * k + 2] - p[3 * j + 2];
            double l = fabs(dx * nx + dy * ny + dz * nz) * nl;
            if (l > tl) tl = l;
        }
    }
    return (float)(tl * 1.01);
}

// pass 2: padded box, lift bound
__global__ __launch_bounds__(256) void k_prims(const float* __restrict__ v, const float* __restrict__ nrm, uint32_t n, const unsigned* __restrict__ g,
                                                Box3* __restrict__ boxes, float* __restrict__ lift, unsigned* __restrict__ lift_max,
                                                unsigned* __restrict__ bounds /* lo[3], hi[3] of all padded boxes, order-preserving integers */) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    float my_lift = 0;
    float slo[3] = {INFINITY, INFINITY, INFINITY}, shi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < n) {
        const float pad_abs = __uint_as_float(g[0]) * 1e-6f;
        const float* p = v + (size_t)i * 9;
        Box3 b;
        prim_padded_box(p, pad_abs, &b);
        for (int a = 0; a < 3; a++) { slo[a] = b.lo[a]; shi[a] = b.hi[a]; }
        boxes[i] = b;
        my_lift = prim_lift(p, nrm + (size_t)i * 9);
        lift[i] = my_lift + 1e-30f;
    }
    for (int off = 32; off >= 1; off >>= 1) my_lift = fmaxf(my_lift, __shfl_xor(my_lift, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(lift_max, __float_as_uint(my_lift));
    // the scene bounds are the union of the padded boxes, as er_build_bvh's (until round 7 they were read off the root's child boxes, which
    // are a box of the builder's own choosing when every centroid coincides and the root is split by position)
    for (int off = 32; off >= 1; off >>= 1)
        for (int a = 0; a < 3; a++) { slo[a] = fminf(slo[a], __shfl_xor(slo[a], off, 64)); shi[a] = fmaxf(shi[a], __shfl_xor(shi[a], off, 64)); }
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; a++) { atomicMin(&bounds[a], f2ord(slo[a])); atomicMax(&bounds[3 + a], f2ord(shi[a])); }
}

// A wide node's frame on one axis: origin p = lo, the smallest exponent e whose 255 steps of 2^e reach hi from there.
// Returns the step 2^e; *biased = e + 127 (ErNode8::e).
__device__ __forceinline__ float wide_axis_frame(float lo, float hi, uint8_t* biased) {
    const float ext = hi - lo;
    int e = 0;
    if (ext > 0) (void)frexpf(ext / 255.0f, &e); else e = -126;
    if (e < -126) e = -126;
    while (lo + 255.0f * ldexpf(1.0f, e) < hi) e++;
    *biased = (uint8_t)(e + 127);
    return ldexpf(1.0f, e);
}

// A child's bounds [clo, chi] on that axis as steps from p, rounded OUTWARD against the expression the decode uses (er_bvh.h ErNode8)
__device__ __forceinline__ void wide_axis_quantise(float p, float scale, float clo, float chi, uint8_t* qlo, uint8_t* qhi) {
    float fl = floorf((clo - p) / scale);
    float fh = ceilf((chi - p) / scale);
    int ql = (int)fminf(255.0f, fmaxf(0.0f, fl));
    int qh = (int)fminf(255.0f, fmaxf(0.0f, fh));
    while (ql > 0 && p + (float)ql * scale > clo) ql--;
    while (qh < 255 && p + (float)qh * scale < chi) qh++;
    *qlo = (uint8_t)ql;
    *qhi = (uint8_t)qh;
}

}  // namespace
