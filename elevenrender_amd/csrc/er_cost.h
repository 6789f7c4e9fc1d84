// er_cost.h -- a measured cost of the acceleration structure as it lies in memory (er_accel_cost, include/eleven_hip.h):
// the byte-weighted sum of the box areas a traversal tests, over the sum of the triangles' own box areas.  Translation and scale leave
// it alone; it rises when node boxes grow while the triangles do not, which is what a refit does to a tree whose triangles scattered.
//
// The arithmetic below is compiled unchanged by the device (er_cost.hip) and the host (er_debug_accel_cost_host): every area is
// float32 with the association written here (build with -ffp-contract=off, as everything in this directory), every sum float64.
//   area(lo, hi)  d = hi - lo per axis, (d.x * d.y + d.y * d.z) + d.z * d.x
//   decoded box   per plane float(p + float(q * 2^(e - 127))), the expression of er_bvh.h ErNode8
//   node_i        sum over inner slots, ascending, of the slot's decoded area
//   leaf_i        sum over leaf slots with 1 or 2 triangles, ascending, of area x count
//   root          area of the union of node 0's occupied decoded boxes
//   tri_k         area of the box of record k's three vertices; 0 for a record that names no triangle
//   cost          (sizeof(ErNode8) * (root + sum node_i) + sizeof(ErTriIsect) * sum leaf_i) / sum tri_k, 0 where that sum is 0
#pragma once
#include <stdint.h>

#include <string>

#include "er_bvh.h"

#if defined(__HIPCC__)
#define ER_COST_HD __host__ __device__ inline
#else
#define ER_COST_HD inline
#endif

namespace ercost {

ER_COST_HD float area(const float lo[3], const float hi[3]) {
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return (dx * dy + dy * dz) + dz * dx;
}

// 2^(e - 127) for a biased exponent byte, as tests/accel_check.py decode_wide_boxes evaluates it: the bit pattern e << 23 for e >= 1.
// e == 0 is the one byte at which the two readings of ErNode8's comment part: the value 2^-127 is a subnormal (taken here, as the
// checker does), its "bit pattern e << 23" is 0.0 (what the traversal forms, er_trav.h).  No builder and no refit writes it
// (wide_axis_frame keeps e - 127 >= -126), and a box 255 x 2^-127 wide has no area in float32 either way.
ER_COST_HD float scale_of(uint8_t e) {
    return __builtin_bit_cast(float, e ? (uint32_t)e << 23 : 0x00400000u);
}

// node_i, leaf_i of one wide node; *root (may be null) = the area of the union of its occupied decoded boxes, 0 if it has none
ER_COST_HD void node_terms(const ErNode8& nd, double* node, double* leaf, float* root) {
    const float sc[3] = {scale_of(nd.e[0]), scale_of(nd.e[1]), scale_of(nd.e[2])};
    float ulo[3] = {0, 0, 0}, uhi[3] = {0, 0, 0};
    bool any = false;
    double n = 0.0, l = 0.0;
    for (int s = 0; s < 8; s++) {
        const bool inner = (nd.imask >> s) & 1u;
        const uint32_t cnt = ((nd.tri_present >> (2 * s)) & 1u) + ((nd.tri_present >> (2 * s + 1)) & 1u);
        if (!inner && cnt == 0) continue;
        float lo[3], hi[3];
        for (int a = 0; a < 3; a++) {
            lo[a] = nd.p[a] + (float)nd.qlo[a][s] * sc[a];
            hi[a] = nd.p[a] + (float)nd.qhi[a][s] * sc[a];
        }
        const float ar = area(lo, hi);
        if (inner) n += (double)ar;
        else l += (double)ar * (double)cnt;
        for (int a = 0; a < 3; a++) {
            ulo[a] = any ? (lo[a] < ulo[a] ? lo[a] : ulo[a]) : lo[a];
            uhi[a] = any ? (hi[a] > uhi[a] ? hi[a] : uhi[a]) : hi[a];
        }
        any = true;
    }
    *node = n;
    *leaf = l;
    if (root) *root = any ? area(ulo, uhi) : 0.0f;
}

// tri_k of one intersection record of a structure over n triangles
ER_COST_HD float record_term(const ErTriIsect& r, uint32_t n) {
    if ((uint32_t)r.tri_id >= n) return 0.0f;
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        const float x = r.v0[a], y = r.v1[a], z = r.v2[a];
        const float mn = x < y ? x : y, mx = x > y ? x : y;
        lo[a] = z < mn ? z : mn;
        hi[a] = z > mx ? z : mx;
    }
    return area(lo, hi);
}

ER_COST_HD double cost_of(double node_area, double leaf_area, double tri_area) {
    if (!(tri_area > 0.0)) return 0.0;
    return ((double)sizeof(ErNode8) * node_area + (double)sizeof(ErTriIsect) * leaf_area) / tri_area;
}

}  // namespace ercost

struct ErCostSums {
    double node_area = 0, leaf_area = 0, tri_area = 0, cost = 0;
    float ms = 0;               // device time of the measurement (HIP events); 0 on the host
};

// The host compilation over arrays in host memory: nodes8 at a stride of `pieces` 16-byte pieces, tri_count records.  node_terms
// (2 doubles per node: node_i, leaf_i) and tri_terms (one float per record) may be null.  Sums are sequential, ascending.
void er_cost_host(const void* nodes8, uint32_t node8_count, uint32_t pieces, const ErTriIsect* isect, uint32_t tri_count, ErCostSums* out, double* node_terms,
                  float* tri_terms);

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// The device measurement of a structure in device memory (er_cost.hip); blocks until done.  node_terms / tri_terms: HOST arrays as
// above or null.  Returns 0; -2 = out of device memory, -1 = any other HIP error (`err` says which).  Two calls on the same bytes
// return the same bits: no atomics, one fixed order of additions.
int er_cost_device(const float4* nodes8, uint32_t node8_count, const ErTriIsect* isect, uint32_t tri_count, hipStream_t stream, ErCostSums* out, double* node_terms,
                   float* tri_terms, std::string& err);
hipError_t er_probe_cost(const char** which);   // see er_kernels.h
#endif
