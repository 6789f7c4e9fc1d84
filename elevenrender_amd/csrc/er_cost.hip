// er_cost.hip -- the structure's measured cost on the device (er_cost.h): what er_accel_cost reports and what er_render_update judges a
// refit by under ER_REBUILD_AUTO.
//
//   1. nodes     one thread per wide node: the 80 bytes as five 16-byte loads at the buffer's stride, node_i and leaf_i with the
//                arithmetic of er_cost.h into a temporary, and the root's area from node 0;
//   2. records   one thread per record: tri_k into a temporary;
//   3. sums      every workgroup of 1. and 2. adds its own terms -- per wave a shuffle reduction of a fixed pattern, the four waves
//                through LDS in ascending order -- and STORES the partial sum; the host adds the partials in ascending order.
//
// No float or double atomics and no workgroup that waits for another (er_refit.hip's rule): the order of every addition is fixed by
// the indices alone, so two measurements of the same bytes return the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "er_cost.h"

namespace {

__device__ __forceinline__ double wave_sum(double v) {      // lane 0 holds the sum
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// the sum of `v` over the 256 threads of the workgroup, valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* lds4) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void k_cost_nodes(const float4* __restrict__ nodes8, uint32_t node8_count, double2* __restrict__ terms, double2* __restrict__ partial,
                                                     double* __restrict__ root) {
    __shared__ double lds[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    double node = 0.0, leaf = 0.0;
    if (i < node8_count) {
        const float4* q = nodes8 + (size_t)i * ER_NODE8_PIECES;
        float4 w[5];
        for (int k = 0; k < 5; k++) w[k] = q[k];
        ErNode8 nd;
        __builtin_memcpy(&nd, w, sizeof(ErNode8));
        float r = 0.0f;
        ercost::node_terms(nd, &node, &leaf, i == 0 ? &r : nullptr);
        terms[i] = make_double2(node, leaf);
        if (i == 0) *root = (double)r;
    }
    const double sn = block_sum(node, lds), sl = block_sum(leaf, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = make_double2(sn, sl);
}

__global__ __launch_bounds__(256) void k_cost_records(const ErTriIsect* __restrict__ isect, uint32_t n, float* __restrict__ terms, double* __restrict__ partial) {
    __shared__ double lds[4];
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    float t = 0.0f;
    if (k < n) {
        const float4* q = (const float4*)(isect + k);
        float4 w[3];
        for (int j = 0; j < 3; j++) w[j] = q[j];
        ErTriIsect r;
        __builtin_memcpy(&r, w, sizeof(ErTriIsect));
        t = ercost::record_term(r, n);
        terms[k] = t;
    }
    const double s = block_sum((double)t, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

template <class T>
struct Tmp {
    T* p = nullptr;
    Tmp() = default;
    Tmp(const Tmp&) = delete;
    Tmp& operator=(const Tmp&) = delete;
    ~Tmp() { if (p) (void)hipFree(p); }
};
struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

#define CO_OK(x)                                                                             \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) { err = std::string(#x) + ": " + hipGetErrorString(e_); return e_ == hipErrorOutOfMemory ? -2 : -1; } \
    } while (0)

}  // namespace

hipError_t er_probe_cost(const char** which) {
    hipFuncAttributes at;
    *which = "k_cost_nodes (er_cost.hip)";
    return hipFuncGetAttributes(&at, (const void*)k_cost_nodes);
}

int er_cost_device(const float4* nodes8, uint32_t node8_count, const ErTriIsect* isect, uint32_t tri_count, hipStream_t st, ErCostSums* out, double* node_terms,
                   float* tri_terms, std::string& err) {
    *out = ErCostSums{};
    const uint32_t N = nodes8 ? node8_count : 0u, n = isect ? tri_count : 0u;
    const uint32_t nb = (N + 255) / 256, tb = (n + 255) / 256;
    Events ev;
    CO_OK(hipEventCreate(&ev.a));
    CO_OK(hipEventCreate(&ev.b));
    // one allocation: [node terms N x 16 | node partials nb x 16 | record partials tb x 8 | root 8 | record terms n x 4], widest alignment first
    Tmp<char> d_all;
    const size_t o_npart = (size_t)N * sizeof(double2), o_tpart = o_npart + (size_t)nb * sizeof(double2), o_root = o_tpart + (size_t)tb * sizeof(double),
                 o_tterms = o_root + sizeof(double), total = o_tterms + (size_t)n * sizeof(float);
    CO_OK(hipMalloc((void**)&d_all.p, total));
    double2* const d_nterms = (double2*)d_all.p;
    double2* const d_npart = (double2*)(d_all.p + o_npart);
    double* const d_tpart = (double*)(d_all.p + o_tpart);
    double* const d_root = (double*)(d_all.p + o_root);
    float* const d_tterms = (float*)(d_all.p + o_tterms);
    CO_OK(hipEventRecord(ev.a, st));
    CO_OK(hipMemsetAsync(d_root, 0, sizeof(double), st));
    if (nb) hipLaunchKernelGGL(k_cost_nodes, dim3(nb), dim3(256), 0, st, nodes8, N, d_nterms, d_npart, d_root);
    if (tb) hipLaunchKernelGGL(k_cost_records, dim3(tb), dim3(256), 0, st, isect, n, d_tterms, d_tpart);
    CO_OK(hipGetLastError());
    CO_OK(hipEventRecord(ev.b, st));
    std::vector<double2> npart(nb);
    std::vector<double> tpart(tb);
    double root = 0.0;
    if (nb) CO_OK(hipMemcpyAsync(npart.data(), d_npart, (size_t)nb * sizeof(double2), hipMemcpyDeviceToHost, st));
    if (tb) CO_OK(hipMemcpyAsync(tpart.data(), d_tpart, (size_t)tb * sizeof(double), hipMemcpyDeviceToHost, st));
    CO_OK(hipMemcpyAsync(&root, d_root, sizeof(double), hipMemcpyDeviceToHost, st));
    if (node_terms && N) CO_OK(hipMemcpyAsync(node_terms, d_nterms, (size_t)N * sizeof(double2), hipMemcpyDeviceToHost, st));
    if (tri_terms && n) CO_OK(hipMemcpyAsync(tri_terms, d_tterms, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
    CO_OK(hipStreamSynchronize(st));
    double sn = 0.0, sl = 0.0, stri = 0.0;      // the partials, ascending
    for (uint32_t b = 0; b < nb; b++) { sn += npart[b].x; sl += npart[b].y; }
    for (uint32_t b = 0; b < tb; b++) stri += tpart[b];
    out->node_area = root + sn;
    out->leaf_area = sl;
    out->tri_area = stri;
    out->cost = n ? ercost::cost_of(out->node_area, out->leaf_area, out->tri_area) : 0.0;
    (void)hipEventElapsedTime(&out->ms, ev.a, ev.b);
    return 0;
}

void er_cost_host(const void* nodes8, uint32_t node8_count, uint32_t pieces, const ErTriIsect* isect, uint32_t tri_count, ErCostSums* out, double* node_terms,
                  float* tri_terms) {
    *out = ErCostSums{};
    double sn = 0.0, sl = 0.0, stri = 0.0;
    float root = 0.0f;
    for (uint32_t i = 0; nodes8 && i < node8_count; i++) {
        ErNode8 nd;
        memcpy(&nd, (const char*)nodes8 + (size_t)i * pieces * 16, sizeof(ErNode8));
        double node, leaf;
        ercost::node_terms(nd, &node, &leaf, i == 0 ? &root : nullptr);
        if (node_terms) { node_terms[2 * (size_t)i] = node; node_terms[2 * (size_t)i + 1] = leaf; }
        sn += node;
        sl += leaf;
    }
    for (uint32_t k = 0; isect && k < tri_count; k++) {
        const float t = ercost::record_term(isect[k], tri_count);
        if (tri_terms) tri_terms[k] = t;
        stri += (double)t;
    }
    out->node_area = (double)root + sn;
    out->leaf_area = sl;
    out->tri_area = stri;
    out->cost = tri_count ? ercost::cost_of(out->node_area, out->leaf_area, out->tri_area) : 0.0;
}
