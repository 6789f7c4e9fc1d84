// er_refit.hip -- refit of the acceleration structure in place (er_refit.h): what er_render_update does instead of a build when the
// triangles of a begun scene moved.
//
//   1. bounds    k_scene_bounds + k_prims of er_build_dev.h, the builders' own passes: largest coordinate, padded box and lift per
//                triangle, the lift maximum, the scene bounds;
//   2. records   one thread per slot, gathering by the tri_id already in the record: vertices, lift, normals and tangents where given
//                (tri_id, sign, uv, material, pad and the sentinel record are not touched), and the slot's padded box for steps 3-4;
//   3. binary    bottom-up, one launch per level: a leaf child's box = the union of its slots' padded boxes, an inner child's box = the
//                union of that child's two boxes;
//   4. wide      bottom-up, one launch per level: the float box under every occupied slot (a leaf slot: its one or two triangles; an
//                inner slot: the union kept per wide node in a temporary), then origin, exponents and outward-quantised child boxes
//                with the builder's own functions.  imask, child_base, tri_base, tri_present, reserved and the slot assignment stay.
//
// Level-synchronous on purpose: a level's launch reads only what deeper launches on the same stream wrote, so no workgroup ever waits
// for another inside a kernel -- no arrival counters, no spinning, nothing that depends on when one XCD's L2 shows another's stores.
// The depth of every node is derived once per topology (top-down passes, then a counting sort on the host) and kept as index lists.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "er_build_dev.h"
#include "er_refit.h"

namespace {

constexpr uint32_t NO_DEPTH = 0xffffffffu;

__device__ __forceinline__ const ErNode8* node8_at(const float4* nodes8, uint32_t i) { return (const ErNode8*)(nodes8 + (size_t)i * ER_NODE8_PIECES); }
__device__ __forceinline__ bool ref_inner(int ref) { return ref >= 0 && ref != ER_BVH_NO_CHILD; }

// ---- topology: one top-down pass per level ----
__global__ __launch_bounds__(256) void k_depth2_pass(const ErNode* __restrict__ nodes, uint32_t count, uint32_t* depth, uint32_t pass) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count || depth[i] != pass) return;
    const int c[2] = {nodes[i].c0, nodes[i].c1};
    for (int k = 0; k < 2; k++)
        if (ref_inner(c[k]) && (uint32_t)c[k] < count && (uint32_t)c[k] != i) depth[c[k]] = pass + 1;
}

__global__ __launch_bounds__(256) void k_depth8_pass(const float4* __restrict__ nodes8, uint32_t count, uint32_t* depth, uint32_t pass) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count || depth[i] != pass) return;
    const ErNode8* nd = node8_at(nodes8, i);
    const uint32_t kids = (uint32_t)__popc((unsigned)nd->imask), base = nd->child_base;
    for (uint32_t k = 0; k < kids; k++) {
        const uint32_t c = base + k;
        if (c > i && c < count) depth[c] = pass + 1;      // (breadth-first layout: children lie behind their parent)
    }
}

// ---- records ----
__global__ __launch_bounds__(256) void k_refit_records(uint32_t n, const Box3* __restrict__ boxes, const float* __restrict__ lift, const float* __restrict__ v,
                                                        const float* __restrict__ nrm, const float* __restrict__ tan, ErTriIsect* isect, ErTriAttr* attr,
                                                        Box3* __restrict__ sbox) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    float4* q = (float4*)(isect + k);
    const float4 q0 = q[0], q2 = q[2];
    const uint32_t id = (uint32_t)__float_as_int(q0.w);
    if (id >= n) {      // a record that names no triangle constrains nothing
        Box3 e;
        for (int a = 0; a < 3; a++) { e.lo[a] = INFINITY; e.hi[a] = -INFINITY; }
        sbox[k] = e;
        return;
    }
    const float* p = v + (size_t)id * 9;
    q[0] = make_float4(p[0], p[1], p[2], q0.w);
    q[1] = make_float4(p[3], p[4], p[5], lift[id]);
    q[2] = make_float4(p[6], p[7], p[8], q2.w);
    if (nrm) for (int j = 0; j < 3; j++) for (int a = 0; a < 3; a++) attr[k].n[j][a] = nrm[(size_t)id * 9 + 3 * j + a];
    if (tan) for (int j = 0; j < 3; j++) for (int a = 0; a < 3; a++) attr[k].t[j][a] = tan[(size_t)id * 9 + 3 * j + a];
    sbox[k] = boxes[id];
}

__device__ __forceinline__ void box_empty(float* lo, float* hi) {
    for (int a = 0; a < 3; a++) { lo[a] = INFINITY; hi[a] = -INFINITY; }
}
__device__ __forceinline__ void box_add(float* lo, float* hi, const float* blo, const float* bhi) {
    for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], blo[a]); hi[a] = fmaxf(hi[a], bhi[a]); }
}
__device__ __forceinline__ void box_of_slots(const Box3* __restrict__ sbox, uint32_t n, uint32_t first, uint32_t count, float* lo, float* hi) {
    box_empty(lo, hi);
    for (uint32_t j = 0; j < count; j++)
        if (first + j < n) { const Box3 b = sbox[first + j]; box_add(lo, hi, b.lo, b.hi); }
}

// ---- binary tree, one level ----
__global__ __launch_bounds__(256) void k_refit_binary(ErNode* nodes, uint32_t node_count, const uint32_t* __restrict__ list, uint32_t m,
                                                       const Box3* __restrict__ sbox, uint32_t n) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const uint32_t i = list[t];
    if (i >= node_count) return;
    ErNode nd = nodes[i];
    const int c[2] = {nd.c0, nd.c1};
    for (int k = 0; k < 2; k++) {
        float lo[3], hi[3];
        if (c[k] < 0) {
            const uint32_t code = (uint32_t)~c[k];
            box_of_slots(sbox, n, code >> 3, (code & 7u) + 1u, lo, hi);
        } else if (ref_inner(c[k]) && (uint32_t)c[k] < node_count) {
            const ErNode ch = nodes[c[k]];      // (a deeper level: written by an earlier launch)
            box_empty(lo, hi);
            box_add(lo, hi, ch.lo0, ch.hi0);
            if (ch.c1 != ER_BVH_NO_CHILD) box_add(lo, hi, ch.lo1, ch.hi1);
        } else continue;                        // no child: its box stays as it is
        for (int a = 0; a < 3; a++) {
            if (k == 0) { nd.lo0[a] = lo[a]; nd.hi0[a] = hi[a]; } else { nd.lo1[a] = lo[a]; nd.hi1[a] = hi[a]; }
        }
    }
    nodes[i] = nd;
}

// ---- wide tree, one level ----
__global__ __launch_bounds__(256) void k_refit_wide(float4* nodes8, uint32_t node8_count, const uint32_t* __restrict__ list, uint32_t m,
                                                     const Box3* __restrict__ sbox, uint32_t n, Box3* nbox) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const uint32_t i = list[t];
    if (i >= node8_count) return;
    ErNode8* out = (ErNode8*)(nodes8 + (size_t)i * ER_NODE8_PIECES);
    ErNode8 nd = *out;
    float clo[8][3], chi[8][3];
    float lo[3], hi[3];
    box_empty(lo, hi);
    uint32_t occupied = 0, inner_rank = 0, tri_pos = nd.tri_base;
    for (int s = 0; s < 8; s++) {
        box_empty(clo[s], chi[s]);
        if ((nd.imask >> s) & 1u) {
            const uint32_t c = nd.child_base + inner_rank++;
            if (c < node8_count && c > i) { const Box3 b = nbox[c]; box_add(clo[s], chi[s], b.lo, b.hi); }      // (a deeper level: written by an earlier launch)
        } else {
            const uint32_t cnt = ((nd.tri_present >> (2 * s)) & 1u) + ((nd.tri_present >> (2 * s + 1)) & 1u);
            if (cnt == 0) continue;
            box_of_slots(sbox, n, tri_pos, cnt, clo[s], chi[s]);
            tri_pos += cnt;
        }
        if (!(clo[s][0] <= chi[s][0])) continue;      // nothing beneath (cannot happen in a structure that checks clean): the slot keeps its bytes
        occupied |= 1u << s;
        box_add(lo, hi, clo[s], chi[s]);
    }
    Box3 self;
    for (int a = 0; a < 3; a++) { self.lo[a] = lo[a]; self.hi[a] = hi[a]; }
    nbox[i] = self;
    if (!occupied) return;
    float scale[3];
    for (int a = 0; a < 3; a++) {
        nd.p[a] = lo[a];
        scale[a] = wide_axis_frame(lo[a], hi[a], &nd.e[a]);
    }
    for (int s = 0; s < 8; s++) {
        if (!((occupied >> s) & 1u)) continue;
        for (int a = 0; a < 3; a++) wide_axis_quantise(nd.p[a], scale[a], clo[s][a], chi[s][a], &nd.qlo[a][s], &nd.qhi[a][s]);
    }
    *out = nd;
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

#define RF_OK(x)                                                                             \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) { err = std::string(#x) + ": " + hipGetErrorString(e_); return e_ == hipErrorOutOfMemory ? -2 : -1; } \
    } while (0)

// depth array (read back) -> index list by level on the device + the levels' offsets
int level_lists(const std::vector<uint32_t>& depth, uint32_t max_levels, uint32_t** d_list, std::vector<uint32_t>& off, hipStream_t st, std::string& err) {
    uint32_t levels = 0;
    for (uint32_t d : depth)
        if (d != NO_DEPTH) {
            if (d >= max_levels) { err = "a node lies deeper than the traversal stacks allow"; return -1; }
            levels = std::max(levels, d + 1);
        }
    off.assign((size_t)levels + 1, 0u);
    for (uint32_t d : depth) if (d != NO_DEPTH) off[d + 1]++;
    for (uint32_t l = 0; l < levels; l++) off[l + 1] += off[l];
    std::vector<uint32_t> list(off[levels]), at(off.begin(), off.end() - (levels ? 1 : 0));
    for (uint32_t i = 0; i < (uint32_t)depth.size(); i++) if (depth[i] != NO_DEPTH) list[at[depth[i]]++] = i;
    RF_OK(hipMalloc((void**)d_list, std::max<size_t>(1, list.size()) * 4));
    if (!list.empty()) RF_OK(hipMemcpyAsync(*d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice, st));
    RF_OK(hipStreamSynchronize(st));      // (`list` goes out of scope)
    return 0;
}

int derive_topology(ErRefitTopo& topo, const ErRefitBuffers& b, hipStream_t st, std::string& err) {
    topo.release();
    const uint32_t zero = 0;
    for (int which = 0; which < 2; which++) {
        const uint32_t count = which == 0 ? b.node_count : b.node8_count;
        const uint32_t max_levels = which == 0 ? ER_BVH_MAX_DEPTH : ER_STACK8;
        const uint32_t passes = std::min<uint32_t>(which == 0 ? b.depth2 : b.depth8, max_levels);
        std::vector<uint32_t> depth(count);
        if (count) {
            Tmp<uint32_t> d_depth;
            RF_OK(hipMalloc((void**)&d_depth.p, (size_t)count * 4));
            RF_OK(hipMemsetAsync(d_depth.p, 0xff, (size_t)count * 4, st));
            RF_OK(hipMemcpyAsync(d_depth.p, &zero, 4, hipMemcpyHostToDevice, st));
            const uint32_t blocks = (count + 255) / 256;
            for (uint32_t pass = 0; pass < passes; pass++) {      // (one more than the levels need: it finds nothing)
                if (which == 0) hipLaunchKernelGGL(k_depth2_pass, dim3(blocks), dim3(256), 0, st, b.nodes, count, d_depth.p, pass);
                else hipLaunchKernelGGL(k_depth8_pass, dim3(blocks), dim3(256), 0, st, b.nodes8, count, d_depth.p, pass);
            }
            RF_OK(hipGetLastError());
            RF_OK(hipMemcpyAsync(depth.data(), d_depth.p, (size_t)count * 4, hipMemcpyDeviceToHost, st));
            RF_OK(hipStreamSynchronize(st));
        }
        int rc = level_lists(depth, max_levels, which == 0 ? &topo.d_lv2 : &topo.d_lv8, which == 0 ? topo.off2 : topo.off8, st, err);
        if (rc != 0) { topo.release(); return rc; }
    }
    topo.valid = true;
    return 0;
}

}  // namespace

hipError_t er_probe_refit(const char** which) {
    hipFuncAttributes at;
    *which = "k_refit_wide (er_refit.hip)";
    return hipFuncGetAttributes(&at, (const void*)k_refit_wide);
}

int er_refit_device(ErRefitTopo& topo, const ErRefitBuffers& b, const ErRefitArrays& a, hipStream_t st, ErRefitResult* out, std::string& err) {
    const uint32_t n = b.tri_count;
    *out = ErRefitResult{};
    if (n == 0) return 0;      // nothing to move: an empty structure stays an empty structure
    if (!a.vertices || !a.normals || !b.isect || !b.attr || !b.nodes8) { err = "refit: missing array"; return -1; }
    if (!topo.valid) {
        int rc = derive_topology(topo, b, st, err);
        if (rc != 0) return rc;
    }
    Events ev;
    RF_OK(hipEventCreate(&ev.a));
    RF_OK(hipEventCreate(&ev.b));
    Tmp<float> d_v, d_n, d_t, d_lift;
    Tmp<Box3> d_box, d_sbox, d_nbox;
    Tmp<unsigned> d_g;
    RF_OK(hipMalloc((void**)&d_v.p, (size_t)n * 36));
    RF_OK(hipMalloc((void**)&d_n.p, (size_t)n * 36));
    if (a.tangents) RF_OK(hipMalloc((void**)&d_t.p, (size_t)n * 36));
    RF_OK(hipMalloc((void**)&d_lift.p, (size_t)n * 4));
    RF_OK(hipMalloc((void**)&d_box.p, (size_t)n * sizeof(Box3)));
    RF_OK(hipMalloc((void**)&d_sbox.p, (size_t)n * sizeof(Box3)));
    RF_OK(hipMalloc((void**)&d_nbox.p, std::max<size_t>(1, b.node8_count) * sizeof(Box3)));
    RF_OK(hipMalloc((void**)&d_g.p, 12 * 4));
    RF_OK(hipEventRecord(ev.a, st));
    RF_OK(hipMemcpyAsync(d_v.p, a.vertices, (size_t)n * 36, hipMemcpyHostToDevice, st));
    RF_OK(hipMemcpyAsync(d_n.p, a.normals, (size_t)n * 36, hipMemcpyHostToDevice, st));
    if (a.tangents) RF_OK(hipMemcpyAsync(d_t.p, a.tangents, (size_t)n * 36, hipMemcpyHostToDevice, st));
    // [0] vmax, [1..6] scene bounds (order-preserving integers), [7] lift max: the layout of the builder's counters
    unsigned g[12];
    for (int k = 0; k < 12; k++) g[k] = (k >= 1 && k <= 3) ? 0xffffffffu : 0u;
    RF_OK(hipMemcpyAsync(d_g.p, g, sizeof(g), hipMemcpyHostToDevice, st));
    const uint32_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_scene_bounds, dim3(blocks), dim3(256), 0, st, d_v.p, n, d_g.p);
    hipLaunchKernelGGL(k_prims, dim3(blocks), dim3(256), 0, st, d_v.p, d_n.p, n, d_g.p, d_box.p, d_lift.p, d_g.p + 7, d_g.p + 1);
    hipLaunchKernelGGL(k_refit_records, dim3(blocks), dim3(256), 0, st, n, d_box.p, d_lift.p, d_v.p, a.write_normals ? d_n.p : (const float*)nullptr,
                       (const float*)d_t.p, b.isect, b.attr, d_sbox.p);
    for (size_t l = topo.off2.size(); l-- > 1;) {      // deepest level first
        const uint32_t first = topo.off2[l - 1], m = topo.off2[l] - first;
        if (m) hipLaunchKernelGGL(k_refit_binary, dim3((m + 255) / 256), dim3(256), 0, st, b.nodes, b.node_count, topo.d_lv2 + first, m, d_sbox.p, n);
    }
    for (size_t l = topo.off8.size(); l-- > 1;) {
        const uint32_t first = topo.off8[l - 1], m = topo.off8[l] - first;
        if (m) hipLaunchKernelGGL(k_refit_wide, dim3((m + 255) / 256), dim3(256), 0, st, b.nodes8, b.node8_count, topo.d_lv8 + first, m, d_sbox.p, n, d_nbox.p);
    }
    RF_OK(hipGetLastError());
    RF_OK(hipEventRecord(ev.b, st));
    RF_OK(hipMemcpyAsync(g, d_g.p, sizeof(g), hipMemcpyDeviceToHost, st));
    RF_OK(hipStreamSynchronize(st));
    for (int k = 0; k < 3; k++) { out->lo[k] = er_ord2f_host(g[1 + k]); out->hi[k] = er_ord2f_host(g[4 + k]); }
    memcpy(&out->lift_bound, &g[7], 4);
    (void)hipEventElapsedTime(&out->refit_ms, ev.a, ev.b);
    return 0;
}
