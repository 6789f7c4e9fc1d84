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
//
// The sparse refit (er_refit_sparse) gets a LIST of moved triangles and leaves the same bytes: records scattered through
// slot_of, the largest coordinate reduced over the records, and -- if its bits are those the kept boxes were padded with -- only the
// marked nodes recomputed, level by level, by the same node code; else the whole refit above from arrays gathered out of the records.
//
// The transform refit (er_refit_xform) is the sparse refit with one kernel exchanged: the listed triangles are not uploaded
// but posed by k_xform_scatter from a rest copy that lies on the device (er_xform.h has the arithmetic), which also writes the id list
// that everything behind the scatter runs over.  The skin refit (er_refit_skin) exchanges the same kernel once more:
// k_skin_scatter blends each corner's matrix from a palette (er_skin.h).  refit_listed is the one body of all three.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>
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

// ---- topology maps: the way UP from a triangle (the sparse refit) ----
__global__ __launch_bounds__(256) void k_map_slots(const ErTriIsect* __restrict__ isect, uint32_t n, uint32_t* slot_of) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const uint32_t id = (uint32_t)isect[k].tri_id;
    if (id < n) slot_of[id] = k;
}

__global__ __launch_bounds__(256) void k_map_binary(const ErNode* __restrict__ nodes, uint32_t node_count, const uint32_t* __restrict__ list, uint32_t m, uint32_t n,
                                                     uint32_t* par2, uint32_t* leaf2) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const uint32_t i = list[t];
    if (i >= node_count) return;
    const int c[2] = {nodes[i].c0, nodes[i].c1};
    for (int k = 0; k < 2; k++) {
        if (c[k] < 0) {
            const uint32_t code = (uint32_t)~c[k], first = code >> 3, cnt = (code & 7u) + 1u;
            for (uint32_t j = 0; j < cnt; j++) if (first + j < n) leaf2[first + j] = i;
        } else if (ref_inner(c[k]) && (uint32_t)c[k] < node_count && (uint32_t)c[k] != i) {
            par2[c[k]] = i;
        }
    }
}

__global__ __launch_bounds__(256) void k_map_wide(const float4* __restrict__ nodes8, uint32_t node8_count, const uint32_t* __restrict__ list, uint32_t m, uint32_t n,
                                                   uint32_t* par8, uint32_t* leaf8) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const uint32_t i = list[t];
    if (i >= node8_count) return;
    const ErNode8* nd = node8_at(nodes8, i);
    uint32_t inner_rank = 0, tri_pos = nd->tri_base;
    for (int s = 0; s < 8; s++) {
        if ((nd->imask >> s) & 1u) {
            const uint32_t c = nd->child_base + inner_rank++;
            if (c < node8_count && c > i) par8[c] = i;
        } else {
            const uint32_t cnt = ((nd->tri_present >> (2 * s)) & 1u) + ((nd->tri_present >> (2 * s + 1)) & 1u);
            for (uint32_t j = 0; j < cnt; j++) if (tri_pos + j < n) leaf8[tri_pos + j] = i;
            tri_pos += cnt;
        }
    }
}

// ---- records ----
// (nrm_all: the scene's normals whether they are written or not -- the term of the lift maximum is kept per slot for the sparse refit)
__global__ __launch_bounds__(256) void k_refit_records(uint32_t n, const Box3* __restrict__ boxes, const float* __restrict__ lift, const float* __restrict__ v,
                                                        const float* __restrict__ nrm, const float* __restrict__ tan, ErTriIsect* isect, ErTriAttr* attr,
                                                        Box3* __restrict__ sbox, const float* __restrict__ nrm_all, float* __restrict__ slift) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    float4* q = (float4*)(isect + k);
    const float4 q0 = q[0], q2 = q[2];
    const uint32_t id = (uint32_t)__float_as_int(q0.w);
    if (id >= n) {      // a record that names no triangle constrains nothing
        Box3 e;
        for (int a = 0; a < 3; a++) { e.lo[a] = INFINITY; e.hi[a] = -INFINITY; }
        sbox[k] = e;
        slift[k] = 0.0f;
        return;
    }
    const float* p = v + (size_t)id * 9;
    q[0] = make_float4(p[0], p[1], p[2], q0.w);
    q[1] = make_float4(p[3], p[4], p[5], lift[id]);
    q[2] = make_float4(p[6], p[7], p[8], q2.w);
    if (nrm) for (int j = 0; j < 3; j++) for (int a = 0; a < 3; a++) attr[k].n[j][a] = nrm[(size_t)id * 9 + 3 * j + a];
    if (tan) for (int j = 0; j < 3; j++) for (int a = 0; a < 3; a++) attr[k].t[j][a] = tan[(size_t)id * 9 + 3 * j + a];
    sbox[k] = boxes[id];
    slift[k] = prim_lift(p, nrm_all + (size_t)id * 9);
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

// ---- binary tree: one node (i < node_count), its deeper levels done ----
__device__ __forceinline__ void refit_binary_node(ErNode* nodes, uint32_t node_count, uint32_t i, const Box3* __restrict__ sbox, uint32_t n) {
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

__global__ __launch_bounds__(256) void k_refit_binary(ErNode* nodes, uint32_t node_count, const uint32_t* __restrict__ list, uint32_t m,
                                                       const Box3* __restrict__ sbox, uint32_t n) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const uint32_t i = list[t];
    if (i >= node_count) return;
    refit_binary_node(nodes, node_count, i, sbox, n);
}

// ---- wide tree: one node (i < node8_count), its deeper levels done ----
__device__ __forceinline__ void refit_wide_node(float4* nodes8, uint32_t node8_count, uint32_t i, const Box3* __restrict__ sbox, uint32_t n, Box3* nbox) {
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

__global__ __launch_bounds__(256) void k_refit_wide(float4* nodes8, uint32_t node8_count, const uint32_t* __restrict__ list, uint32_t m,
                                                     const Box3* __restrict__ sbox, uint32_t n, Box3* nbox) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const uint32_t i = list[t];
    if (i >= node8_count) return;
    refit_wide_node(nodes8, node8_count, i, sbox, n, nbox);
}

// ---- the sparse refit ----
// the listed triangles into their records, found through slot_of: one writer per record (no id is listed twice)
__global__ __launch_bounds__(256) void k_sparse_scatter(uint32_t count, const uint32_t* __restrict__ ids, const float* __restrict__ v, const float* __restrict__ nrm,
                                                         const float* __restrict__ tan, const uint32_t* __restrict__ slot_of, uint32_t n, ErTriIsect* isect,
                                                         ErTriAttr* attr) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const uint32_t id = ids[t];
    if (id >= n) return;
    const uint32_t k = slot_of[id];
    if (k >= n) return;
    float4* q = (float4*)(isect + k);
    const float* p = v + (size_t)t * 9;
    q[0] = make_float4(p[0], p[1], p[2], q[0].w);
    q[1] = make_float4(p[3], p[4], p[5], q[1].w);
    q[2] = make_float4(p[6], p[7], p[8], q[2].w);
    if (nrm) for (int j = 0; j < 3; j++) for (int a = 0; a < 3; a++) attr[k].n[j][a] = nrm[(size_t)t * 9 + 3 * j + a];
    if (tan) for (int j = 0; j < 3; j++) for (int a = 0; a < 3; a++) attr[k].t[j][a] = tan[(size_t)t * 9 + 3 * j + a];
}

// er_render_transform: the triangles of the listed objects posed from the device-resident rest copy (er_xform.h has the arithmetic) into
// their records, found through slot_of.  One work item per triangle of the listed objects; `ent` holds each listed object's first work
// item (a prefix of their sizes), so a work item finds its object by bisection over the few entries and its CSR position from `first`.
// Pure bandwidth.  Per triangle it READS seven 16-byte pieces of the rest copy (112 bytes; consecutive lanes, consecutive addresses),
// 4 bytes of slot_of and the three w words of its record (tri_id, lift, sign: kept, as k_sparse_scatter keeps them), and WRITES the
// record's 48 bytes as three 16-byte stores, n and t of the attribute record (72 bytes: four 16-byte stores and one of 8) and its id into
// ids_out (4 bytes: the list the rest of the sparse refit runs over).  Plain vector stores; one writer per record (no triangle is in
// two objects, no object is listed twice); no atomics.
__global__ __launch_bounds__(256) void k_xform_scatter(uint32_t moved, uint32_t entries, const ErXformEntry* __restrict__ ent, const uint32_t* __restrict__ first,
                                                        const float4* __restrict__ rest, uint32_t total, const uint32_t* __restrict__ slot_of, uint32_t n,
                                                        ErTriIsect* isect, ErTriAttr* attr, uint32_t* __restrict__ ids_out) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= moved) return;
    uint32_t lo = 0, hi = entries;      // the LAST entry that starts at or before t (an empty object shares its start with the next one)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ent[mid].start <= t) lo = mid; else hi = mid;
    }
    const ErXformEntry* e = ent + lo;
    const uint32_t j = first[e->object] + (t - e->start);
    ids_out[t] = 0xffffffffu;           // (names no triangle: the kernels behind this one skip it)
    if (j >= total) return;             // cannot happen with a checked list
    float r[4 * ER_XFORM_PIECES];
    for (uint32_t p = 0; p < ER_XFORM_PIECES; p++) {
        const float4 q = rest[(size_t)p * total + j];
        r[4 * p] = q.x; r[4 * p + 1] = q.y; r[4 * p + 2] = q.z; r[4 * p + 3] = q.w;
    }
    const uint32_t id = __float_as_uint(r[27]);
    if (id >= n) return;
    ids_out[t] = id;
    const uint32_t k = slot_of[id];
    if (k >= n) return;
    float m[12], N[9], T[9];
    for (int a = 0; a < 12; a++) m[a] = e->m[a];
    for (int a = 0; a < 9; a++) { N[a] = e->N[a]; T[a] = e->T[a]; }
    float v[9], o[18];
    er_xform_triangle(m, N, T, r, r + 9, r + 18, v, o, o + 9);
    float4* q = (float4*)(isect + k);
    const float* w = (const float*)q;
    q[0] = make_float4(v[0], v[1], v[2], w[3]);
    q[1] = make_float4(v[3], v[4], v[5], w[7]);
    q[2] = make_float4(v[6], v[7], v[8], w[11]);
    float4* a4 = (float4*)(attr + k);      // n[3][3] and t[3][3] lie first in the record, back to back
    for (int p = 0; p < 4; p++) a4[p] = make_float4(o[4 * p], o[4 * p + 1], o[4 * p + 2], o[4 * p + 3]);
    ((float2*)a4)[8] = make_float2(o[16], o[17]);
}

// er_render_skin: k_xform_scatter with the pose of each CORNER blended from a palette (er_skin.h has the arithmetic).  The same work
// items, the same reads of the rest copy, slot_of and the record's w words, the same stores.  New per triangle: its 72 bytes of
// influences, six pieces laid out piece-major over the rows of the skinned objects (ErSkinDev: consecutive lanes, consecutive
// addresses), and per corner up to four matrices of the listed object's palette -- 48 bytes each, the same few for every lane of the
// object, read through the cache.  A bone index is clamped to the entry's bone count (er_skin_set checked it: the clamp changes
// nothing, and no index can reach past the palette).  Plain vector stores; one writer per record; no atomics.
__global__ __launch_bounds__(256) void k_skin_scatter(uint32_t moved, uint32_t entries, const ErSkinEntry* __restrict__ ent, const uint32_t* __restrict__ first,
                                                       const float4* __restrict__ rest, uint32_t total, const float4* __restrict__ inf_w, const uint2* __restrict__ inf_b,
                                                       uint32_t rows, const float* __restrict__ palette, uint32_t bones, const uint32_t* __restrict__ slot_of, uint32_t n,
                                                       ErTriIsect* isect, ErTriAttr* attr, uint32_t* __restrict__ ids_out) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= moved) return;
    uint32_t lo = 0, hi = entries;      // the LAST entry that starts at or before t
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ent[mid].start <= t) lo = mid; else hi = mid;
    }
    const ErSkinEntry e = ent[lo];
    const uint32_t j = first[e.object] + (t - e.start), row = e.row + (t - e.start);
    ids_out[t] = 0xffffffffu;           // (names no triangle: the kernels behind this one skip it)
    if (j >= total || row >= rows || e.bones == 0 || e.pal >= bones || e.bones > bones - e.pal) return;      // cannot happen with a checked list
    float r[4 * ER_XFORM_PIECES];
    for (uint32_t p = 0; p < ER_XFORM_PIECES; p++) {
        const float4 q = rest[(size_t)p * total + j];
        r[4 * p] = q.x; r[4 * p + 1] = q.y; r[4 * p + 2] = q.z; r[4 * p + 3] = q.w;
    }
    const uint32_t id = __float_as_uint(r[27]);
    if (id >= n) return;
    ids_out[t] = id;
    const uint32_t k = slot_of[id];
    if (k >= n) return;
    const float* P = palette + (size_t)e.pal * 12;
    const uint32_t last = e.bones - 1;
    float v[9], o[18];
    for (uint32_t c = 0; c < 3; c++) {
        const float4 w4 = inf_w[(size_t)c * rows + row];
        const uint2 b2 = inf_b[(size_t)c * rows + row];
        const float w[ER_SKIN_K] = {w4.x, w4.y, w4.z, w4.w};
        const uint32_t b[ER_SKIN_K] = {min(b2.x & 0xffffu, last), min(b2.x >> 16, last), min(b2.y & 0xffffu, last), min(b2.y >> 16, last)};
        er_skin_corner(P, b, w, r + 3 * c, r + 9 + 3 * c, r + 18 + 3 * c, v + 3 * c, o + 3 * c, o + 9 + 3 * c);
    }
    float4* q = (float4*)(isect + k);
    const float* w = (const float*)q;
    q[0] = make_float4(v[0], v[1], v[2], w[3]);
    q[1] = make_float4(v[3], v[4], v[5], w[7]);
    q[2] = make_float4(v[6], v[7], v[8], w[11]);
    float4* a4 = (float4*)(attr + k);      // n[3][3] and t[3][3] lie first in the record, back to back
    for (int p = 0; p < 4; p++) a4[p] = make_float4(o[4 * p], o[4 * p + 1], o[4 * p + 2], o[4 * p + 3]);
    ((float2*)a4)[8] = make_float2(o[16], o[17]);
}

// k_scene_bounds over the records: the largest |coordinate| of what lies on the device (a maximum: the order does not matter).
// This and k_sparse_globals stride over the slots with a bounded grid (REDUCE_BLOCKS): one atomic per wave of a grid of n threads is
// 7 x n / 64 atomics on the same few words, and at 10 M triangles those, not the bytes, set the time.
__global__ __launch_bounds__(256) void k_records_vmax(const ErTriIsect* __restrict__ isect, uint32_t n, unsigned* g /* [0] vmax bits */) {
    float vm = 0;
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        const ErTriIsect r = isect[k];
        if ((uint32_t)r.tri_id < n)
            for (int a = 0; a < 3; a++) vm = fmaxf(vm, fmaxf(fabsf(r.v0[a]), fmaxf(fabsf(r.v1[a]), fabsf(r.v2[a]))));
    }
    for (int off = 32; off >= 1; off >>= 1) vm = fmaxf(vm, __shfl_xor(vm, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(&g[0], __float_as_uint(vm));
}

// path 1, per listed triangle: lift and padded box by k_prims' own arithmetic from what its record and attribute record now hold,
// and the marks on the two nodes that hold its slot
__global__ __launch_bounds__(256) void k_sparse_prims(uint32_t count, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ slot_of, uint32_t n,
                                                       ErTriIsect* isect, const ErTriAttr* __restrict__ attr, const unsigned* __restrict__ g, Box3* sbox, float* slift,
                                                       const uint32_t* __restrict__ leaf2, uint32_t* mark2, uint32_t node_count,
                                                       const uint32_t* __restrict__ leaf8, uint32_t* mark8, uint32_t node8_count, uint32_t epoch) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const uint32_t id = ids[t];
    if (id >= n) return;
    const uint32_t k = slot_of[id];
    if (k >= n) return;
    const ErTriIsect r = isect[k];
    float p[9], nn[9];
    for (int a = 0; a < 3; a++) { p[a] = r.v0[a]; p[3 + a] = r.v1[a]; p[6 + a] = r.v2[a]; }
    for (int j = 0; j < 3; j++) for (int a = 0; a < 3; a++) nn[3 * j + a] = attr[k].n[j][a];
    Box3 b;
    prim_padded_box(p, __uint_as_float(g[0]) * 1e-6f, &b);
    const float raw = prim_lift(p, nn);
    sbox[k] = b;
    slift[k] = raw;
    isect[k].lift = raw + 1e-30f;
    const uint32_t l2 = leaf2[k], l8 = leaf8[k];
    if (l2 < node_count) mark2[l2] = epoch;
    if (l8 < node8_count) mark8[l8] = epoch;
}

// path 1: the scene bounds and the lift maximum from the kept per-slot values, as k_prims reduces them
__global__ __launch_bounds__(256) void k_sparse_globals(uint32_t n, const Box3* __restrict__ sbox, const float* __restrict__ slift, unsigned* g) {
    float my_lift = 0;
    float slo[3] = {INFINITY, INFINITY, INFINITY}, shi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        const Box3 b = sbox[k];
        for (int a = 0; a < 3; a++) { slo[a] = fminf(slo[a], b.lo[a]); shi[a] = fmaxf(shi[a], b.hi[a]); }
        my_lift = fmaxf(my_lift, slift[k]);
    }
    for (int off = 32; off >= 1; off >>= 1) my_lift = fmaxf(my_lift, __shfl_xor(my_lift, off, 64));
    for (int off = 32; off >= 1; off >>= 1)
        for (int a = 0; a < 3; a++) { slo[a] = fminf(slo[a], __shfl_xor(slo[a], off, 64)); shi[a] = fmaxf(shi[a], __shfl_xor(shi[a], off, 64)); }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&g[7], __float_as_uint(my_lift));
        for (int a = 0; a < 3; a++) { atomicMin(&g[1 + a], f2ord(slo[a])); atomicMax(&g[4 + a], f2ord(shi[a])); }
    }
}

// path 1, one level: a node that no deeper launch (or k_sparse_prims) marked returns after one flag read; a marked one is recomputed by
// the full refit's own code and marks its parent, which a LATER launch reads.  g[8], g[9]: the nodes rewritten.
__global__ __launch_bounds__(256) void k_dirty_binary(ErNode* nodes, uint32_t node_count, const uint32_t* __restrict__ list, uint32_t m, const Box3* __restrict__ sbox,
                                                       uint32_t n, uint32_t* mark2, const uint32_t* __restrict__ par2, uint32_t epoch, unsigned* g) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const uint32_t i = list[t];
    if (i >= node_count || mark2[i] != epoch) return;
    refit_binary_node(nodes, node_count, i, sbox, n);
    const uint32_t up = par2[i];
    if (up < node_count) mark2[up] = epoch;
    atomicAdd(&g[8], 1u);
}

__global__ __launch_bounds__(256) void k_dirty_wide(float4* nodes8, uint32_t node8_count, const uint32_t* __restrict__ list, uint32_t m, const Box3* __restrict__ sbox,
                                                     uint32_t n, Box3* nbox, uint32_t* mark8, const uint32_t* __restrict__ par8, uint32_t epoch, unsigned* g) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const uint32_t i = list[t];
    if (i >= node8_count || mark8[i] != epoch) return;
    refit_wide_node(nodes8, node8_count, i, sbox, n, nbox);
    const uint32_t up = par8[i];
    if (up < node8_count) mark8[up] = epoch;
    atomicAdd(&g[9], 1u);
}

// path 2: triangle-ordered vertices and normals out of the records, for the full refit's kernels
__global__ __launch_bounds__(256) void k_gather_arrays(uint32_t n, const ErTriIsect* __restrict__ isect, const ErTriAttr* __restrict__ attr, float* v, float* nrm) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const ErTriIsect r = isect[k];
    const uint32_t id = (uint32_t)r.tri_id;
    if (id >= n) return;
    float* p = v + (size_t)id * 9;
    for (int a = 0; a < 3; a++) { p[a] = r.v0[a]; p[3 + a] = r.v1[a]; p[6 + a] = r.v2[a]; }
    for (int j = 0; j < 3; j++) for (int a = 0; a < 3; a++) nrm[(size_t)id * 9 + 3 * j + a] = attr[k].n[j][a];
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

// the maps of the sparse refit and the storage of the kept boxes, once the level lists exist
int derive_maps(ErRefitTopo& topo, const ErRefitBuffers& b, hipStream_t st, std::string& err) {
    const size_t n = b.tri_count, n2 = std::max<size_t>(1, b.node_count), n8 = std::max<size_t>(1, b.node8_count);
    RF_OK(hipMalloc((void**)&topo.d_slot_of, n * 4));
    RF_OK(hipMalloc((void**)&topo.d_leaf2, n * 4));
    RF_OK(hipMalloc((void**)&topo.d_leaf8, n * 4));
    RF_OK(hipMalloc((void**)&topo.d_par2, n2 * 4));
    RF_OK(hipMalloc((void**)&topo.d_mark2, n2 * 4));
    RF_OK(hipMalloc((void**)&topo.d_par8, n8 * 4));
    RF_OK(hipMalloc((void**)&topo.d_mark8, n8 * 4));
    RF_OK(hipMalloc((void**)&topo.d_sbox, n * sizeof(Box3)));
    RF_OK(hipMalloc((void**)&topo.d_slift, n * 4));
    RF_OK(hipMalloc((void**)&topo.d_nbox, n8 * sizeof(Box3)));
    RF_OK(hipMemsetAsync(topo.d_slot_of, 0xff, n * 4, st));
    RF_OK(hipMemsetAsync(topo.d_leaf2, 0xff, n * 4, st));
    RF_OK(hipMemsetAsync(topo.d_leaf8, 0xff, n * 4, st));
    RF_OK(hipMemsetAsync(topo.d_par2, 0xff, n2 * 4, st));
    RF_OK(hipMemsetAsync(topo.d_par8, 0xff, n8 * 4, st));
    RF_OK(hipMemsetAsync(topo.d_mark2, 0, n2 * 4, st));
    RF_OK(hipMemsetAsync(topo.d_mark8, 0, n8 * 4, st));
    hipLaunchKernelGGL(k_map_slots, dim3(((uint32_t)n + 255) / 256), dim3(256), 0, st, b.isect, b.tri_count, topo.d_slot_of);
    const uint32_t m2 = topo.off2.empty() ? 0u : topo.off2.back(), m8 = topo.off8.empty() ? 0u : topo.off8.back();
    if (m2) hipLaunchKernelGGL(k_map_binary, dim3((m2 + 255) / 256), dim3(256), 0, st, b.nodes, b.node_count, topo.d_lv2, m2, b.tri_count, topo.d_par2, topo.d_leaf2);
    if (m8) hipLaunchKernelGGL(k_map_wide, dim3((m8 + 255) / 256), dim3(256), 0, st, b.nodes8, b.node8_count, topo.d_lv8, m8, b.tri_count, topo.d_par8, topo.d_leaf8);
    RF_OK(hipGetLastError());
    RF_OK(hipStreamSynchronize(st));
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
    const int rc = derive_maps(topo, b, st, err);
    if (rc != 0) { topo.release(); return rc; }
    topo.valid = true;
    return 0;
}

// [0] vmax, [1..6] scene bounds (order-preserving integers), [7] lift max: the layout of the builder's counters; [8], [9] the sparse
// refit's counts of rewritten nodes
constexpr int G_WORDS = 16;
constexpr uint32_t REDUCE_BLOCKS = 2048;      // grid bound of the strided reductions: eight workgroups for each of the 256 CUs
void globals_init(unsigned* g) {
    for (int k = 0; k < G_WORDS; k++) g[k] = (k >= 1 && k <= 3) ? 0xffffffffu : 0u;
}

// The whole refit from triangle-ordered arrays ON THE DEVICE (d_t: NULL = keep; normals are written only if write_normals), d_g
// initialised: bounds, records, both trees level by level.  Fills the kept boxes of `topo`.  Launches only.
int refit_full_launch(ErRefitTopo& topo, const ErRefitBuffers& b, const float* d_v, const float* d_n, const float* d_t, bool write_normals, unsigned* d_g,
                      Box3* d_box, float* d_lift, hipStream_t st, std::string& err) {
    const uint32_t n = b.tri_count, blocks = (n + 255) / 256;
    Box3 *sbox = (Box3*)topo.d_sbox, *nbox = (Box3*)topo.d_nbox;
    hipLaunchKernelGGL(k_scene_bounds, dim3(blocks), dim3(256), 0, st, d_v, n, d_g);
    hipLaunchKernelGGL(k_prims, dim3(blocks), dim3(256), 0, st, d_v, d_n, n, d_g, d_box, d_lift, d_g + 7, d_g + 1);
    hipLaunchKernelGGL(k_refit_records, dim3(blocks), dim3(256), 0, st, n, d_box, d_lift, d_v, write_normals ? d_n : (const float*)nullptr, d_t, b.isect, b.attr, sbox,
                       d_n, topo.d_slift);
    for (size_t l = topo.off2.size(); l-- > 1;) {      // deepest level first
        const uint32_t first = topo.off2[l - 1], m = topo.off2[l] - first;
        if (m) hipLaunchKernelGGL(k_refit_binary, dim3((m + 255) / 256), dim3(256), 0, st, b.nodes, b.node_count, topo.d_lv2 + first, m, sbox, n);
    }
    for (size_t l = topo.off8.size(); l-- > 1;) {
        const uint32_t first = topo.off8[l - 1], m = topo.off8[l] - first;
        if (m) hipLaunchKernelGGL(k_refit_wide, dim3((m + 255) / 256), dim3(256), 0, st, b.nodes8, b.node8_count, topo.d_lv8 + first, m, sbox, n, nbox);
    }
    RF_OK(hipGetLastError());
    return 0;
}

void result_of_globals(const unsigned* g, ErRefitResult* out) {
    for (int k = 0; k < 3; k++) { out->lo[k] = er_ord2f_host(g[1 + k]); out->hi[k] = er_ord2f_host(g[4 + k]); }
    memcpy(&out->lift_bound, &g[7], 4);
}

}  // namespace

hipError_t er_probe_refit(const char** which) {
    hipFuncAttributes at;
    *which = "k_refit_wide (er_refit.hip)";
    return hipFuncGetAttributes(&at, (const void*)k_refit_wide);
}

hipError_t er_probe_refit_sparse(const char** which) {
    hipFuncAttributes at;
    *which = "k_dirty_wide (er_refit.hip)";
    return hipFuncGetAttributes(&at, (const void*)k_dirty_wide);
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
    Tmp<Box3> d_box;
    Tmp<unsigned> d_g;
    RF_OK(hipMalloc((void**)&d_v.p, (size_t)n * 36));
    RF_OK(hipMalloc((void**)&d_n.p, (size_t)n * 36));
    if (a.tangents) RF_OK(hipMalloc((void**)&d_t.p, (size_t)n * 36));
    RF_OK(hipMalloc((void**)&d_lift.p, (size_t)n * 4));
    RF_OK(hipMalloc((void**)&d_box.p, (size_t)n * sizeof(Box3)));
    RF_OK(hipMalloc((void**)&d_g.p, G_WORDS * 4));
    topo.boxes_valid = false;      // (until the last level has run)
    RF_OK(hipEventRecord(ev.a, st));
    RF_OK(hipMemcpyAsync(d_v.p, a.vertices, (size_t)n * 36, hipMemcpyHostToDevice, st));
    RF_OK(hipMemcpyAsync(d_n.p, a.normals, (size_t)n * 36, hipMemcpyHostToDevice, st));
    if (a.tangents) RF_OK(hipMemcpyAsync(d_t.p, a.tangents, (size_t)n * 36, hipMemcpyHostToDevice, st));
    unsigned g[G_WORDS];
    globals_init(g);
    RF_OK(hipMemcpyAsync(d_g.p, g, sizeof(g), hipMemcpyHostToDevice, st));
    int rc = refit_full_launch(topo, b, d_v.p, d_n.p, d_t.p, a.write_normals, d_g.p, d_box.p, d_lift.p, st, err);
    if (rc != 0) return rc;
    RF_OK(hipEventRecord(ev.b, st));
    RF_OK(hipMemcpyAsync(g, d_g.p, sizeof(g), hipMemcpyDeviceToHost, st));
    RF_OK(hipStreamSynchronize(st));
    result_of_globals(g, out);
    topo.vmax_bits = g[0];
    topo.boxes_valid = true;
    (void)hipEventElapsedTime(&out->refit_ms, ev.a, ev.b);
    return 0;
}

namespace {

static_assert(offsetof(ErTriAttr, n) == 0 && offsetof(ErTriAttr, t) == 36, "k_xform_scatter writes n and t as the record's first 18 floats");

// How the listed triangles of a sparse refit reach their records.  Either form allocates, enqueues its uploads, and scatters; what it
// leaves is the device list of the triangles' ids that the rest of refit_listed runs over, and the bytes it uploaded.
struct HostListed {      // er_render_update_sparse: ids and arrays come from the host and go through k_sparse_scatter
    const ErSparseList& a;
    uint32_t count;
    Tmp<uint32_t> d_ids;
    Tmp<float> d_v, d_n, d_t;
    explicit HostListed(const ErSparseList& l) : a(l), count(l.count) {}
    size_t list_bytes() const { return (size_t)count * 36; }
    const uint32_t* ids() const { return d_ids.p; }
    int allocate(std::string& err) {
        RF_OK(hipMalloc((void**)&d_ids.p, (size_t)count * 4));
        RF_OK(hipMalloc((void**)&d_v.p, list_bytes()));
        if (a.normals) RF_OK(hipMalloc((void**)&d_n.p, list_bytes()));
        if (a.tangents) RF_OK(hipMalloc((void**)&d_t.p, list_bytes()));
        return 0;
    }
    int upload(hipStream_t st, uint64_t* bytes, std::string& err) {
        RF_OK(hipMemcpyAsync(d_ids.p, a.tri_ids, (size_t)count * 4, hipMemcpyHostToDevice, st));
        RF_OK(hipMemcpyAsync(d_v.p, a.vertices, list_bytes(), hipMemcpyHostToDevice, st));
        if (a.normals) RF_OK(hipMemcpyAsync(d_n.p, a.normals, list_bytes(), hipMemcpyHostToDevice, st));
        if (a.tangents) RF_OK(hipMemcpyAsync(d_t.p, a.tangents, list_bytes(), hipMemcpyHostToDevice, st));
        *bytes = (uint64_t)count * 4 + list_bytes() * (1 + (a.normals ? 1 : 0) + (a.tangents ? 1 : 0));
        return 0;
    }
    void scatter(const ErRefitTopo& topo, const ErRefitBuffers& b, hipStream_t st) {
        hipLaunchKernelGGL(k_sparse_scatter, dim3((count + 255) / 256), dim3(256), 0, st, count, d_ids.p, d_v.p, (const float*)d_n.p, (const float*)d_t.p, topo.d_slot_of,
                           b.tri_count, b.isect, b.attr);
    }
};

struct DeviceListed {    // er_render_transform: the rest copy lies on the device; the entries go up and k_xform_scatter poses and scatters
    const ErXformCall& x;
    uint32_t count;
    Tmp<uint32_t> d_ids;
    Tmp<ErXformEntry> d_ent;
    explicit DeviceListed(const ErXformCall& c) : x(c), count(c.moved) {}
    const uint32_t* ids() const { return d_ids.p; }
    int allocate(std::string& err) {
        RF_OK(hipMalloc((void**)&d_ids.p, (size_t)count * 4));
        RF_OK(hipMalloc((void**)&d_ent.p, (size_t)x.entries * sizeof(ErXformEntry)));
        return 0;
    }
    int upload(hipStream_t st, uint64_t* bytes, std::string& err) {
        RF_OK(hipMemcpyAsync(d_ent.p, x.list, (size_t)x.entries * sizeof(ErXformEntry), hipMemcpyHostToDevice, st));
        *bytes = (uint64_t)x.entries * sizeof(ErXformEntry);
        return 0;
    }
    void scatter(const ErRefitTopo& topo, const ErRefitBuffers& b, hipStream_t st) {
        hipLaunchKernelGGL(k_xform_scatter, dim3((count + 255) / 256), dim3(256), 0, st, count, x.entries, (const ErXformEntry*)d_ent.p, (const uint32_t*)x.table->d_first,
                           (const float4*)x.table->d_rest, x.table->total, topo.d_slot_of, b.tri_count, b.isect, b.attr, d_ids.p);
    }
};

struct SkinListed {      // er_render_skin: rest copy and influences lie on the device; entries and palettes go up and k_skin_scatter poses and scatters
    const ErSkinCall& x;
    uint32_t count;
    Tmp<uint32_t> d_ids;
    Tmp<ErSkinEntry> d_ent;
    Tmp<float> d_pal;
    explicit SkinListed(const ErSkinCall& c) : x(c), count(c.moved) {}
    const uint32_t* ids() const { return d_ids.p; }
    int allocate(std::string& err) {
        RF_OK(hipMalloc((void**)&d_ids.p, (size_t)count * 4));
        RF_OK(hipMalloc((void**)&d_ent.p, (size_t)x.entries * sizeof(ErSkinEntry)));
        RF_OK(hipMalloc((void**)&d_pal.p, (size_t)x.bones * 48));
        return 0;
    }
    int upload(hipStream_t st, uint64_t* bytes, std::string& err) {
        RF_OK(hipMemcpyAsync(d_ent.p, x.list, (size_t)x.entries * sizeof(ErSkinEntry), hipMemcpyHostToDevice, st));
        RF_OK(hipMemcpyAsync(d_pal.p, x.palette, (size_t)x.bones * 48, hipMemcpyHostToDevice, st));
        *bytes = (uint64_t)x.entries * sizeof(ErSkinEntry) + (uint64_t)x.bones * 48;
        return 0;
    }
    void scatter(const ErRefitTopo& topo, const ErRefitBuffers& b, hipStream_t st) {
        hipLaunchKernelGGL(k_skin_scatter, dim3((count + 255) / 256), dim3(256), 0, st, count, x.entries, (const ErSkinEntry*)d_ent.p, (const uint32_t*)x.table->d_first,
                           (const float4*)x.table->d_rest, x.table->total, (const float4*)x.skin->d_w, (const uint2*)x.skin->d_b, x.skin->rows, (const float*)d_pal.p, x.bones,
                           topo.d_slot_of, b.tri_count, b.isect, b.attr, d_ids.p);
    }
};

// The sparse refit over `L`'s triangles (its arguments checked by the caller): er_refit_sparse, er_refit_xform and er_refit_skin
template <class Listed>
int refit_listed(ErRefitTopo& topo, const ErRefitBuffers& b, Listed& L, hipStream_t st, ErSparseResult* out, std::string& err) {
    const uint32_t n = b.tri_count, count = L.count;
    if (!topo.valid) {
        int rc = derive_topology(topo, b, st, err);
        if (rc != 0) return rc;
    }
    Events ev;
    RF_OK(hipEventCreate(&ev.a));
    RF_OK(hipEventCreate(&ev.b));
    Tmp<unsigned> d_g;
    int lrc = L.allocate(err);
    if (lrc != 0) return lrc;
    RF_OK(hipMalloc((void**)&d_g.p, G_WORDS * 4));
    const bool had_boxes = topo.boxes_valid;
    topo.boxes_valid = false;      // (until the last level has run)
    RF_OK(hipEventRecord(ev.a, st));
    uint64_t list_uploaded = 0;
    if ((lrc = L.upload(st, &list_uploaded, err)) != 0) return lrc;
    unsigned g[G_WORDS];
    globals_init(g);
    RF_OK(hipMemcpyAsync(d_g.p, g, sizeof(g), hipMemcpyHostToDevice, st));
    out->bytes_uploaded = list_uploaded + sizeof(g);
    const uint32_t blocks = (n + 255) / 256, lblocks = (count + 255) / 256;
    L.scatter(topo, b, st);
    const uint32_t rblocks = std::min(blocks, REDUCE_BLOCKS);
    hipLaunchKernelGGL(k_records_vmax, dim3(rblocks), dim3(256), 0, st, b.isect, n, d_g.p);
    RF_OK(hipGetLastError());
    unsigned vmax = 0;
    RF_OK(hipMemcpyAsync(&vmax, d_g.p, 4, hipMemcpyDeviceToHost, st));
    RF_OK(hipStreamSynchronize(st));
    const uint32_t* d_ids = L.ids();
    // The largest |coordinate| sets the absolute padding of EVERY box: only under the bits the kept boxes were padded with do the
    // boxes of the triangles that did not move still hold.
    out->why_full = !had_boxes ? 1u : vmax != topo.vmax_bits ? 2u : 0u;
    Tmp<float> d_av, d_an, d_lift;      // path 2's temporaries
    Tmp<Box3> d_box;
    if (out->why_full) {
        out->path = 2;
        RF_OK(hipMalloc((void**)&d_av.p, (size_t)n * 36));
        RF_OK(hipMalloc((void**)&d_an.p, (size_t)n * 36));
        RF_OK(hipMalloc((void**)&d_lift.p, (size_t)n * 4));
        RF_OK(hipMalloc((void**)&d_box.p, (size_t)n * sizeof(Box3)));
        RF_OK(hipMemsetAsync(d_av.p, 0, (size_t)n * 36, st));      // (a triangle id that no record names: cannot happen in a structure that checks clean)
        RF_OK(hipMemsetAsync(d_an.p, 0, (size_t)n * 36, st));
        RF_OK(hipMemcpyAsync(d_g.p, g, sizeof(g), hipMemcpyHostToDevice, st));      // k_scene_bounds finds the maximum again, from the gathered array
        out->bytes_uploaded += sizeof(g);
        hipLaunchKernelGGL(k_gather_arrays, dim3(blocks), dim3(256), 0, st, n, b.isect, b.attr, d_av.p, d_an.p);
        // (the records already hold the listed normals and tangents: nothing but vertices, lifts and boxes is written)
        int rc = refit_full_launch(topo, b, d_av.p, d_an.p, nullptr, false, d_g.p, d_box.p, d_lift.p, st, err);
        if (rc != 0) return rc;
        out->dirty_nodes2 = b.node_count;
        out->dirty_nodes8 = b.node8_count;
    } else {
        out->path = 1;
        if (++topo.epoch == 0) {      // the epoch wrapped: marks of 2^32 calls ago would read as this call's
            RF_OK(hipMemsetAsync(topo.d_mark2, 0, std::max<size_t>(1, b.node_count) * 4, st));
            RF_OK(hipMemsetAsync(topo.d_mark8, 0, std::max<size_t>(1, b.node8_count) * 4, st));
            topo.epoch = 1;
        }
        Box3 *sbox = (Box3*)topo.d_sbox, *nbox = (Box3*)topo.d_nbox;
        hipLaunchKernelGGL(k_sparse_prims, dim3(lblocks), dim3(256), 0, st, count, d_ids, topo.d_slot_of, n, b.isect, b.attr, d_g.p, sbox, topo.d_slift, topo.d_leaf2,
                           topo.d_mark2, b.node_count, topo.d_leaf8, topo.d_mark8, b.node8_count, topo.epoch);
        hipLaunchKernelGGL(k_sparse_globals, dim3(rblocks), dim3(256), 0, st, n, sbox, topo.d_slift, d_g.p);
        for (size_t l = topo.off2.size(); l-- > 1;) {      // deepest level first
            const uint32_t first = topo.off2[l - 1], m = topo.off2[l] - first;
            if (m) hipLaunchKernelGGL(k_dirty_binary, dim3((m + 255) / 256), dim3(256), 0, st, b.nodes, b.node_count, topo.d_lv2 + first, m, sbox, n, topo.d_mark2,
                                      topo.d_par2, topo.epoch, d_g.p);
        }
        for (size_t l = topo.off8.size(); l-- > 1;) {
            const uint32_t first = topo.off8[l - 1], m = topo.off8[l] - first;
            if (m) hipLaunchKernelGGL(k_dirty_wide, dim3((m + 255) / 256), dim3(256), 0, st, b.nodes8, b.node8_count, topo.d_lv8 + first, m, sbox, n, nbox, topo.d_mark8,
                                      topo.d_par8, topo.epoch, d_g.p);
        }
        RF_OK(hipGetLastError());
    }
    RF_OK(hipEventRecord(ev.b, st));
    RF_OK(hipMemcpyAsync(g, d_g.p, sizeof(g), hipMemcpyDeviceToHost, st));
    RF_OK(hipStreamSynchronize(st));
    result_of_globals(g, &out->refit);
    if (out->path == 1) { out->dirty_nodes2 = g[8]; out->dirty_nodes8 = g[9]; }
    topo.vmax_bits = g[0];
    topo.boxes_valid = true;
    (void)hipEventElapsedTime(&out->refit.refit_ms, ev.a, ev.b);
    return 0;
}

}  // namespace

hipError_t er_probe_xform(const char** which) {
    hipFuncAttributes at;
    *which = "k_xform_scatter (er_refit.hip)";
    return hipFuncGetAttributes(&at, (const void*)k_xform_scatter);
}

int er_refit_sparse(ErRefitTopo& topo, const ErRefitBuffers& b, const ErSparseList& a, hipStream_t st, ErSparseResult* out, std::string& err) {
    *out = ErSparseResult{};
    if (b.tri_count == 0 || a.count == 0 || !a.tri_ids || !a.vertices || !b.isect || !b.attr || !b.nodes8) { err = "sparse refit: missing array"; return -1; }
    HostListed L(a);
    return refit_listed(topo, b, L, st, out, err);
}

int er_refit_xform(ErRefitTopo& topo, const ErRefitBuffers& b, const ErXformCall& x, hipStream_t st, ErSparseResult* out, std::string& err) {
    *out = ErSparseResult{};
    if (b.tri_count == 0 || x.moved == 0 || x.entries == 0 || !x.list || !x.table || !x.table->valid || !x.table->d_rest || !x.table->d_first || x.moved > x.table->total ||
        !b.isect || !b.attr || !b.nodes8) { err = "transform refit: missing array"; return -1; }
    DeviceListed L(x);
    return refit_listed(topo, b, L, st, out, err);
}

hipError_t er_probe_skin(const char** which) {
    hipFuncAttributes at;
    *which = "k_skin_scatter (er_refit.hip)";
    return hipFuncGetAttributes(&at, (const void*)k_skin_scatter);
}

int er_refit_skin(ErRefitTopo& topo, const ErRefitBuffers& b, const ErSkinCall& x, hipStream_t st, ErSparseResult* out, std::string& err) {
    *out = ErSparseResult{};
    if (b.tri_count == 0 || x.moved == 0 || x.entries == 0 || x.bones == 0 || !x.list || !x.palette || !x.table || !x.table->valid || !x.table->d_rest || !x.table->d_first ||
        x.moved > x.table->total || !x.skin || !x.skin->valid || !x.skin->d_w || !x.skin->d_b || x.moved > x.skin->rows || !b.isect || !b.attr || !b.nodes8) {
        err = "skin refit: missing array";
        return -1;
    }
    SkinListed L(x);
    return refit_listed(topo, b, L, st, out, err);
}

int er_skin_table_build(ErSkinDev& dev, const ErObjectTable& t, const ErSkinTable& k, hipStream_t st, uint64_t* bytes, std::string& err) {
    dev.release();
    *bytes = 0;
    const uint32_t rows = k.rows(), objects = t.objects();
    if (!rows || k.rec.size() != objects) { err = "skin: no object has a skin"; return -1; }
    std::vector<float> w;
    std::vector<uint16_t> bn;
    try {
        w.resize((size_t)rows * 3 * ER_SKIN_K);
        bn.resize((size_t)rows * 3 * ER_SKIN_K);
    } catch (const std::bad_alloc&) {      // (as a failed device allocation: the caller ends the render, the host copy is already marked)
        err = "skin: out of host memory for the influences' staging";
        return -2;
    }
    for (uint32_t o = 0; o < objects; o++) {
        if (!k.has(o)) continue;
        const ErSkinRecord& r = k.rec[o];
        const uint32_t size = t.size_of(o);
        for (uint32_t i = 0; i < size; i++)
            for (uint32_t c = 0; c < 3; c++) {
                const size_t from = ((size_t)i * 3 + c) * ER_SKIN_K, to = ((size_t)c * rows + k.row_first[o] + i) * ER_SKIN_K;
                memcpy(&w[to], &r.weights[from], ER_SKIN_K * 4);
                memcpy(&bn[to], &r.bones[from], ER_SKIN_K * 2);
            }
    }
    RF_OK(hipMalloc((void**)&dev.d_w, w.size() * 4));
    RF_OK(hipMalloc((void**)&dev.d_b, bn.size() * 2));
    hipError_t e = hipMemcpyAsync(dev.d_w, w.data(), w.size() * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dev.d_b, bn.data(), bn.size() * 2, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);      // (the staging goes out of scope)
    if (e != hipSuccess) { dev.release(); RF_OK(e); }
    dev.rows = rows;
    dev.valid = true;
    *bytes = (uint64_t)rows * 72;
    return 0;
}

int er_xform_table_build(ErXformDev& dev, const ErObjectTable& t, hipStream_t st, std::string& err) {
    dev.release();
    const uint32_t total = (uint32_t)t.ids.size(), objects = t.objects();
    if (!total || !objects) { err = "transform: the object table holds no triangle"; return -1; }
    std::vector<float> pieces;
    try {
        pieces.resize((size_t)total * 4 * ER_XFORM_PIECES);
    } catch (const std::bad_alloc&) {      // (as a failed device allocation: the caller ends the render, the host copy is already marked)
        err = "transform: out of host memory for the rest copy's staging";
        return -2;
    }
    for (uint32_t j = 0; j < total; j++) {
        float r[4 * ER_XFORM_PIECES];
        memcpy(r, &t.rest_v[(size_t)j * 9], 36);
        memcpy(r + 9, &t.rest_n[(size_t)j * 9], 36);
        memcpy(r + 18, &t.rest_t[(size_t)j * 9], 36);
        memcpy(r + 27, &t.ids[j], 4);
        for (uint32_t p = 0; p < ER_XFORM_PIECES; p++) memcpy(&pieces[((size_t)p * total + j) * 4], r + 4 * p, 16);
    }
    RF_OK(hipMalloc((void**)&dev.d_rest, pieces.size() * 4));
    RF_OK(hipMalloc((void**)&dev.d_first, ((size_t)objects + 1) * 4));
    hipError_t e = hipMemcpyAsync(dev.d_rest, pieces.data(), pieces.size() * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dev.d_first, t.first.data(), ((size_t)objects + 1) * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);      // (`pieces` goes out of scope)
    if (e != hipSuccess) { dev.release(); RF_OK(e); }
    dev.total = total;
    dev.objects = objects;
    dev.valid = true;
    return 0;
}
