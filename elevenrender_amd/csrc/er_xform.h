// er_xform.h -- object transforms (er_objects_set / er_render_transform, include/eleven_hip.h): the arithmetic that poses
// a registered object from its rest copy, stated ONCE for the device kernel (k_xform_scatter, er_refit.hip), for the host copy of the
// scene (er_objects_flush below) and for the tests (er_debug_transform_apply; elevenrender_amd/transform.py restates it in numpy).
// Plain C++ plus __host__ __device__, without a HIP or library header: tests/native/xform_host.cpp compiles it alone under ASan + UBSan.
//
// A transform is a row-major 3x4 matrix m: x' = L x + t, L = its 3x3 part, det(L) > 0 (a mirror would have to flip the records' sign,
// which no refit does).  Per object the HOST derives, in double, every product and every sum rounded by itself in the written order
// (-ffp-contract=off):
//   C = the cofactor matrix of L (= det x L^-T: what normals transform by),   N = float32(C / max|C_ij|),   T = float32(L / max|L_ij|)
// Per vertex, in float32, nothing contracted:
//   position  row i:  ((m[4i] x + m[4i+1] y) + m[4i+2] z) + m[4i+3]
//   normal    q = N n with the same association;  len = sqrtf((qx qx + qy qy) + qz qz);  n' = len > 0 ? q / len : (0, 0, 0)
//   tangent   the same with T
// Directions therefore come out unit or zero.  pose(rest, identity) reproduces the vertices bit for bit; it need NOT reproduce rest
// normals or tangents that are not of unit length (they are normalised), nor, to the last bit, those that are.
// Finite vertices are the host's business, not the kernel's: er_objects_take keeps each object's largest rest |coordinate| per axis,
// B, and er_xform_bound_ok refuses a matrix unless |m_i0| Bx + |m_i1| By + |m_i2| Bz + |m_i3| <= 1e37 in every row.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define ER_XF_HD __host__ __device__
#else
#define ER_XF_HD
#endif

// What is uploaded per listed object: 128 bytes, whatever the object's size.
struct ErXformEntry {
    uint32_t object;      // index into the object table
    uint32_t start;       // the triangles of the objects listed before this one: its first work item of k_xform_scatter
    float m[12], N[9], T[9];
};
static_assert(sizeof(ErXformEntry) == 128, "an upload entry is 128 bytes");

ER_XF_HD inline float er_xf_row(const float* r, float x, float y, float z) { return (r[0] * x + r[1] * y) + r[2] * z; }

ER_XF_HD inline void er_xform_point(const float* m, const float* p, float* out) {
    const float x = p[0], y = p[1], z = p[2];
    for (int i = 0; i < 3; i++) out[i] = er_xf_row(m + 4 * i, x, y, z) + m[4 * i + 3];
}

ER_XF_HD inline void er_xform_dir(const float* M, const float* d, float* out) {
    const float x = d[0], y = d[1], z = d[2];
    const float qx = er_xf_row(M, x, y, z), qy = er_xf_row(M + 3, x, y, z), qz = er_xf_row(M + 6, x, y, z);
    const float len = sqrtf((qx * qx + qy * qy) + qz * qz);
    const bool unit = len > 0;      // (a NaN length gives the zero vector too)
    out[0] = unit ? qx / len : 0.0f;
    out[1] = unit ? qy / len : 0.0f;
    out[2] = unit ? qz / len : 0.0f;
}

// one triangle: [3][3] rest vertices, normals, tangents -> the posed ones (the outputs must not overlap the inputs)
ER_XF_HD inline void er_xform_triangle(const float* m, const float* N, const float* T, const float* rv, const float* rn, const float* rt, float* ov, float* on, float* ot) {
    for (int j = 0; j < 3; j++) {
        er_xform_point(m, rv + 3 * j, ov + 3 * j);
        er_xform_dir(N, rn + 3 * j, on + 3 * j);
        er_xform_dir(T, rt + 3 * j, ot + 3 * j);
    }
}

// ---- host only from here on ----

// N and T of a matrix; false if an entry is not finite or det(L) is not > 0
inline bool er_xform_derive(const float* m, float* N, float* T) {
    for (int k = 0; k < 12; k++) if (!std::isfinite(m[k])) return false;
    double L[9], C[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) L[3 * i + j] = (double)m[4 * i + j];
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
    double cmax = 0, lmax = 0;
    for (int k = 0; k < 9; k++) { cmax = std::max(cmax, std::fabs(C[k])); lmax = std::max(lmax, std::fabs(L[k])); }
    if (!(cmax > 0) || !(lmax > 0)) return false;      // (cannot happen with det > 0)
    for (int k = 0; k < 9; k++) { N[k] = (float)(C[k] / cmax); T[k] = (float)(L[k] / lmax); }
    return true;
}

// the overflow bound: B = an object's largest rest |coordinate| per axis
inline bool er_xform_bound_ok(const float* m, const float* B) {
    for (int i = 0; i < 3; i++) {
        const double s = ((std::fabs((double)m[4 * i]) * (double)B[0] + std::fabs((double)m[4 * i + 1]) * (double)B[1]) + std::fabs((double)m[4 * i + 2]) * (double)B[2]) +
                         std::fabs((double)m[4 * i + 3]);
        if (!(s <= 1e37)) return false;
    }
    return true;
}

// the host form on caller arrays: count triangles, [count][3][3] each (er_debug_transform_apply); false = er_xform_derive refuses m
inline bool er_xform_apply(const float* m, uint32_t count, const float* rv, const float* rn, const float* rt, float* ov, float* on, float* ot) {
    float N[9], T[9];
    if (!er_xform_derive(m, N, T)) return false;
    for (size_t i = 0; i < (size_t)count; i++) er_xform_triangle(m, N, T, rv + i * 9, rn + i * 9, rt + i * 9, ov + i * 9, on + i * 9, ot + i * 9);
    return true;
}

// The object table of a scene: disjoint lists of triangle ids in CSR form, the REST pose of every listed triangle in CSR order (what
// er_objects_set saw), each object's bound, and the lazy half of the host copy: per object the last matrix, and whether the scene's
// host arrays still lack that pose (er_render_transform sets the two and touches no triangle).
struct ErObjectTable {
    std::vector<uint32_t> first, ids;                 // object o = ids[first[o] .. first[o + 1])
    std::vector<float> rest_v, rest_n, rest_t;        // [ids.size()][3][3]
    std::vector<float> bound;                         // [objects][3]
    std::vector<float> last_m;                        // [objects][12]
    std::vector<uint8_t> pending;                     // [objects]
    uint32_t pending_count = 0;
    uint32_t objects() const { return first.empty() ? 0u : (uint32_t)first.size() - 1u; }
    uint32_t size_of(uint32_t o) const { return first[o + 1] - first[o]; }
    void forget_pending() { std::fill(pending.begin(), pending.end(), (uint8_t)0); pending_count = 0; }      // (the arrays were replaced whole)
};

// true if (object_count, first, ids) may become the table of a scene of tri_count triangles; else `why` says what is wrong
inline bool er_objects_check(uint32_t tri_count, uint32_t object_count, const uint32_t* first, const uint32_t* ids, std::string& why) {
    if (object_count == 0) return true;      // clears the table: neither array is read
    if (!first) { why = "objects without `first`"; return false; }
    if (first[0] != 0) { why = "first[0] is not 0"; return false; }
    for (uint32_t o = 0; o < object_count; o++)
        if (first[o + 1] < first[o]) { why = "first decreases at object " + std::to_string(o); return false; }
    const uint32_t total = first[object_count];
    if (total && !ids) { why = "objects without tri_ids"; return false; }
    if (total > tri_count) { why = "more ids than triangles: an id is listed twice"; return false; }
    for (uint32_t i = 0; i < total; i++)
        if (ids[i] >= tri_count) { why = "tri_ids[" + std::to_string(i) + "] = " + std::to_string(ids[i]) + " is not below tri_count " + std::to_string(tri_count); return false; }
    std::vector<uint32_t> sorted(ids, ids + total);      // (two objects that share a triangle would be two writers of one record)
    std::sort(sorted.begin(), sorted.end());
    const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
    if (twice != sorted.end()) { why = "triangle " + std::to_string(*twice) + " is listed twice"; return false; }
    return true;
}

// a checked description into `t` (replacing what it held), the rest pose taken from the scene's [tri_count][3][3] arrays
inline void er_objects_take(ErObjectTable& t, uint32_t object_count, const uint32_t* first, const uint32_t* ids, const float* v, const float* n, const float* tg) {
    ErObjectTable x;
    if (object_count) {
        const uint32_t total = first[object_count];
        x.first.assign(first, first + object_count + 1);
        if (total) x.ids.assign(ids, ids + total);
        x.rest_v.resize((size_t)total * 9); x.rest_n.resize((size_t)total * 9); x.rest_t.resize((size_t)total * 9);
        x.bound.assign((size_t)object_count * 3, 0.0f);
        x.last_m.assign((size_t)object_count * 12, 0.0f);
        x.pending.assign(object_count, (uint8_t)0);
        for (uint32_t o = 0; o < object_count; o++) {
            float* B = &x.bound[(size_t)o * 3];
            for (uint32_t j = first[o]; j < first[o + 1]; j++) {
                const size_t from = (size_t)ids[j] * 9, to = (size_t)j * 9;
                std::copy(v + from, v + from + 9, &x.rest_v[to]);
                std::copy(n + from, n + from + 9, &x.rest_n[to]);
                std::copy(tg + from, tg + from + 9, &x.rest_t[to]);
                for (int k = 0; k < 9; k++) B[k % 3] = std::max(B[k % 3], std::fabs(v[from + k]));
            }
            for (int k = 0; k < 3; k++) x.last_m[(size_t)o * 12 + 5 * k] = 1.0f;      // the identity
        }
    }
    std::swap(t, x);
}

// The checks of er_render_transform's list, O(count) time and memory: x[i].object and x[i].m[12] (ErObjectTransform).  On success
// `entries` holds what is uploaded and `moved` the triangles of the listed objects.
template <class X>
inline bool er_xform_check(const ErObjectTable& t, uint32_t count, const X* x, std::vector<ErXformEntry>& entries, uint32_t& moved, std::string& why) {
    if (count == 0) { why = "the geometry bit with count 0"; return false; }
    if (!x) { why = "the geometry bit without transforms"; return false; }
    const uint32_t objects = t.objects();
    for (uint32_t i = 0; i < count; i++)
        if (x[i].object >= objects) { why = "transforms[" + std::to_string(i) + "].object = " + std::to_string(x[i].object) + " is not below the object count " + std::to_string(objects); return false; }
    if (count > objects) { why = "more transforms than objects: an object is listed twice"; return false; }
    std::vector<uint32_t> sorted(count);
    for (uint32_t i = 0; i < count; i++) sorted[i] = x[i].object;
    std::sort(sorted.begin(), sorted.end());
    const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
    if (twice != sorted.end()) { why = "object " + std::to_string(*twice) + " is listed twice"; return false; }
    entries.assign(count, ErXformEntry{});
    moved = 0;
    for (uint32_t i = 0; i < count; i++) {
        ErXformEntry& e = entries[i];
        e.object = x[i].object;
        e.start = moved;
        std::copy(x[i].m, x[i].m + 12, e.m);
        for (int k = 0; k < 12; k++)
            if (!std::isfinite(e.m[k])) { why = "transforms[" + std::to_string(i) + "]: a matrix entry is not finite"; return false; }
        if (!er_xform_derive(e.m, e.N, e.T)) { why = "transforms[" + std::to_string(i) + "]: det(L) is not > 0 (a mirror or a singular matrix)"; return false; }
        if (!er_xform_bound_ok(e.m, &t.bound[(size_t)e.object * 3])) { why = "transforms[" + std::to_string(i) + "]: the posed object would leave the float range (bound 1e37)"; return false; }
        moved += t.size_of(e.object);
    }
    if (moved == 0) { why = "the listed objects hold no triangle"; return false; }
    return true;
}

// what er_render_transform does to the host copy: matrix and flag, no triangle touched.  Nothing here allocates or can fail.
inline void er_objects_mark(ErObjectTable& t, const ErXformEntry* entries, uint32_t count) noexcept {
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t o = entries[i].object;
        std::copy(entries[i].m, entries[i].m + 12, &t.last_m[(size_t)o * 12]);
        if (!t.pending[o]) { t.pending[o] = 1; t.pending_count++; }
    }
}

// The pending poses into the scene's [tri_count][3][3] arrays: called wherever those arrays are read or partly overwritten.  Nothing
// here allocates or can fail (the matrices passed er_xform_check).
inline void er_objects_flush(ErObjectTable& t, float* v, float* n, float* tg) noexcept {
    if (!t.pending_count) return;
    const uint32_t objects = t.objects();
    for (uint32_t o = 0; o < objects; o++) {
        if (!t.pending[o]) continue;
        const float* m = &t.last_m[(size_t)o * 12];
        float N[9], T[9];
        if (er_xform_derive(m, N, T))
            for (uint32_t j = t.first[o]; j < t.first[o + 1]; j++) {
                const size_t from = (size_t)j * 9, to = (size_t)t.ids[j] * 9;
                er_xform_triangle(m, N, T, &t.rest_v[from], &t.rest_n[from], &t.rest_t[from], v + to, n + to, tg + to);
            }
        t.pending[o] = 0;
    }
    t.pending_count = 0;
}
