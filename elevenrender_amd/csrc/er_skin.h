// er_skin.h -- linear-blend skinning of registered objects (er_skin_set / er_render_skin, include/eleven_hip.h): the
// arithmetic that deforms an object from its rest copy and a palette of bone matrices, stated ONCE for the device kernel (k_skin_scatter,
// er_refit.hip), for the host copy of the scene (er_skin_flush below) and for the tests (er_debug_skin_apply; elevenrender_amd/skin.py
// restates it in numpy).  Plain C++ plus __host__ __device__, without a HIP or library header (er_xform.h, which it builds on, is plain
// too): tests/native/skin_host.cpp compiles it alone under ASan + UBSan.
//
// Geometry is a triangle soup, so influences are per CORNER: ER_SKIN_K = 4 pairs (bone index, weight) for each of a triangle's three
// corners, in the order of the object's rows of the rest copy (the CSR order of er_objects_set).  A corner with rest position x, normal
// n, tangent t, bones b0..b3, weights w0..w3 and a palette of row-major 3x4 matrices P[b] becomes, in float32, every product and every
// sum rounded by itself in the written order (-ffp-contract=off):
//   M[a] = ((w0 P[b0][a] + w1 P[b1][a]) + w2 P[b2][a]) + w3 P[b3][a]     a = 0..11, the blended matrix
//   x'   = er_xform_point(M, x)
//   n'   = er_xform_dir(C, n)     C = the cofactor matrix of M's 3x3 part, the nine formulas of er_xform_derive in that order, in float32
//   t'   = er_xform_dir(L, t)     L = M's 3x3 part as nine contiguous floats
// er_xform_dir normalises at the end, so no per-bone scaling is needed, and directions come out unit or zero.  A palette of identities
// with a single weight of exactly 1 per corner reproduces the rest vertices bit for bit (1 x = x, 0 x = 0, x + 0 = x).  Weights are used
// AS GIVEN: they are not renormalised, and a corner whose weights sum to s is posed by s times the blend of its bones.
//
// What keeps every intermediate finite, for weights in [0, 1]: er_skin_pose_check refuses a bone unless (a) it passes er_xform_bound_ok
// against the object's bound B -- each w_k P[b_k] row then stays within 1e37 of the origin and their sum within 4e37 < FLT_MAX -- and (b)
// every entry of its 3x3 part has |L_ij| <= ER_SKIN_MAX_LINEAR = 2^14:
//   |M_ij| <= 4 x 2^14 = 2^16;  a cofactor product <= 2^32, a cofactor <= 2^33;  a row of C n <= 3 x 2^33 |n| < 2^35 |n|;  its squared
//   length <= 3 x 2^70 |n|^2, finite for rest directions up to 2^27 long.
// (A blend of matrices with det > 0 each may still be singular: the corner's normal is then the zero vector, as for a zero rest normal.
// Cofactors of very small scales may underflow to the same end.  Neither is refused.)
#pragma once
#include "er_xform.h"

constexpr int ER_SKIN_K = 4;                          // ER_SKIN_INFLUENCES
constexpr uint32_t ER_SKIN_BONES_MAX = 1024u;         // ER_SKIN_MAX_BONES
constexpr float ER_SKIN_MAX_LINEAR = 16384.0f;        // 2^14: the derivation above

// What is uploaded per listed object: 32 bytes, whatever the object's size; its palette follows in a second array at 48 bytes per bone.
struct ErSkinEntry {
    uint32_t object;      // index into the object table
    uint32_t start;       // the triangles of the objects listed before this one: its first work item of k_skin_scatter
    uint32_t row;         // the object's first row in the device's influence store (skinned objects only, in object order)
    uint32_t pal;         // its first bone in the call's palette array
    uint32_t bones;       // its bone count
    uint32_t reserved[3];
};
static_assert(sizeof(ErSkinEntry) == 32, "an upload entry is 32 bytes");

// the blended matrix of one corner: P = the object's palette, b = four bone indices, w = four weights
ER_XF_HD inline void er_skin_blend(const float* P, const uint32_t* b, const float* w, float* M) {
    const float *p0 = P + 12 * (size_t)b[0], *p1 = P + 12 * (size_t)b[1], *p2 = P + 12 * (size_t)b[2], *p3 = P + 12 * (size_t)b[3];
    for (int a = 0; a < 12; a++) M[a] = ((w[0] * p0[a] + w[1] * p1[a]) + w[2] * p2[a]) + w[3] * p3[a];
}

// L = the 3x3 part of M, C = its cofactor matrix, in float32
ER_XF_HD inline void er_skin_linear(const float* M, float* L, float* C) {
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) L[3 * i + j] = M[4 * i + j];
    C[0] = L[4] * L[8] - L[5] * L[7];
    C[1] = L[5] * L[6] - L[3] * L[8];
    C[2] = L[3] * L[7] - L[4] * L[6];
    C[3] = L[2] * L[7] - L[1] * L[8];
    C[4] = L[0] * L[8] - L[2] * L[6];
    C[5] = L[1] * L[6] - L[0] * L[7];
    C[6] = L[1] * L[5] - L[2] * L[4];
    C[7] = L[2] * L[3] - L[0] * L[5];
    C[8] = L[0] * L[4] - L[1] * L[3];
}

// one corner: rest position, normal, tangent -> the posed ones (the outputs must not overlap the inputs)
ER_XF_HD inline void er_skin_corner(const float* P, const uint32_t* b, const float* w, const float* x, const float* n, const float* t, float* ox, float* on, float* ot) {
    float M[12], L[9], C[9];
    er_skin_blend(P, b, w, M);
    er_skin_linear(M, L, C);
    er_xform_point(M, x, ox);
    er_xform_dir(C, n, on);
    er_xform_dir(L, t, ot);
}

// ---- host only from here on ----

// one triangle: its twelve influences as stored ([3][ER_SKIN_K] each) and [3][3] rest vertices, normals, tangents
inline void er_skin_triangle(const float* P, const uint16_t* bones, const float* weights, const float* rv, const float* rn, const float* rt, float* ov, float* on, float* ot) {
    for (int j = 0; j < 3; j++) {
        uint32_t b[ER_SKIN_K];
        for (int k = 0; k < ER_SKIN_K; k++) b[k] = bones[ER_SKIN_K * j + k];
        er_skin_corner(P, b, weights + ER_SKIN_K * j, rv + 3 * j, rn + 3 * j, rt + 3 * j, ov + 3 * j, on + 3 * j, ot + 3 * j);
    }
}

// true if `count` triangles' influences may be used with a palette of bone_count bones; else `why` says what is wrong.  A bone index is
// checked also where its weight is 0: the blend reads that matrix.
inline bool er_skin_influences_ok(uint32_t bone_count, size_t count, const uint16_t* bones, const float* weights, std::string& why) {
    if (bone_count == 0 || bone_count > ER_SKIN_BONES_MAX) { why = "bone_count " + std::to_string(bone_count) + " is not in 1.." + std::to_string(ER_SKIN_BONES_MAX); return false; }
    if (count && (!bones || !weights)) { why = "a skin without bones or weights"; return false; }
    for (size_t i = 0; i < count * 3 * ER_SKIN_K; i++) {
        if (bones[i] >= bone_count) { why = "bones[" + std::to_string(i) + "] = " + std::to_string(bones[i]) + " is not below bone_count " + std::to_string(bone_count); return false; }
        if (!std::isfinite(weights[i]) || !(weights[i] >= 0.0f && weights[i] <= 1.0f)) { why = "weights[" + std::to_string(i) + "] is not a finite number in [0, 1]"; return false; }
    }
    return true;
}

// the host form on caller arrays: count triangles (er_debug_skin_apply); false = the influences do not fit the palette
inline bool er_skin_apply(const float* P, uint32_t bone_count, uint32_t count, const uint16_t* bones, const float* weights, const float* rv, const float* rn, const float* rt,
                          float* ov, float* on, float* ot, std::string& why) {
    if (!er_skin_influences_ok(bone_count, count, bones, weights, why)) return false;
    for (size_t i = 0; i < (size_t)count; i++)
        er_skin_triangle(P, bones + i * 3 * ER_SKIN_K, weights + i * 3 * ER_SKIN_K, rv + i * 9, rn + i * 9, rt + i * 9, ov + i * 9, on + i * 9, ot + i * 9);
    return true;
}

// The skins of a scene, kept BESIDE its ErObjectTable and indexed like it: per object the influences in the order of its rows of the rest
// copy, the last palette (storage for bone_count matrices from er_skin_set on, so that marking never allocates), and `kind`: how the
// object's current absolute pose was given -- 0 by matrix (er_render_transform; also "never posed"), 1 by palette (er_render_skin).  The
// table's own `pending` says whether the host arrays still lack that pose; `kind` says which arithmetic applies it.
// Empty vectors until the first er_skin_set; cleared whenever the table is replaced or renumbered (skins do not survive that).
struct ErSkinRecord {
    uint32_t bone_count = 0;                  // 0: the object has no skin
    std::vector<uint16_t> bones;              // [size_of(object)][3][ER_SKIN_K]
    std::vector<float> weights;               // the same shape
    std::vector<float> palette;               // [bone_count][12]
};
struct ErSkinTable {
    std::vector<ErSkinRecord> rec;            // [objects], or empty
    std::vector<uint8_t> kind;                // [objects], or empty
    std::vector<uint32_t> row_first;          // [objects + 1]: the rows of the skinned objects before each one (the device store's order)
    uint32_t skinned = 0;
    bool has(uint32_t o) const { return o < rec.size() && rec[o].bone_count != 0; }
    uint32_t rows() const { return row_first.empty() ? 0u : row_first.back(); }
    void clear() { rec.clear(); kind.clear(); row_first.clear(); skinned = 0; }
};

// The checks of er_skin_set, with nothing touched: k.object, k.bone_count, k.bones, k.weights (ErSkin).  bone_count 0 removes the skin
// and reads neither array.
template <class S>
inline bool er_skin_check(const ErObjectTable& t, const S& k, std::string& why) {
    const uint32_t objects = t.objects();
    if (k.object >= objects) { why = "object " + std::to_string(k.object) + " is not below the object count " + std::to_string(objects); return false; }
    if (t.size_of(k.object) == 0) { why = "object " + std::to_string(k.object) + " holds no triangle"; return false; }
    if (k.bone_count == 0) return true;
    return er_skin_influences_ok(k.bone_count, t.size_of(k.object), k.bones, k.weights, why);
}

// a checked skin into K (replacing the object's earlier one); what can fail here for want of memory fails before K changes
template <class S>
inline void er_skin_take(ErSkinTable& K, const ErObjectTable& t, const S& k) {
    const uint32_t objects = t.objects(), o = k.object;
    if (k.bone_count == 0 && !K.has(o)) return;
    ErSkinRecord r;
    if (k.bone_count) {
        const size_t m = (size_t)t.size_of(o) * 3 * ER_SKIN_K;
        r.bone_count = k.bone_count;
        r.bones.assign(k.bones, k.bones + m);
        r.weights.assign(k.weights, k.weights + m);
        r.palette.assign((size_t)k.bone_count * 12, 0.0f);
    }
    if (K.rec.size() != objects) {
        std::vector<ErSkinRecord> rec(objects);
        std::vector<uint8_t> kind(objects, (uint8_t)0);
        std::vector<uint32_t> row_first((size_t)objects + 1, 0u);
        K.rec.swap(rec); K.kind.swap(kind); K.row_first.swap(row_first);
        K.skinned = 0;
    }
    // An object that loses or changes its skin while a palette pose is still pending keeps that pose: the caller flushes first.  `kind`
    // stays: the object lies where its last pose put it.
    std::swap(K.rec[o], r);
    K.skinned = 0;
    for (uint32_t i = 0; i < objects; i++) {
        K.row_first[i + 1] = K.row_first[i] + (K.has(i) ? t.size_of(i) : 0u);
        K.skinned += K.has(i) ? 1u : 0u;
    }
}

// The checks of er_render_skin's list, O(listed objects + listed bones) time and memory: p[i].object, p[i].bone_count, p[i].palette
// (ErSkinPose).  0 = passed: `entries` and `palette` hold what is uploaded and `moved` the triangles of the listed objects; 1 = an
// invalid argument; 2 = a listed object has no skin (a state error: er_skin_set comes first).
template <class P>
inline int er_skin_pose_check(const ErObjectTable& t, const ErSkinTable& K, uint32_t count, const P* p, std::vector<ErSkinEntry>& entries, std::vector<float>& palette,
                              uint32_t& moved, std::string& why) {
    if (count == 0) { why = "the geometry bit with count 0"; return 1; }
    if (!p) { why = "the geometry bit without poses"; return 1; }
    const uint32_t objects = t.objects();
    for (uint32_t i = 0; i < count; i++)
        if (p[i].object >= objects) { why = "poses[" + std::to_string(i) + "].object = " + std::to_string(p[i].object) + " is not below the object count " + std::to_string(objects); return 1; }
    if (count > objects) { why = "more poses than objects: an object is listed twice"; return 1; }
    std::vector<uint32_t> sorted(count);
    for (uint32_t i = 0; i < count; i++) sorted[i] = p[i].object;
    std::sort(sorted.begin(), sorted.end());
    const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
    if (twice != sorted.end()) { why = "object " + std::to_string(*twice) + " is listed twice"; return 1; }
    for (uint32_t i = 0; i < count; i++)
        if (!K.has(p[i].object)) { why = "object " + std::to_string(p[i].object) + " has no skin (er_skin_set)"; return 2; }
    size_t bones = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (p[i].bone_count != K.rec[p[i].object].bone_count) {
            why = "poses[" + std::to_string(i) + "].bone_count = " + std::to_string(p[i].bone_count) + ", the object's skin has " + std::to_string(K.rec[p[i].object].bone_count);
            return 1;
        }
        if (!p[i].palette) { why = "poses[" + std::to_string(i) + "] without a palette"; return 1; }
        bones += p[i].bone_count;
    }
    entries.assign(count, ErSkinEntry{});
    palette.resize(bones * 12);
    moved = 0;
    uint32_t pal = 0;
    for (uint32_t i = 0; i < count; i++) {
        ErSkinEntry& e = entries[i];
        e.object = p[i].object; e.start = moved; e.row = K.row_first[e.object]; e.pal = pal; e.bones = p[i].bone_count;
        const std::string who = "poses[" + std::to_string(i) + "]";
        for (uint32_t b = 0; b < e.bones; b++) {
            const float* m = p[i].palette + (size_t)b * 12;
            float N[9], T[9];
            for (int k = 0; k < 12; k++)
                if (!std::isfinite(m[k])) { why = who + ": an entry of bone " + std::to_string(b) + " is not finite"; return 1; }
            if (!er_xform_derive(m, N, T)) { why = who + ": det(L) of bone " + std::to_string(b) + " is not > 0 (a mirror or a singular matrix)"; return 1; }
            if (!er_xform_bound_ok(m, &t.bound[(size_t)e.object * 3])) { why = who + ": bone " + std::to_string(b) + " would take the object out of the float range (bound 1e37)"; return 1; }
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++)
                if (!(std::fabs(m[4 * r + c]) <= ER_SKIN_MAX_LINEAR)) { why = who + ": a linear entry of bone " + std::to_string(b) + " is beyond " + std::to_string((int)ER_SKIN_MAX_LINEAR); return 1; }
            std::copy(m, m + 12, &palette[((size_t)pal + b) * 12]);
        }
        pal += e.bones;
        moved += t.size_of(e.object);
    }
    return 0;
}

// what er_render_skin does to the host copy: palette, kind and flag, no triangle touched.  Nothing here allocates or can fail.
inline void er_skin_mark(ErObjectTable& t, ErSkinTable& K, const ErSkinEntry* entries, uint32_t count, const float* palette) noexcept {
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t o = entries[i].object;
        std::copy(palette + (size_t)entries[i].pal * 12, palette + ((size_t)entries[i].pal + entries[i].bones) * 12, K.rec[o].palette.begin());
        K.kind[o] = 1;
        if (!t.pending[o]) { t.pending[o] = 1; t.pending_count++; }
    }
}

// what er_render_transform adds where skins exist: the listed objects' poses are matrices now.  True if one of them was posed by palette.
inline bool er_skin_mark_matrix(ErSkinTable& K, const ErXformEntry* entries, uint32_t count) noexcept {
    bool was = false;
    if (K.kind.empty()) return false;
    for (uint32_t i = 0; i < count; i++) {
        was = was || K.kind[entries[i].object] != 0;
        K.kind[entries[i].object] = 0;
    }
    return was;
}

// The pending poses of BOTH kinds into the scene's [tri_count][3][3] arrays: called wherever those arrays are read or partly overwritten.
// Nothing here allocates or can fail (the palettes passed er_skin_pose_check, the matrices er_xform_check).
inline void er_skin_flush(ErObjectTable& t, ErSkinTable& K, float* v, float* n, float* tg) noexcept {
    if (!t.pending_count) return;
    if (!K.kind.empty()) {
        const uint32_t objects = t.objects();
        for (uint32_t o = 0; o < objects; o++) {
            if (!t.pending[o] || K.kind[o] != 1 || !K.has(o)) continue;
            const ErSkinRecord& r = K.rec[o];
            for (uint32_t j = t.first[o]; j < t.first[o + 1]; j++) {
                const size_t from = (size_t)j * 9, to = (size_t)t.ids[j] * 9, at = (size_t)(j - t.first[o]) * 3 * ER_SKIN_K;
                er_skin_triangle(r.palette.data(), &r.bones[at], &r.weights[at], &t.rest_v[from], &t.rest_n[from], &t.rest_t[from], v + to, n + to, tg + to);
            }
            t.pending[o] = 0;
            t.pending_count--;
        }
    }
    er_objects_flush(t, v, n, tg);
}

// er_objects_set and er_render_topology: the table changes, every skin goes (the caller has flushed)
inline void er_skin_drop(ErSkinTable& K) noexcept { K.clear(); }
