// er_topology_host.h -- the host half of er_render_topology that needs no device (er_api_edit.cpp): the numbering, every
// check of the two lists with nothing touched, the compaction of the scene's host arrays and the remap of its object table.
// Plain C++ on purpose, without a HIP or library header (er_xform.h, which has the object table, is plain too):
// tests/native/topology_patch.cpp compiles it alone under ASan + UBSan; elevenrender_amd/topology.py restates it in numpy.
//
// THE NUMBERING.  A topology edit removes the listed triangles, then appends the given ones:
//   survivors keep their relative order:  new_id(old) = old - |{r in remove_ids : r < old}|
//   appended triangle j gets id            survivors + j,   survivors = tri_count - remove_count
// Everything that lives in triangle-id space follows it: the six host arrays, the device-resident geometry store (er_topology.hip, the
// same ordered gather), the object table's id lists, and -- by being made again -- the records' tri_id, the emitter table and the
// tri -> object map.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "er_xform.h"

#define ER_TOPO_HOST_REMOVE 1u      // = ER_TOPO_REMOVE, ER_TOPO_APPEND of include/eleven_hip.h (er_api_edit.cpp asserts it)
#define ER_TOPO_HOST_APPEND 2u

struct ErTopoList {                 // ErTopologyEdit's own fields
    uint32_t what = 0;
    uint32_t remove_count = 0;
    const uint32_t* remove_ids = nullptr;
    uint32_t append_count = 0;
    const float *vertices = nullptr, *normals = nullptr, *tangents = nullptr, *uvs = nullptr, *tangent_sign = nullptr;
    const int32_t* material_id = nullptr;
    uint32_t append_as_object = 0;
    uint32_t removes() const { return (what & ER_TOPO_HOST_REMOVE) ? remove_count : 0u; }
    uint32_t appends() const { return (what & ER_TOPO_HOST_APPEND) ? append_count : 0u; }
};

// true if the lists may be applied to a scene of tri_count triangles; else `why` says what is wrong.  On success `sorted` holds the
// removed ids ascending (what every later step works from) and `new_count` the resulting triangle count.  O(remove_count log
// remove_count + append_count) time, O(remove_count) memory, whatever the scene's size.  Material ids are the caller's to check: the
// resulting material list is not known here.
inline bool er_topo_check(uint32_t tri_count, const ErTopoList& l, std::vector<uint32_t>& sorted, uint32_t& new_count, std::string& why) {
    if ((l.what & (ER_TOPO_HOST_REMOVE | ER_TOPO_HOST_APPEND)) == 0) { why = "`what` names neither ER_TOPO_REMOVE nor ER_TOPO_APPEND"; return false; }
    if (l.what & ~(ER_TOPO_HOST_REMOVE | ER_TOPO_HOST_APPEND)) { why = "`what` has unknown bits"; return false; }
    sorted.clear();
    if (l.what & ER_TOPO_HOST_REMOVE) {
        if (l.remove_count == 0) { why = "ER_TOPO_REMOVE with remove_count 0"; return false; }
        if (!l.remove_ids) { why = "ER_TOPO_REMOVE without remove_ids"; return false; }
        for (uint32_t i = 0; i < l.remove_count; i++)
            if (l.remove_ids[i] >= tri_count) { why = "remove_ids[" + std::to_string(i) + "] = " + std::to_string(l.remove_ids[i]) + " is not below tri_count " + std::to_string(tri_count); return false; }
        if (l.remove_count > tri_count) { why = "more removed ids than triangles: an id is listed twice"; return false; }
        sorted.assign(l.remove_ids, l.remove_ids + l.remove_count);
        std::sort(sorted.begin(), sorted.end());
        const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
        if (twice != sorted.end()) { why = "triangle " + std::to_string(*twice) + " is removed twice"; return false; }
    }
    if (l.what & ER_TOPO_HOST_APPEND) {
        if (l.append_count == 0) { why = "ER_TOPO_APPEND with append_count 0"; return false; }
        if (!l.vertices || !l.normals || !l.tangents || !l.uvs || !l.tangent_sign || !l.material_id) { why = "ER_TOPO_APPEND without one of its six arrays"; return false; }
        const size_t n9 = (size_t)l.append_count * 9;
        for (size_t i = 0; i < n9; i++)
            if (!std::isfinite(l.vertices[i])) { why = "vertex " + std::to_string(i % 9 / 3) + " of appended triangle " + std::to_string(i / 9) + " is not finite"; return false; }
    }
    const uint64_t total = (uint64_t)tri_count - l.removes() + l.appends();
    if (total > 0xffffffffull) { why = "the resulting triangle count does not fit 32 bits"; return false; }
    new_count = (uint32_t)total;
    return true;
}

// new_id of a SURVIVING old id (sorted: the removed ids ascending)
inline uint32_t er_topo_new_id(const std::vector<uint32_t>& sorted, uint32_t old_id) {
    return old_id - (uint32_t)(std::lower_bound(sorted.begin(), sorted.end(), old_id) - sorted.begin());
}
inline bool er_topo_removed(const std::vector<uint32_t>& sorted, uint32_t old_id) { return std::binary_search(sorted.begin(), sorted.end(), old_id); }

// The survivors of a [n][stride] array moved down in place, in order: the runs between removed ids, one memmove each.  Returns the
// survivors.  Nothing here allocates or can fail.
template <class T>
inline uint32_t er_topo_compact(T* a, size_t stride, uint32_t n, const std::vector<uint32_t>& sorted) noexcept {
    uint32_t out = 0, from = 0;
    for (size_t k = 0; k <= sorted.size(); k++) {
        const uint32_t to = k < sorted.size() ? sorted[k] : n;      // the run [from, to) survives
        if (to > from) {
            if (out != from) memmove(a + (size_t)out * stride, a + (size_t)from * stride, (size_t)(to - from) * stride * sizeof(T));
            out += to - from;
        }
        from = to + 1;
    }
    return out;
}

// The scene's six arrays edited: storage for the result is reserved FIRST (an allocation that fails leaves every array as it was),
// then the compaction and the append, which cannot fail.  n: the current count; sorted: from er_topo_check.
struct ErTopoArrays {
    std::vector<float>*vertices, *normals, *tangents, *uvs, *tangent_sign;
    std::vector<int32_t>* material_id;
};
inline void er_topo_reserve(const ErTopoArrays& a, uint32_t new_count) {
    a.vertices->reserve((size_t)new_count * 9); a.normals->reserve((size_t)new_count * 9); a.tangents->reserve((size_t)new_count * 9);
    a.uvs->reserve((size_t)new_count * 6); a.tangent_sign->reserve(new_count); a.material_id->reserve(new_count);
}
template <class T>
inline void er_topo_apply_one(std::vector<T>& v, size_t stride, uint32_t n, const std::vector<uint32_t>& sorted, const T* tail, uint32_t appended) noexcept {
    const uint32_t kept = er_topo_compact(v.data(), stride, n, sorted);
    v.resize((size_t)kept * stride);                                       // (shrinks: no allocation)
    if (appended) v.insert(v.end(), tail, tail + (size_t)appended * stride);      // (within the reserved capacity: no allocation)
}
inline uint32_t er_topo_apply(const ErTopoArrays& a, uint32_t n, const std::vector<uint32_t>& sorted, const ErTopoList& l) noexcept {
    const uint32_t ap = l.appends();
    er_topo_apply_one(*a.vertices, 9, n, sorted, l.vertices, ap);
    er_topo_apply_one(*a.normals, 9, n, sorted, l.normals, ap);
    er_topo_apply_one(*a.tangents, 9, n, sorted, l.tangents, ap);
    er_topo_apply_one(*a.uvs, 6, n, sorted, l.uvs, ap);
    er_topo_apply_one(*a.tangent_sign, 1, n, sorted, l.tangent_sign, ap);
    er_topo_apply_one(*a.material_id, 1, n, sorted, l.material_id, ap);
    return n - (uint32_t)sorted.size() + ap;
}

// The object table after the edit, made beside the old one (swap it in after the last allocation).  Removed ids leave their objects
// (an object may become empty); surviving rows keep their rest copy, their order and the object's last matrix; bounds are recomputed from
// the surviving rest rows; with l.append_as_object and a table present the appended triangles become a new LAST object whose rest pose is
// the arrays given (identity matrix).  Without a table the flag is ignored.  The pending poses must have been flushed
// (er_objects_flush): the result has none pending.
inline void er_topo_remap_objects(const ErObjectTable& t, uint32_t tri_count, const std::vector<uint32_t>& sorted, const ErTopoList& l, ErObjectTable& out) {
    ErObjectTable x;
    const uint32_t objects = t.objects();
    if (objects) {
        const uint32_t ap = l.append_as_object ? l.appends() : 0u, survivors = tri_count - (uint32_t)sorted.size();
        const uint32_t total = objects + (ap ? 1u : 0u);
        x.first.reserve((size_t)total + 1);
        x.first.push_back(0u);
        x.ids.reserve(t.ids.size() + ap);
        x.rest_v.reserve((t.ids.size() + ap) * 9); x.rest_n.reserve((t.ids.size() + ap) * 9); x.rest_t.reserve((t.ids.size() + ap) * 9);
        x.bound.assign((size_t)total * 3, 0.0f);
        x.last_m.assign((size_t)total * 12, 0.0f);
        x.pending.assign(total, (uint8_t)0);
        for (uint32_t o = 0; o < objects; o++) {
            float* B = &x.bound[(size_t)o * 3];
            for (uint32_t j = t.first[o]; j < t.first[o + 1]; j++) {
                if (er_topo_removed(sorted, t.ids[j])) continue;
                x.ids.push_back(er_topo_new_id(sorted, t.ids[j]));
                const size_t from = (size_t)j * 9;
                x.rest_v.insert(x.rest_v.end(), &t.rest_v[from], &t.rest_v[from] + 9);
                x.rest_n.insert(x.rest_n.end(), &t.rest_n[from], &t.rest_n[from] + 9);
                x.rest_t.insert(x.rest_t.end(), &t.rest_t[from], &t.rest_t[from] + 9);
                for (int k = 0; k < 9; k++) B[k % 3] = std::max(B[k % 3], std::fabs(t.rest_v[from + k]));
            }
            x.first.push_back((uint32_t)x.ids.size());
            std::copy(&t.last_m[(size_t)o * 12], &t.last_m[(size_t)o * 12] + 12, &x.last_m[(size_t)o * 12]);
        }
        if (ap) {
            float* B = &x.bound[(size_t)objects * 3];
            for (uint32_t j = 0; j < ap; j++) x.ids.push_back(survivors + j);
            x.rest_v.insert(x.rest_v.end(), l.vertices, l.vertices + (size_t)ap * 9);
            x.rest_n.insert(x.rest_n.end(), l.normals, l.normals + (size_t)ap * 9);
            x.rest_t.insert(x.rest_t.end(), l.tangents, l.tangents + (size_t)ap * 9);
            for (size_t k = 0; k < (size_t)ap * 9; k++) B[k % 3] = std::max(B[k % 3], std::fabs(l.vertices[k]));
            x.first.push_back((uint32_t)x.ids.size());
            for (int k = 0; k < 3; k++) x.last_m[(size_t)objects * 12 + 5 * k] = 1.0f;      // the identity
        }
    }
    std::swap(out, x);
}
