// er_sparse_host.h -- the host half of er_render_update_sparse that needs no device (er_api_edit.cpp): every check of the listed
// triangles with nothing touched, and the patch of the scene's host copy.  O(count) time and memory, whatever the scene's size.
// Plain C++ on purpose, without a HIP or library header: tests/native/sparse_patch.cpp compiles it alone under ASan + UBSan.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

struct ErSparseList {               // ErSparseUpdate's geometry fields
    uint32_t count = 0;
    const uint32_t* tri_ids = nullptr;
    const float* vertices = nullptr;
    const float* normals = nullptr;      // or NULL = keep
    const float* tangents = nullptr;     // or NULL = keep
};

// true if the list may be applied to a scene of tri_count triangles; else `why` says what is wrong with it
inline bool er_sparse_check(uint32_t tri_count, const ErSparseList& l, std::string& why) {
    if (l.count == 0) { why = "the geometry bit with count 0"; return false; }
    if (!l.tri_ids || !l.vertices) { why = "the geometry bit without tri_ids or vertices"; return false; }
    for (uint32_t i = 0; i < l.count; i++)
        if (l.tri_ids[i] >= tri_count) { why = "tri_ids[" + std::to_string(i) + "] = " + std::to_string(l.tri_ids[i]) + " is not below tri_count " + std::to_string(tri_count); return false; }
    if (l.count > tri_count) { why = "more ids than triangles: an id is listed twice"; return false; }
    std::vector<uint32_t> sorted(l.tri_ids, l.tri_ids + l.count);      // (a device scatter with two writers has no defined result)
    std::sort(sorted.begin(), sorted.end());
    const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
    if (twice != sorted.end()) { why = "triangle " + std::to_string(*twice) + " is listed twice"; return false; }
    const size_t n9 = (size_t)l.count * 9;
    for (size_t i = 0; i < n9; i++)
        if (!std::isfinite(l.vertices[i])) { why = "vertex " + std::to_string(i % 9 / 3) + " of listed triangle " + std::to_string(i / 9) + " is not finite"; return false; }
    return true;
}

// a checked list into the complete [tri_count][3][3] arrays; nothing here allocates or can fail
inline void er_sparse_patch(const ErSparseList& l, float* vertices, float* normals, float* tangents) noexcept {
    for (uint32_t i = 0; i < l.count; i++) {
        const size_t to = (size_t)l.tri_ids[i] * 9, from = (size_t)i * 9;
        std::copy(l.vertices + from, l.vertices + from + 9, vertices + to);
        if (l.normals) std::copy(l.normals + from, l.normals + from + 9, normals + to);
        if (l.tangents) std::copy(l.tangents + from, l.tangents + from + 9, tangents + to);
    }
}
