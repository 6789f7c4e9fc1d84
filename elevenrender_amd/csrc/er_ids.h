// er_ids.h -- id planes, coverage mattes and picking (include/eleven_hip.h er_render_ids, er_id_info, er_read_ids, er_gather_ids,
// er_id_matte, er_pick_rect, er_pick; er_ids.hip has the kernels and entry points).  The small integer routines the
// kernels, the host and the tests share are stated ONCE here: the ranking of a pixel's ids, the membership search of the matte and the
// object search of the tri -> object scatter.  Plain C++ plus __host__ __device__, without a HIP or library header:
// tests/native/ids_host.cpp compiles this file alone under ASan + UBSan; er_debug_id_rank exports the ranking and
// elevenrender_amd/ids.py restates it in numpy.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/eleven_hip.h"      // ER_ID_NONE, ER_ID_SLOTS, ER_ID_KIND_COUNT

#if defined(__HIPCC__)
#define ER_ID_HD __host__ __device__
#else
#define ER_ID_HD
#endif

// (count, id) a ranks before (count, id) b: count descending, then id ascending as unsigned -- so ER_ID_NONE is last among equals and an
// empty slot (ER_ID_NONE, 0) is behind every entry
ER_ID_HD inline bool er_id_before(uint32_t ca, uint32_t ia, uint32_t cb, uint32_t ib) { return ca > cb || (ca == cb && ia < ib); }

// The ranking of one pixel.  ids[j * stride], j < m: the ids of the m rays that hit (misses are not in the array), in any order, m <=
// 64.  out_id / out_count [ER_ID_SLOTS]: the distinct ids by (count descending, id ascending), the first ER_ID_SLOTS of them; unused
// slots are (ER_ID_NONE, 0).  Returns the number of distinct ids (more than ER_ID_SLOTS: the pixel overflows).  Reads only; O(m^2)
// comparisons and no storage beyond the outputs, which is what lets a lane rank its own column of LDS words in registers.
ER_ID_HD inline uint32_t er_id_rank(const uint32_t* ids, size_t stride, uint32_t m, uint32_t* out_id, uint32_t* out_count) {
    uint32_t bi[ER_ID_SLOTS], bc[ER_ID_SLOTS];
    for (int s = 0; s < ER_ID_SLOTS; s++) { bi[s] = ER_ID_NONE; bc[s] = 0u; }
    uint32_t distinct = 0;
    for (uint32_t i = 0; i < m; i++) {
        const uint32_t id = ids[i * stride];
        bool seen = false;
        for (uint32_t j = 0; j < i; j++) seen = seen || ids[j * stride] == id;
        if (seen) continue;
        uint32_t c = 1;
        for (uint32_t j = i + 1; j < m; j++) c += ids[j * stride] == id ? 1u : 0u;
        distinct++;
        // one pass of an insertion: the candidate sinks to its place, what it displaces sinks on, the last one falls out
        uint32_t ci = id, cc = c;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int s = 0; s < ER_ID_SLOTS; s++)
            if (er_id_before(cc, ci, bc[s], bi[s])) {
                const uint32_t ti = bi[s], tc = bc[s];
                bi[s] = ci; bc[s] = cc;
                ci = ti; cc = tc;
            }
    }
    for (int s = 0; s < ER_ID_SLOTS; s++) { out_id[s] = bi[s]; out_count[s] = bc[s]; }
    return distinct;
}

// `id` is in the ascending, duplicate-free list[0 .. count): bisection, at most 32 steps
ER_ID_HD inline bool er_id_member(const uint32_t* list, uint32_t count, uint32_t id) {
    uint32_t lo = 0, hi = count;      // the first entry >= id lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (list[mid] < id) lo = mid + 1u;
        else hi = mid;
    }
    return lo < count && list[lo] == id;
}

// the object that holds CSR position j < first[objects]: the last o with first[o] <= j (empty objects share a `first` with their
// successor and are skipped)
ER_ID_HD inline uint32_t er_id_object_of(const uint32_t* first, uint32_t objects, uint32_t j) {
    uint32_t lo = 0, hi = objects;      // the first o with first[o] > j lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (first[mid] <= j) lo = mid + 1u;
        else hi = mid;
    }
    return lo - 1u;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
hipError_t er_probe_ids(const char** which);      // see er_kernels.h; er_render_begin asks it after er_probe_kernels
// the tri -> object map of the current table made current; the map, or NULL without a table.  The scene's mutex is held and its stream idle.
struct ErScene;
int er_id_prepare(ErScene* s);
const uint32_t* er_id_map(ErScene* s);
#endif

// the matte's list as the device searches it: ascending, each id once (host only)
inline std::vector<uint32_t> er_id_list_prepare(const uint32_t* ids, uint32_t count) {
    std::vector<uint32_t> l(ids, ids + count);
    std::sort(l.begin(), l.end());
    l.erase(std::unique(l.begin(), l.end()), l.end());
    return l;
}

// one pixel of er_id_matte: the counts of the slots whose id is in the list, over n
ER_ID_HD inline float er_id_matte_px(const uint32_t* slot_id, const uint32_t* slot_count, const uint32_t* list, uint32_t count, uint32_t n) {
    uint32_t sum = 0;
    for (int s = 0; s < ER_ID_SLOTS; s++)
        if (slot_count[s] && er_id_member(list, count, slot_id[s])) sum += slot_count[s];
    return (float)sum / (float)n;
}
