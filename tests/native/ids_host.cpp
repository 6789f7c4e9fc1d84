// ids_host.cpp -- the host functions of csrc/er_ids.h alone: the ranking of a pixel's ids, the membership search of the matte, the object
// search and the tri -> object map, the list preparation and a matte pixel, on heap arrays of exactly the sizes the contract names.
// Built with -fsanitize=address,undefined by tests/test_ids_cpu.py: a read past the m ids of a pixel, past a list's last entry or past
// `first`, or a write past the four slots or past tri_count words of the map, is reported.
// Prints "ids_host ok" and returns 0, or says which expectation failed.
#include <cstdio>
#include <map>
#include <memory>
#include <numeric>
#include <random>

#include "er_ids.h"

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); failures++; } } while (0)

// the definition, the slow way: distinct ids by (count descending, id ascending)
static void rank_by_definition(const uint32_t* ids, uint32_t m, uint32_t* oi, uint32_t* oc, uint32_t& distinct) {
    std::map<uint32_t, uint32_t> count;
    for (uint32_t i = 0; i < m; i++) count[ids[i]]++;
    std::vector<std::pair<uint32_t, uint32_t>> v(count.begin(), count.end());      // ascending ids
    std::stable_sort(v.begin(), v.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.second > b.second; });
    distinct = (uint32_t)v.size();
    for (uint32_t s = 0; s < ER_ID_SLOTS; s++) {
        oi[s] = s < v.size() ? v[s].first : ER_ID_NONE;
        oc[s] = s < v.size() ? v[s].second : 0u;
    }
}

// tri -> object as k_id_map_scatter (er_ids.hip) fills it: ER_ID_NONE, then one writer per listed id, its object by er_id_object_of
static void map_as_the_scatter(uint32_t tri_count, uint32_t objects, const uint32_t* first, const uint32_t* tri_ids, uint32_t* map) {
    for (uint32_t t = 0; t < tri_count; t++) map[t] = ER_ID_NONE;
    const uint32_t total = objects ? first[objects] : 0u;
    for (uint32_t j = 0; j < total; j++)
        if (tri_ids[j] < tri_count) map[tri_ids[j]] = er_id_object_of(first, objects, j);
}

static void check_rank(const uint32_t* ids, uint32_t m, size_t stride) {
    // exact-size outputs on the heap: a fifth slot written is an overflow
    std::unique_ptr<uint32_t[]> oi(new uint32_t[ER_ID_SLOTS]), oc(new uint32_t[ER_ID_SLOTS]);
    uint32_t wi[ER_ID_SLOTS], wc[ER_ID_SLOTS], wd = 0;
    std::unique_ptr<uint32_t[]> flat(new uint32_t[m ? m : 1]);
    for (uint32_t i = 0; i < m; i++) flat[i] = ids[i * stride];
    rank_by_definition(flat.get(), m, wi, wc, wd);
    const uint32_t d = er_id_rank(ids, stride, m, oi.get(), oc.get());
    EXPECT(d == wd);
    for (int s = 0; s < ER_ID_SLOTS; s++) { EXPECT(oi[s] == wi[s]); EXPECT(oc[s] == wc[s]); }
}

int main() {
    std::mt19937 gen(5);
    {   // the ranking: every m from 0 to 64, arrays of exactly m words; few ids (ties), many ids (overflow), ER_ID_NONE among them
        for (uint32_t m = 0; m <= 64; m++)
            for (uint32_t spread : {1u, 3u, 6u, 200u}) {
                std::unique_ptr<uint32_t[]> ids(new uint32_t[m]);
                for (uint32_t i = 0; i < m; i++) {
                    const uint32_t r = gen() % spread;
                    ids[i] = r == 2u ? ER_ID_NONE : r * 0x9E3779B1u;
                }
                check_rank(ids.get(), m, 1);
            }
        std::unique_ptr<uint32_t[]> all(new uint32_t[64]);
        std::iota(all.get(), all.get() + 64, 100u);
        std::shuffle(all.get(), all.get() + 64, gen);
        check_rank(all.get(), 64, 1);                                     // 64 distinct
        std::fill(all.get(), all.get() + 64, 7u);
        check_rank(all.get(), 64, 1);                                     // 64 equal
        const uint32_t tie[13] = {9, 9, 9, 5, 5, 8, 8, 2, 3, 3, 7, 7, 1};      // the fourth and the fifth are tied: the smaller id stays
        std::unique_ptr<uint32_t[]> t(new uint32_t[13]);
        std::copy(tie, tie + 13, t.get());
        uint32_t oi[ER_ID_SLOTS], oc[ER_ID_SLOTS];
        EXPECT(er_id_rank(t.get(), 1, 13, oi, oc) == 7u);
        EXPECT(oi[0] == 9u && oi[1] == 3u && oi[2] == 5u && oi[3] == 7u && oc[0] == 3u && oc[1] == 2u && oc[2] == 2u && oc[3] == 2u);
        EXPECT(er_id_rank(nullptr, 1, 0, oi, oc) == 0u);                  // zero hits: nothing is read
        EXPECT(oi[0] == ER_ID_NONE && oi[3] == ER_ID_NONE && oc[0] == 0u && oc[3] == 0u);
        // the kernel's layout: a lane's column of a [k][64] array; lane 63's last word is the array's last
        const uint32_t n = 64, lanes = 64;
        std::unique_ptr<uint32_t[]> cols(new uint32_t[n * lanes]);
        for (uint32_t i = 0; i < n * lanes; i++) cols[i] = gen() % 9u;
        for (uint32_t lane : {0u, 31u, 63u}) check_rank(cols.get() + lane, n, lanes);
    }
    {   // the list of a matte: duplicates go, order comes; membership at both ends, between entries and beyond
        const uint32_t raw[7] = {40, ER_ID_NONE, 3, 40, 17, 3, 0};
        std::unique_ptr<uint32_t[]> in(new uint32_t[7]);
        std::copy(raw, raw + 7, in.get());
        const std::vector<uint32_t> l = er_id_list_prepare(in.get(), 7);
        EXPECT(l.size() == 5 && l[0] == 0u && l[1] == 3u && l[2] == 17u && l[3] == 40u && l[4] == ER_ID_NONE);
        std::unique_ptr<uint32_t[]> list(new uint32_t[l.size()]);
        std::copy(l.begin(), l.end(), list.get());
        for (uint32_t id : {0u, 3u, 17u, 40u, ER_ID_NONE}) EXPECT(er_id_member(list.get(), 5, id));
        for (uint32_t id : {1u, 2u, 4u, 16u, 18u, 39u, 41u, ER_ID_NONE - 1u}) EXPECT(!er_id_member(list.get(), 5, id));
        EXPECT(!er_id_member(list.get(), 0, 3u));                         // an empty list: nothing is read
        std::unique_ptr<uint32_t[]> one(new uint32_t[1]);
        one[0] = 5u;
        EXPECT(er_id_member(one.get(), 1, 5u) && !er_id_member(one.get(), 1, 4u) && !er_id_member(one.get(), 1, 6u));
        // a pixel: slots (3, 2) (ER_ID_NONE, 1) (8, 1) and an empty one, n = 4
        std::unique_ptr<uint32_t[]> si(new uint32_t[ER_ID_SLOTS]), sc(new uint32_t[ER_ID_SLOTS]);
        const uint32_t i4[4] = {3, ER_ID_NONE, 8, ER_ID_NONE}, c4[4] = {2, 1, 1, 0};
        std::copy(i4, i4 + 4, si.get());
        std::copy(c4, c4 + 4, sc.get());
        EXPECT(er_id_matte_px(si.get(), sc.get(), list.get(), 5, 4) == 0.75f);      // 3 and ER_ID_NONE are members, 8 is not; the empty slot adds nothing
        EXPECT(er_id_matte_px(si.get(), sc.get(), one.get(), 1, 4) == 0.0f);
    }
    {   // the object of a CSR position, empty objects at the front, in the middle and at the end; the map
        const uint32_t objects = 7, total = 9, tri_count = 12;
        const uint32_t f[objects + 1] = {0, 0, 3, 3, 3, 4, 9, 9};
        std::unique_ptr<uint32_t[]> first(new uint32_t[objects + 1]), ids(new uint32_t[total]), map(new uint32_t[tri_count]);
        std::copy(f, f + objects + 1, first.get());
        const uint32_t want[total] = {1, 1, 1, 4, 5, 5, 5, 5, 5};
        for (uint32_t j = 0; j < total; j++) EXPECT(er_id_object_of(first.get(), objects, j) == want[j]);
        const uint32_t tri[total] = {11, 0, 5, 7, 2, 3, 10, 1, 8};
        std::copy(tri, tri + total, ids.get());
        map_as_the_scatter(tri_count, objects, first.get(), ids.get(), map.get());
        const uint32_t m[tri_count] = {1, 5, 5, 5, ER_ID_NONE, 1, ER_ID_NONE, 4, 5, ER_ID_NONE, 5, 1};
        for (uint32_t t = 0; t < tri_count; t++) EXPECT(map[t] == m[t]);
        map_as_the_scatter(tri_count, 0, nullptr, nullptr, map.get());        // no table: nothing is read
        for (uint32_t t = 0; t < tri_count; t++) EXPECT(map[t] == ER_ID_NONE);
    }
    if (failures) { std::printf("ids_host: %d expectations failed\n", failures); return 1; }
    std::printf("ids_host ok\n");
    return 0;
}
