// topology_patch.cpp -- csrc/er_topology_host.h alone (tests/test_topology_cpu.py builds it with ASan + UBSan): every refusal of
// er_topo_check with its text, the compaction of the host arrays on heap arrays of exactly the sizes the contract names (a read or
// write past them is reported), and the remap of the object table against hand-written cases.
//   topology_patch            the checks above; prints "topology_patch ok"
//   topology_patch apply      reads a case from stdin -- tri_count, remove_count, the ids, append_count, as_object, object_count, then
//                             per object its size and ids -- and prints what the header makes of it: line 1 the old id of every
//                             resulting triangle (-1 - j for appended triangle j), then one line per resulting object
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "er_topology_host.h"

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } \
    } while (0)

struct Scene {      // six arrays of exactly n triangles; material_id[i] = i and vertices[9 i + k] = 100 i + k name every row
    uint32_t n;
    std::vector<float> v, nn, t, uv, sg;
    std::vector<int32_t> m;
    explicit Scene(uint32_t n_) : n(n_), v((size_t)n_ * 9), nn((size_t)n_ * 9), t((size_t)n_ * 9), uv((size_t)n_ * 6), sg(n_), m(n_) {
        for (uint32_t i = 0; i < n; i++) {
            for (int k = 0; k < 9; k++) { v[(size_t)i * 9 + k] = 100.0f * i + k; nn[(size_t)i * 9 + k] = -(100.0f * i + k); t[(size_t)i * 9 + k] = 0.5f + 100.0f * i + k; }
            for (int k = 0; k < 6; k++) uv[(size_t)i * 6 + k] = 10.0f * i + k;
            sg[i] = (i & 1) ? -1.0f : 1.0f;
            m[i] = (int32_t)i;
        }
        v.shrink_to_fit(); nn.shrink_to_fit(); t.shrink_to_fit(); uv.shrink_to_fit(); sg.shrink_to_fit(); m.shrink_to_fit();
    }
    ErTopoArrays arrays() { return ErTopoArrays{&v, &nn, &t, &uv, &sg, &m}; }
};

static ErTopoList list_of(const std::vector<uint32_t>& rem, const Scene* app, uint32_t as_object = 0) {
    ErTopoList l;
    if (!rem.empty()) { l.what |= ER_TOPO_HOST_REMOVE; l.remove_count = (uint32_t)rem.size(); l.remove_ids = rem.data(); }
    if (app) {
        l.what |= ER_TOPO_HOST_APPEND; l.append_count = app->n;
        l.vertices = app->v.data(); l.normals = app->nn.data(); l.tangents = app->t.data(); l.uvs = app->uv.data(); l.tangent_sign = app->sg.data(); l.material_id = app->m.data();
    }
    l.append_as_object = as_object;
    return l;
}

static bool refused(uint32_t n, const ErTopoList& l, const char* word) {
    std::vector<uint32_t> sorted;
    uint32_t nc = 77;
    std::string why;
    if (er_topo_check(n, l, sorted, nc, why)) { printf("accepted, expected '%s'\n", word); return false; }
    if (why.find(word) == std::string::npos) { printf("refused with '%s', expected '%s'\n", why.c_str(), word); return false; }
    return true;
}

// the edit applied to a scene of n triangles; returns the old ids of the result (appended: 1000 + j, the tail's material ids)
static std::vector<int32_t> edit(uint32_t n, const std::vector<uint32_t>& rem, uint32_t app_n) {
    Scene s(n), tail(app_n);
    for (uint32_t j = 0; j < app_n; j++) tail.m[j] = 1000 + (int32_t)j;
    const ErTopoList l = list_of(rem, app_n ? &tail : nullptr);
    std::vector<uint32_t> sorted;
    uint32_t nc = 0;
    std::string why;
    if (!er_topo_check(n, l, sorted, nc, why)) { printf("unexpected refusal: %s\n", why.c_str()); failures++; return {}; }
    const ErTopoArrays A = s.arrays();
    er_topo_reserve(A, nc);
    const uint32_t got = er_topo_apply(A, n, sorted, l);
    CHECK(got == nc);
    CHECK(s.v.size() == (size_t)nc * 9 && s.nn.size() == (size_t)nc * 9 && s.t.size() == (size_t)nc * 9 && s.uv.size() == (size_t)nc * 6 && s.sg.size() == nc && s.m.size() == nc);
    // every row of every array is the row of the triangle its material id names
    const Scene ref(n), rtail(app_n);
    for (uint32_t i = 0; i < nc; i++) {
        const bool app = s.m[i] >= 1000;
        const uint32_t from = app ? (uint32_t)(s.m[i] - 1000) : (uint32_t)s.m[i];
        const Scene& r = app ? rtail : ref;
        for (int k = 0; k < 9; k++) { CHECK(s.v[(size_t)i * 9 + k] == r.v[(size_t)from * 9 + k]); CHECK(s.nn[(size_t)i * 9 + k] == r.nn[(size_t)from * 9 + k]); CHECK(s.t[(size_t)i * 9 + k] == r.t[(size_t)from * 9 + k]); }
        for (int k = 0; k < 6; k++) CHECK(s.uv[(size_t)i * 6 + k] == r.uv[(size_t)from * 6 + k]);
        CHECK(s.sg[i] == r.sg[from]);
    }
    return s.m;
}

static void test_refusals() {
    const Scene tail(2);
    const std::vector<uint32_t> ids{1, 3};
    ErTopoList l;
    CHECK(refused(5, l, "neither ER_TOPO_REMOVE nor ER_TOPO_APPEND"));
    l = list_of(ids, nullptr); l.what |= 4u;
    CHECK(refused(5, l, "unknown bits"));
    l = list_of(ids, nullptr); l.remove_count = 0;
    CHECK(refused(5, l, "remove_count 0"));
    l = list_of(ids, nullptr); l.remove_ids = nullptr;
    CHECK(refused(5, l, "without remove_ids"));
    l = list_of(ids, nullptr);
    CHECK(refused(3, l, "remove_ids[1] = 3 is not below tri_count 3"));
    const std::vector<uint32_t> twice{2, 0, 2};
    l = list_of(twice, nullptr);
    CHECK(refused(5, l, "triangle 2 is removed twice"));
    const std::vector<uint32_t> many{0, 1, 0};
    l = list_of(many, nullptr);
    CHECK(refused(2, l, "more removed ids than triangles"));
    l = list_of({}, &tail); l.append_count = 0;
    CHECK(refused(5, l, "append_count 0"));
    for (int k = 0; k < 6; k++) {
        l = list_of({}, &tail);
        if (k == 0) l.vertices = nullptr;
        if (k == 1) l.normals = nullptr;
        if (k == 2) l.tangents = nullptr;
        if (k == 3) l.uvs = nullptr;
        if (k == 4) l.tangent_sign = nullptr;
        if (k == 5) l.material_id = nullptr;
        CHECK(refused(5, l, "without one of its six arrays"));
    }
    Scene bad(2);
    bad.v[9 + 4] = INFINITY;
    l = list_of({}, &bad);
    CHECK(refused(5, l, "vertex 1 of appended triangle 1 is not finite"));
    bad.v[9 + 4] = NAN;
    CHECK(refused(5, l, "not finite"));
    l = list_of({}, &tail);
    CHECK(refused(0xffffffffu, l, "does not fit 32 bits"));
    // accepted: the lists sorted, the count
    std::vector<uint32_t> sorted;
    uint32_t nc = 0;
    std::string why;
    const std::vector<uint32_t> rem{4, 0, 2};
    l = list_of(rem, &tail);
    CHECK(er_topo_check(5, l, sorted, nc, why) && nc == 4 && sorted == (std::vector<uint32_t>{0, 2, 4}));
    CHECK(er_topo_new_id(sorted, 1) == 0 && er_topo_new_id(sorted, 3) == 1 && er_topo_removed(sorted, 2) && !er_topo_removed(sorted, 3));
}

static void test_compaction() {
    using V = std::vector<int32_t>;
    CHECK(edit(5, {0}, 0) == (V{1, 2, 3, 4}));                       // the first id
    CHECK(edit(5, {4}, 0) == (V{0, 1, 2, 3}));                       // the last id
    CHECK(edit(6, {5, 0, 2}, 0) == (V{1, 3, 4}));                    // unsorted list
    CHECK(edit(6, {1, 2, 3}, 2) == (V{0, 4, 5, 1000, 1001}));        // a run, and an append
    CHECK(edit(4, {}, 3) == (V{0, 1, 2, 3, 1000, 1001, 1002}));      // nothing but an append
    CHECK(edit(3, {2, 1, 0}, 0) == V{});                             // everything
    CHECK(edit(3, {0, 1, 2}, 2) == (V{1000, 1001}));                 // everything, then an append
    CHECK(edit(0, {}, 2) == (V{1000, 1001}));                        // onto the empty scene
    V every_other;
    std::vector<uint32_t> rem;
    for (uint32_t i = 0; i < 513; i++) { if (i & 1) every_other.push_back((int32_t)i); else rem.push_back(i); }
    CHECK(edit(513, rem, 0) == every_other);
}

static ErObjectTable table_of(const Scene& s, const std::vector<std::vector<uint32_t>>& objs) {
    std::vector<uint32_t> first{0}, ids;
    for (const auto& o : objs) { ids.insert(ids.end(), o.begin(), o.end()); first.push_back((uint32_t)ids.size()); }
    ErObjectTable t;
    std::string why;
    if (!er_objects_check(s.n, (uint32_t)objs.size(), first.data(), ids.data(), why)) { printf("table refused: %s\n", why.c_str()); failures++; }
    er_objects_take(t, (uint32_t)objs.size(), first.data(), ids.data(), s.v.data(), s.nn.data(), s.t.data());
    return t;
}

static std::vector<std::vector<uint32_t>> lists_of(const ErObjectTable& t) {
    std::vector<std::vector<uint32_t>> out;
    for (uint32_t o = 0; o < t.objects(); o++) out.emplace_back(t.ids.begin() + t.first[o], t.ids.begin() + t.first[o + 1]);
    return out;
}

static void test_objects() {
    using L = std::vector<std::vector<uint32_t>>;
    const Scene s(8), tail(2);
    const ErObjectTable t = table_of(s, {{6, 1}, {2, 3}, {}, {7, 0, 4}});      // triangle 5 is in no object
    std::vector<uint32_t> sorted;
    uint32_t nc = 0;
    std::string why;
    ErObjectTable out;
    {   // half of object 0, all of object 1, the first and the last id
        const std::vector<uint32_t> rem{7, 2, 3, 6, 0};
        const ErTopoList l = list_of(rem, &tail, 1);
        CHECK(er_topo_check(8, l, sorted, nc, why) && nc == 5);
        er_topo_remap_objects(t, 8, sorted, l, out);
        CHECK(lists_of(out) == (L{{0}, {}, {}, {1}, {3, 4}}));      // survivors 1 4 5 -> 0 1 2; the appended object last
        CHECK(out.rest_v.size() == 4 * 9 && out.rest_n.size() == 4 * 9 && out.rest_t.size() == 4 * 9);
        CHECK(out.rest_v[0] == s.v[1 * 9] && out.rest_v[9] == s.v[4 * 9] && out.rest_v[18] == tail.v[0] && out.rest_n[9 + 8] == s.nn[4 * 9 + 8] && out.rest_t[27 + 8] == tail.t[9 + 8]);
        CHECK(out.bound[0] == 106.0f && out.bound[1] == 107.0f && out.bound[2] == 108.0f);      // object 0: triangle 1 alone
        CHECK(out.bound[3] == 0.0f && out.bound[6] == 0.0f);                                     // the emptied objects
        CHECK(out.bound[12] == 106.0f && out.bound[14] == 108.0f);                               // the appended one: tail rows 0, 1
        CHECK(out.pending_count == 0 && out.pending.size() == 5 && out.last_m.size() == 5 * 12 && out.last_m[4 * 12] == 1.0f && out.last_m[4 * 12 + 5] == 1.0f && out.last_m[4 * 12 + 1] == 0.0f);
    }
    {   // nothing but an append, not as an object: the table keeps its lists
        const ErTopoList l = list_of({}, &tail, 0);
        CHECK(er_topo_check(8, l, sorted, nc, why) && nc == 10);
        er_topo_remap_objects(t, 8, sorted, l, out);
        CHECK(lists_of(out) == (L{{6, 1}, {2, 3}, {}, {7, 0, 4}}));
        CHECK(out.rest_v == t.rest_v && out.bound == t.bound && out.last_m == t.last_m);
    }
    {   // everything removed: four empty objects
        const std::vector<uint32_t> rem{0, 1, 2, 3, 4, 5, 6, 7};
        const ErTopoList l = list_of(rem, nullptr);
        CHECK(er_topo_check(8, l, sorted, nc, why) && nc == 0);
        er_topo_remap_objects(t, 8, sorted, l, out);
        CHECK(lists_of(out) == (L{{}, {}, {}, {}}) && out.rest_v.empty());
    }
    {   // no table: the flag is ignored, there is still no table
        const ErTopoList l = list_of({}, &tail, 1);
        CHECK(er_topo_check(8, l, sorted, nc, why));
        er_topo_remap_objects(ErObjectTable{}, 8, sorted, l, out);
        CHECK(out.objects() == 0 && out.ids.empty());
    }
    {   // the last matrix of a surviving object is kept
        ErObjectTable moved = t;
        moved.last_m[3 * 12 + 3] = 2.5f;
        const std::vector<uint32_t> rem{1};
        const ErTopoList l = list_of(rem, nullptr);
        CHECK(er_topo_check(8, l, sorted, nc, why));
        er_topo_remap_objects(moved, 8, sorted, l, out);
        CHECK(lists_of(out) == (L{{5}, {1, 2}, {}, {6, 0, 3}}) && out.last_m[3 * 12 + 3] == 2.5f);
    }
}

static int apply_from_stdin() {
    unsigned n = 0, r = 0, a = 0, as_object = 0, objects = 0;
    if (scanf("%u %u", &n, &r) != 2) return 2;
    std::vector<uint32_t> rem(r);
    for (auto& x : rem) if (scanf("%u", &x) != 1) return 2;
    if (scanf("%u %u %u", &a, &as_object, &objects) != 3) return 2;
    std::vector<std::vector<uint32_t>> objs(objects);
    for (auto& o : objs) {
        unsigned k = 0;
        if (scanf("%u", &k) != 1) return 2;
        o.resize(k);
        for (auto& x : o) if (scanf("%u", &x) != 1) return 2;
    }
    Scene s(n), tail(a);
    for (uint32_t j = 0; j < a; j++) tail.m[j] = -1 - (int32_t)j;
    const ErObjectTable t = table_of(s, objs);
    const ErTopoList l = list_of(rem, a ? &tail : nullptr, as_object);
    std::vector<uint32_t> sorted;
    uint32_t nc = 0;
    std::string why;
    if (!er_topo_check(n, l, sorted, nc, why)) { printf("refused: %s\n", why.c_str()); return 1; }
    ErObjectTable out;
    er_topo_remap_objects(t, n, sorted, l, out);
    const ErTopoArrays A = s.arrays();
    er_topo_reserve(A, nc);
    er_topo_apply(A, n, sorted, l);
    for (size_t i = 0; i < s.m.size(); i++) printf("%d ", s.m[i]);
    printf("\n");
    for (const auto& o : lists_of(out)) {
        for (uint32_t x : o) printf("%u ", x);
        printf("\n");
    }
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "apply") return apply_from_stdin();
    test_refusals();
    test_compaction();
    test_objects();
    if (failures) { printf("topology_patch: %d checks FAILED\n", failures); return 1; }
    printf("topology_patch ok\n");
    return 0;
}
