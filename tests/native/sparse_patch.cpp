// sparse_patch.cpp -- the host half of er_render_update_sparse (csrc/er_sparse_host.h) alone: the checks of the listed triangles and the
// patch of the host copy, on heap arrays of exactly the sizes the contract names.  Built with -fsanitize=address,undefined by
// tests/test_update_sparse_cpu.py: a read past `count` entries of a list or a write past tri_count triangles of the copy is reported.
// Prints "sparse_patch ok" and returns 0, or says which expectation failed.
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>
#include <numeric>
#include <random>

#include "er_sparse_host.h"

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); failures++; } } while (0)

struct List {      // heap storage of exactly count entries each
    std::unique_ptr<uint32_t[]> ids;
    std::unique_ptr<float[]> v, n, t;
    ErSparseList l;
    List(uint32_t count, bool normals, bool tangents) : ids(new uint32_t[count]), v(new float[(size_t)count * 9]) {
        l.count = count; l.tri_ids = ids.get(); l.vertices = v.get();
        if (normals) { n.reset(new float[(size_t)count * 9]); l.normals = n.get(); }
        if (tangents) { t.reset(new float[(size_t)count * 9]); l.tangents = t.get(); }
        for (size_t i = 0; i < (size_t)count * 9; i++) { v[i] = 1000.0f + (float)i; if (normals) n[i] = 2000.0f + (float)i; if (tangents) t[i] = 3000.0f + (float)i; }
    }
};

static bool refused(uint32_t tri_count, const ErSparseList& l, const char* word) {
    std::string why;
    if (er_sparse_check(tri_count, l, why)) return false;
    if (why.find(word) == std::string::npos) { std::printf("   refused with \"%s\", expected \"%s\"\n", why.c_str(), word); return false; }
    return true;
}

int main() {
    const uint32_t tri_count = 1000;
    std::string why;
    {   // the refusals of include/eleven_hip.h
        List a(4, true, true);
        uint32_t good[4] = {999, 0, 17, 500};
        std::copy(good, good + 4, a.ids.get());
        EXPECT(er_sparse_check(tri_count, a.l, why));
        ErSparseList l = a.l;
        l.count = 0;
        EXPECT(refused(tri_count, l, "count 0"));
        l = a.l; l.tri_ids = nullptr;
        EXPECT(refused(tri_count, l, "without"));
        l = a.l; l.vertices = nullptr;
        EXPECT(refused(tri_count, l, "without"));
        a.ids[3] = tri_count;
        EXPECT(refused(tri_count, a.l, "not below tri_count"));
        a.ids[3] = 0xffffffffu;
        EXPECT(refused(tri_count, a.l, "not below tri_count"));
        a.ids[3] = 999;                                  // first and last entry equal: the sort finds what a neighbour scan would not
        EXPECT(refused(tri_count, a.l, "listed twice"));
        a.ids[3] = 500;
        a.v[35] = std::numeric_limits<float>::quiet_NaN();      // the last float of the list
        EXPECT(refused(tri_count, a.l, "not finite"));
        a.v[35] = 1.0f; a.v[0] = -std::numeric_limits<float>::infinity();
        EXPECT(refused(tri_count, a.l, "not finite"));
        a.v[0] = 1.0f;
        EXPECT(er_sparse_check(tri_count, a.l, why));
        EXPECT(refused(0, a.l, "not below tri_count"));  // a scene without triangles takes no list
        List big(5, false, false);                       // more ids than triangles: refused before anything of that size is allocated
        for (uint32_t i = 0; i < 5; i++) big.ids[i] = i % 4;
        EXPECT(refused(4, big.l, "twice"));
    }
    for (int pass = 0; pass < 3; pass++) {   // the patch: every id in a seeded permutation, with and without normals / tangents
        const bool nrm = pass >= 1, tan = pass >= 2;
        const uint32_t count = pass == 0 ? tri_count : 137;
        std::vector<uint32_t> perm(tri_count);
        std::iota(perm.begin(), perm.end(), 0u);
        std::shuffle(perm.begin(), perm.end(), std::mt19937(7 + pass));
        List a(count, nrm, tan);
        std::copy(perm.begin(), perm.begin() + count, a.ids.get());
        EXPECT(er_sparse_check(tri_count, a.l, why));
        std::unique_ptr<float[]> v(new float[(size_t)tri_count * 9]), n(new float[(size_t)tri_count * 9]), t(new float[(size_t)tri_count * 9]);
        for (size_t i = 0; i < (size_t)tri_count * 9; i++) { v[i] = -1.0f - (float)i; n[i] = -2.0f - (float)i; t[i] = -3.0f - (float)i; }
        er_sparse_patch(a.l, v.get(), n.get(), t.get());
        std::vector<int> where(tri_count, -1);
        for (uint32_t i = 0; i < count; i++) where[a.ids[i]] = (int)i;
        bool ok = true;
        for (uint32_t id = 0; id < tri_count && ok; id++)
            for (int k = 0; k < 9 && ok; k++) {
                const size_t at = (size_t)id * 9 + k;
                const int w = where[id];
                const size_t from = w < 0 ? 0 : (size_t)w * 9 + k;
                ok = v[at] == (w < 0 ? -1.0f - (float)at : a.v[from]) && n[at] == (w < 0 || !nrm ? -2.0f - (float)at : a.n[from]) &&
                     t[at] == (w < 0 || !tan ? -3.0f - (float)at : a.t[from]);
            }
        EXPECT(ok);
    }
    if (failures) return 1;
    std::printf("sparse_patch ok\n");
    return 0;
}
