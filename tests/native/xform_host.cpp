// xform_host.cpp -- the host half of er_objects_set / er_render_transform (csrc/er_xform.h) alone: the checks of an object table and of
// a list of transforms, the matrix derivation, the overflow bound, and the lazy application of pending poses to the host copy, on heap
// arrays of exactly the sizes the contract names.  Built with -fsanitize=address,undefined by tests/test_transform_cpu.py: a read past
// an object's ids or a write past tri_count triangles of the copy is reported.
// Prints "xform_host ok" and returns 0, or says which expectation failed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>
#include <random>

#include "er_xform.h"

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); failures++; } } while (0)

struct Pose { uint32_t object; float m[12]; };      // ErObjectTransform's fields

static void identity(float* m) { for (int k = 0; k < 12; k++) m[k] = (k % 5 == 0) ? 1.0f : 0.0f; }

static bool objects_refused(uint32_t tri_count, uint32_t objects, const uint32_t* first, const uint32_t* ids, const char* word) {
    std::string why;
    if (er_objects_check(tri_count, objects, first, ids, why)) return false;
    if (why.find(word) == std::string::npos) { std::printf("   refused with \"%s\", expected \"%s\"\n", why.c_str(), word); return false; }
    return true;
}

static bool poses_refused(const ErObjectTable& t, uint32_t count, const Pose* x, const char* word) {
    std::string why;
    std::vector<ErXformEntry> entries;
    uint32_t moved = 0;
    if (er_xform_check(t, count, x, entries, moved, why)) return false;
    if (why.find(word) == std::string::npos) { std::printf("   refused with \"%s\", expected \"%s\"\n", why.c_str(), word); return false; }
    return true;
}

int main() {
    const uint32_t tri_count = 500;
    std::string why;
    // the scene's arrays: exactly tri_count triangles each
    std::unique_ptr<float[]> v(new float[(size_t)tri_count * 9]), n(new float[(size_t)tri_count * 9]), t(new float[(size_t)tri_count * 9]);
    std::mt19937 gen(3);
    std::normal_distribution<float> normal(0.0f, 1.0f);
    for (size_t i = 0; i < (size_t)tri_count * 9; i++) { v[i] = 3.0f * normal(gen); n[i] = normal(gen); t[i] = normal(gen); }

    // objects of 1, 63, 64, 65 and 0 triangles from a seeded permutation: non-contiguous ids, most triangles in no object
    std::vector<uint32_t> perm(tri_count);
    std::iota(perm.begin(), perm.end(), 0u);
    std::shuffle(perm.begin(), perm.end(), std::mt19937(9));
    const uint32_t objects = 5, total = 193;
    std::unique_ptr<uint32_t[]> first(new uint32_t[objects + 1]), ids(new uint32_t[total]);
    const uint32_t f[objects + 1] = {0, 1, 64, 128, 193, 193};
    std::copy(f, f + objects + 1, first.get());
    std::copy(perm.begin(), perm.begin() + total, ids.get());

    {   // the refusals of er_objects_set
        EXPECT(er_objects_check(tri_count, objects, first.get(), ids.get(), why));
        EXPECT(er_objects_check(tri_count, 0, nullptr, nullptr, why));      // clears: nothing is read
        EXPECT(objects_refused(tri_count, objects, nullptr, ids.get(), "without"));
        EXPECT(objects_refused(tri_count, objects, first.get(), nullptr, "without"));
        first[0] = 1;
        EXPECT(objects_refused(tri_count, objects, first.get(), ids.get(), "not 0"));
        first[0] = 0; first[2] = 0;
        EXPECT(objects_refused(tri_count, objects, first.get(), ids.get(), "decreases"));
        first[2] = 64;
        const uint32_t keep = ids[192];
        ids[192] = tri_count;
        EXPECT(objects_refused(tri_count, objects, first.get(), ids.get(), "not below tri_count"));
        ids[192] = ids[0];                                   // the first object's triangle again in the fourth
        EXPECT(objects_refused(tri_count, objects, first.get(), ids.get(), "listed twice"));
        ids[192] = ids[191];                                 // twice in one object
        EXPECT(objects_refused(tri_count, objects, first.get(), ids.get(), "listed twice"));
        ids[192] = keep;
        EXPECT(objects_refused(100, objects, first.get(), ids.get(), "more ids than triangles"));
        EXPECT(er_objects_check(tri_count, objects, first.get(), ids.get(), why));
    }

    ErObjectTable tab;
    er_objects_take(tab, objects, first.get(), ids.get(), v.get(), n.get(), t.get());
    EXPECT(tab.objects() == objects && tab.ids.size() == total && tab.rest_v.size() == (size_t)total * 9 && tab.pending_count == 0);
    {   // the rest copy and the bounds are the arrays' own
        bool same = true;
        float B[3] = {0, 0, 0};
        for (uint32_t j = 0; j < total; j++)
            for (int k = 0; k < 9; k++) {
                same = same && tab.rest_v[(size_t)j * 9 + k] == v[(size_t)ids[j] * 9 + k] && tab.rest_n[(size_t)j * 9 + k] == n[(size_t)ids[j] * 9 + k] &&
                       tab.rest_t[(size_t)j * 9 + k] == t[(size_t)ids[j] * 9 + k];
                if (j >= first[3] && j < first[4]) B[k % 3] = std::max(B[k % 3], std::fabs(v[(size_t)ids[j] * 9 + k]));
            }
        EXPECT(same);
        EXPECT(B[0] == tab.bound[9] && B[1] == tab.bound[10] && B[2] == tab.bound[11]);
        EXPECT(tab.bound[12] == 0 && tab.bound[13] == 0 && tab.bound[14] == 0);      // the empty object
    }

    {   // the matrix derivation
        float m[12], N[9], T[9];
        identity(m);
        EXPECT(er_xform_derive(m, N, T));
        for (int k = 0; k < 9; k++) EXPECT(N[k] == (k % 4 == 0 ? 1.0f : 0.0f) && T[k] == N[k]);
        m[0] = 2.0f; m[5] = 4.0f; m[10] = 8.0f;      // scale (2, 4, 8): cofactors (32, 16, 8) / 32, L / 8
        EXPECT(er_xform_derive(m, N, T));
        EXPECT(N[0] == 1.0f && N[4] == 0.5f && N[8] == 0.25f && T[0] == 0.25f && T[4] == 0.5f && T[8] == 1.0f);
        m[0] = -2.0f;                                 // a mirror
        EXPECT(!er_xform_derive(m, N, T));
        m[0] = 0.0f;                                  // singular
        EXPECT(!er_xform_derive(m, N, T));
        m[0] = 2.0f; m[7] = std::numeric_limits<float>::quiet_NaN();      // the translation is checked too
        EXPECT(!er_xform_derive(m, N, T));
        m[7] = std::numeric_limits<float>::infinity();
        EXPECT(!er_xform_derive(m, N, T));
        identity(m);
        for (int k = 0; k < 3; k++) m[5 * k] = 1e-20f;      // tiny and huge uniform scales keep N and T at the identity
        EXPECT(er_xform_derive(m, N, T) && N[0] == 1.0f && N[4] == 1.0f && N[8] == 1.0f && T[0] == 1.0f && N[1] == 0.0f);
        for (int k = 0; k < 3; k++) m[5 * k] = 1e15f;
        EXPECT(er_xform_derive(m, N, T) && N[0] == 1.0f && N[4] == 1.0f && N[8] == 1.0f && T[8] == 1.0f);
    }

    {   // the overflow bound: just inside, just beyond
        const float B[3] = {2.0f, 3.0f, 5.0f};
        float m[12];
        identity(m);
        m[0] = 0.49e37f;                              // row 0: 0.49e37 * 2 = 0.98e37
        EXPECT(er_xform_bound_ok(m, B));
        m[3] = 0.01e37f;                              // + 0.01e37: 0.99e37
        EXPECT(er_xform_bound_ok(m, B));
        m[3] = 0.03e37f;                              // 1.01e37
        EXPECT(!er_xform_bound_ok(m, B));
        m[3] = -0.03e37f;                             // magnitudes count
        EXPECT(!er_xform_bound_ok(m, B));
        identity(m);
        m[11] = 1.1e37f;                              // the last row's translation alone
        EXPECT(!er_xform_bound_ok(m, B));
    }

    {   // the refusals of er_render_transform's list
        std::unique_ptr<Pose[]> x(new Pose[2]);
        x[0].object = 3; identity(x[0].m);
        x[1].object = 0; identity(x[1].m);
        std::vector<ErXformEntry> entries;
        uint32_t moved = 0;
        EXPECT(er_xform_check(tab, 2, x.get(), entries, moved, why));
        EXPECT(moved == 66 && entries.size() == 2 && entries[0].object == 3 && entries[0].start == 0 && entries[1].object == 0 && entries[1].start == 65);
        EXPECT(poses_refused(tab, 0, x.get(), "count 0"));
        EXPECT(poses_refused(tab, 2, (const Pose*)nullptr, "without"));
        x[1].object = objects;
        EXPECT(poses_refused(tab, 2, x.get(), "not below the object count"));
        x[1].object = 3;
        EXPECT(poses_refused(tab, 2, x.get(), "listed twice"));
        x[1].object = 0;
        x[1].m[6] = std::numeric_limits<float>::quiet_NaN();
        EXPECT(poses_refused(tab, 2, x.get(), "not finite"));
        x[1].m[6] = 0.0f; x[1].m[0] = -1.0f;
        EXPECT(poses_refused(tab, 2, x.get(), "det(L)"));
        x[1].m[0] = 1.0f; x[1].m[3] = 2e37f;
        EXPECT(poses_refused(tab, 2, x.get(), "float range"));
        x[1].m[3] = 0.0f;
        x[0].object = 4;                              // the empty object alone moves nothing
        EXPECT(poses_refused(tab, 1, x.get(), "no triangle"));
        std::unique_ptr<Pose[]> many(new Pose[objects + 1]);
        for (uint32_t i = 0; i <= objects; i++) { many[i].object = i % objects; identity(many[i].m); }
        EXPECT(poses_refused(tab, objects + 1, many.get(), "twice"));
    }

    {   // mark, then the lazy application: only the marked objects' triangles change, and they become pose(rest, m)
        std::unique_ptr<Pose[]> x(new Pose[2]);
        x[0].object = 2; identity(x[0].m);
        x[0].m[0] = 0.0f; x[0].m[1] = -2.0f; x[0].m[4] = 3.0f; x[0].m[5] = 0.0f; x[0].m[3] = 7.0f; x[0].m[11] = -1.0f;      // a turn about z with scales, and a shift
        x[1].object = 0; identity(x[1].m);
        x[1].m[7] = 100.0f;
        std::vector<ErXformEntry> entries;
        uint32_t moved = 0;
        EXPECT(er_xform_check(tab, 2, x.get(), entries, moved, why));
        std::unique_ptr<float[]> v0(new float[(size_t)tri_count * 9]), n0(new float[(size_t)tri_count * 9]), t0(new float[(size_t)tri_count * 9]);
        std::memcpy(v0.get(), v.get(), (size_t)tri_count * 36); std::memcpy(n0.get(), n.get(), (size_t)tri_count * 36); std::memcpy(t0.get(), t.get(), (size_t)tri_count * 36);
        er_objects_mark(tab, entries.data(), (uint32_t)entries.size());
        EXPECT(tab.pending_count == 2 && tab.pending[2] && tab.pending[0] && !tab.pending[1]);
        EXPECT(std::memcmp(v0.get(), v.get(), (size_t)tri_count * 36) == 0);      // marking touches no triangle
        er_objects_mark(tab, entries.data(), 1);                                   // the same object again: counted once
        EXPECT(tab.pending_count == 2);
        er_objects_flush(tab, v.get(), n.get(), t.get());
        EXPECT(tab.pending_count == 0 && !tab.pending[2] && !tab.pending[0]);
        std::vector<int> owner(tri_count, -1);
        for (uint32_t o = 0; o < objects; o++) for (uint32_t j = first[o]; j < first[o + 1]; j++) owner[ids[j]] = (int)o;
        bool ok = true;
        for (uint32_t id = 0; id < tri_count && ok; id++) {
            const size_t at = (size_t)id * 9;
            const int e = owner[id] == 2 ? 0 : owner[id] == 0 ? 1 : -1;
            if (e < 0) {
                ok = std::memcmp(&v[at], &v0[at], 36) == 0 && std::memcmp(&n[at], &n0[at], 36) == 0 && std::memcmp(&t[at], &t0[at], 36) == 0;
                continue;
            }
            float ev[9], en[9], et[9];
            er_xform_triangle(entries[e].m, entries[e].N, entries[e].T, &v0[at], &n0[at], &t0[at], ev, en, et);
            ok = std::memcmp(&v[at], ev, 36) == 0 && std::memcmp(&n[at], en, 36) == 0 && std::memcmp(&t[at], et, 36) == 0;
            for (int k = 0; k < 9 && ok; k += 3) {      // directions come out unit (these rest normals are not zero)
                const double len = std::sqrt((double)n[at + k] * n[at + k] + (double)n[at + k + 1] * n[at + k + 1] + (double)n[at + k + 2] * n[at + k + 2]);
                ok = std::fabs(len - 1.0) < 1e-6;
            }
        }
        EXPECT(ok);
        // a second flush finds nothing; a pose of the same object again is absolute: from the REST copy, not from the arrays as they are
        std::unique_ptr<float[]> v1(new float[(size_t)tri_count * 9]);
        std::memcpy(v1.get(), v.get(), (size_t)tri_count * 36);
        er_objects_flush(tab, v.get(), n.get(), t.get());
        EXPECT(std::memcmp(v1.get(), v.get(), (size_t)tri_count * 36) == 0);
        identity(x[0].m);
        EXPECT(er_xform_check(tab, 1, x.get(), entries, moved, why));
        er_objects_mark(tab, entries.data(), 1);
        er_objects_flush(tab, v.get(), n.get(), t.get());
        bool back = true;
        for (uint32_t j = first[2]; j < first[3]; j++) back = back && std::memcmp(&v[(size_t)ids[j] * 9], &v0[(size_t)ids[j] * 9], 36) == 0;
        EXPECT(back);                                  // pose(rest, identity) reproduces the vertices
        // forget_pending: marks dropped, arrays untouched
        er_objects_mark(tab, entries.data(), 1);
        tab.forget_pending();
        std::memcpy(v1.get(), v.get(), (size_t)tri_count * 36);
        er_objects_flush(tab, v.get(), n.get(), t.get());
        EXPECT(tab.pending_count == 0 && std::memcmp(v1.get(), v.get(), (size_t)tri_count * 36) == 0);
    }

    {   // er_xform_apply on arrays of exactly count triangles; zero normals stay zero; a refused matrix writes nothing
        const uint32_t count = 7;
        std::unique_ptr<float[]> rv(new float[count * 9]), rn(new float[count * 9]), rt(new float[count * 9]), ov(new float[count * 9]), on(new float[count * 9]), ot(new float[count * 9]);
        for (uint32_t i = 0; i < count * 9; i++) { rv[i] = (float)i; rn[i] = i < 9 ? 0.0f : 1.0f + (float)i; rt[i] = 1e20f; ov[i] = on[i] = ot[i] = -7.0f; }
        float m[12];
        identity(m);
        m[0] = -1.0f;
        EXPECT(!er_xform_apply(m, count, rv.get(), rn.get(), rt.get(), ov.get(), on.get(), ot.get()) && ov[0] == -7.0f && ot[count * 9 - 1] == -7.0f);
        m[0] = 1.0f; m[3] = 0.5f;
        EXPECT(er_xform_apply(m, count, rv.get(), rn.get(), rt.get(), ov.get(), on.get(), ot.get()));
        EXPECT(ov[0] == 0.5f && ov[1] == 1.0f && ov[count * 9 - 1] == (float)(count * 9 - 1));
        for (int k = 0; k < 9; k++) EXPECT(on[k] == 0.0f);
        EXPECT(er_xform_apply(m, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    }

    {   // an empty table, and a table replaced by a smaller one
        ErObjectTable none;
        er_objects_take(none, 0, nullptr, nullptr, v.get(), n.get(), t.get());
        EXPECT(none.objects() == 0);
        Pose p; p.object = 0; identity(p.m);
        EXPECT(poses_refused(none, 1, &p, "not below the object count"));
        const uint32_t f1[2] = {0, 2};
        er_objects_take(tab, 1, f1, ids.get(), v.get(), n.get(), t.get());
        EXPECT(tab.objects() == 1 && tab.ids.size() == 2 && tab.pending.size() == 1 && tab.last_m.size() == 12);
        er_objects_take(tab, 0, nullptr, nullptr, v.get(), n.get(), t.get());
        EXPECT(tab.objects() == 0 && tab.ids.empty());
    }

    if (failures) return 1;
    std::printf("xform_host ok\n");
    return 0;
}
