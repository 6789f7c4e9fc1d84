// skin_host.cpp -- the host half of er_skin_set / er_render_skin (csrc/er_skin.h) alone: the checks of a skin and of a list of palettes,
// the bound on linear entries, mark and the lazy application of BOTH kinds of pending pose to the host copy -- with the interleaving
// transform -> skin -> transform on one object -- and the drop of every skin when the table changes, on heap arrays of exactly the sizes
// the contract names.  Built with -fsanitize=address,undefined by tests/test_skin_cpu.py: a read past an object's influences or past a
// palette, or a write past tri_count triangles of the copy, is reported.
// Prints "skin_host ok" and returns 0, or says which expectation failed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>
#include <random>

#include "er_skin.h"

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); failures++; } } while (0)

struct Skin { uint32_t object, bone_count; const uint16_t* bones; const float* weights; };      // ErSkin's fields
struct Pose { uint32_t object, bone_count; const float* palette; };                             // ErSkinPose's
struct Matrix { uint32_t object; float m[12]; };                                                // ErObjectTransform's

static void identity(float* m) { for (int k = 0; k < 12; k++) m[k] = (k % 5 == 0) ? 1.0f : 0.0f; }

static bool skin_refused(const ErObjectTable& t, const Skin& k, const char* word) {
    std::string why;
    if (er_skin_check(t, k, why)) return false;
    if (why.find(word) == std::string::npos) { std::printf("   refused with \"%s\", expected \"%s\"\n", why.c_str(), word); return false; }
    return true;
}

static bool poses_refused(const ErObjectTable& t, const ErSkinTable& K, uint32_t count, const Pose* p, int code, const char* word) {
    std::string why;
    std::vector<ErSkinEntry> entries;
    std::vector<float> palette;
    uint32_t moved = 0;
    const int rc = er_skin_pose_check(t, K, count, p, entries, palette, moved, why);
    if (rc != code) { std::printf("   returned %d (\"%s\"), expected %d\n", rc, why.c_str(), code); return false; }
    if (why.find(word) == std::string::npos) { std::printf("   refused with \"%s\", expected \"%s\"\n", why.c_str(), word); return false; }
    return true;
}

int main() {
    const uint32_t tri_count = 400;
    std::string why;
    std::unique_ptr<float[]> v(new float[(size_t)tri_count * 9]), n(new float[(size_t)tri_count * 9]), t(new float[(size_t)tri_count * 9]);
    std::mt19937 gen(5);
    std::normal_distribution<float> normal(0.0f, 1.0f);
    for (size_t i = 0; i < (size_t)tri_count * 9; i++) { v[i] = 3.0f * normal(gen); n[i] = normal(gen); t[i] = normal(gen); }

    // objects of 1, 63, 65 and 0 triangles from a seeded permutation
    std::vector<uint32_t> perm(tri_count);
    std::iota(perm.begin(), perm.end(), 0u);
    std::shuffle(perm.begin(), perm.end(), std::mt19937(11));
    const uint32_t objects = 4, total = 129;
    const uint32_t first[objects + 1] = {0, 1, 64, 129, 129};
    std::unique_ptr<uint32_t[]> ids(new uint32_t[total]);
    std::copy(perm.begin(), perm.begin() + total, ids.get());
    ErObjectTable tab;
    er_objects_take(tab, objects, first, ids.get(), v.get(), n.get(), t.get());
    ErSkinTable K;
    EXPECT(K.skinned == 0 && K.rows() == 0 && !K.has(0));

    // influences of object 2 (65 triangles, 5 bones) and object 1 (63 triangles, 2 bones): exactly size x 12 entries each
    const uint32_t bones2 = 5, bones1 = 2;
    std::unique_ptr<uint16_t[]> b2(new uint16_t[65 * 12]), b1(new uint16_t[63 * 12]);
    std::unique_ptr<float[]> w2(new float[65 * 12]), w1(new float[63 * 12]);
    std::uniform_real_distribution<float> unit(0.0f, 1.0f);
    for (int i = 0; i < 65 * 12; i++) { b2[i] = (uint16_t)(gen() % bones2); w2[i] = (i % 4) <= (i / 4) % 4 ? unit(gen) * 0.5f : 0.0f; }      // 1 to 4 non-zero weights, not summing to 1
    for (int i = 0; i < 63 * 12; i++) { b1[i] = (uint16_t)(gen() % bones1); w1[i] = i % 4 == 0 ? 1.0f : 0.0f; }

    {   // the refusals of er_skin_set, and what passes
        Skin k{2, bones2, b2.get(), w2.get()};
        EXPECT(er_skin_check(tab, k, why));
        k.object = objects;
        EXPECT(skin_refused(tab, k, "not below the object count"));
        k.object = 3;
        EXPECT(skin_refused(tab, k, "holds no triangle"));
        k.object = 2; k.bone_count = ER_SKIN_BONES_MAX + 1;
        EXPECT(skin_refused(tab, k, "bone_count"));
        k.bone_count = bones2;
        const uint16_t keep_b = b2[65 * 12 - 1];
        const float keep_w = w2[65 * 12 - 1];
        b2[65 * 12 - 1] = bones2; w2[65 * 12 - 1] = 0.0f;      // a bone index out of range counts also under a weight of 0
        EXPECT(skin_refused(tab, k, "not below bone_count"));
        b2[65 * 12 - 1] = keep_b;
        w2[65 * 12 - 1] = std::numeric_limits<float>::quiet_NaN();
        EXPECT(skin_refused(tab, k, "[0, 1]"));
        w2[65 * 12 - 1] = std::numeric_limits<float>::infinity();
        EXPECT(skin_refused(tab, k, "[0, 1]"));
        w2[65 * 12 - 1] = -0.25f;
        EXPECT(skin_refused(tab, k, "[0, 1]"));
        w2[65 * 12 - 1] = 1.0f + 1e-6f;
        EXPECT(skin_refused(tab, k, "[0, 1]"));
        w2[65 * 12 - 1] = keep_w;
        k.bones = nullptr;
        EXPECT(skin_refused(tab, k, "without"));
        k.bone_count = 0;                                       // removal reads neither array
        EXPECT(er_skin_check(tab, k, why));
        k = Skin{2, ER_SKIN_BONES_MAX, b2.get(), w2.get()};     // the maximum itself is legal
        EXPECT(er_skin_check(tab, k, why));
    }

    er_skin_take(K, tab, Skin{2, bones2, b2.get(), w2.get()});
    EXPECT(K.skinned == 1 && K.has(2) && !K.has(1) && K.rows() == 65 && K.row_first[2] == 0 && K.rec[2].palette.size() == bones2 * 12 && K.rec[2].bones.size() == 65 * 12);
    er_skin_take(K, tab, Skin{1, bones1, b1.get(), w1.get()});
    EXPECT(K.skinned == 2 && K.rows() == 128 && K.row_first[1] == 0 && K.row_first[2] == 63);
    er_skin_take(K, tab, Skin{0, 0, nullptr, nullptr});        // removing what is not there changes nothing
    EXPECT(K.skinned == 2);

    // palettes: rotations about z with non-uniform scales and shifts
    std::unique_ptr<float[]> P2(new float[bones2 * 12]), P1(new float[bones1 * 12]);
    for (uint32_t b = 0; b < bones2; b++) {
        float* m = &P2[b * 12];
        const float a = 0.3f + 0.5f * (float)b, c = std::cos(a), s = std::sin(a);
        const float M[12] = {1.5f * c, -0.7f * s, 0, 0.1f * (float)b, 1.5f * s, 0.7f * c, 0, -0.2f, 0, 0, 1.0f + 0.25f * (float)b, 0.05f};
        std::copy(M, M + 12, m);
    }
    for (uint32_t b = 0; b < bones1; b++) { identity(&P1[b * 12]); P1[b * 12 + 3] = 2.0f + (float)b; }

    {   // the refusals of er_render_skin's list
        std::unique_ptr<Pose[]> p(new Pose[2]);
        p[0] = Pose{2, bones2, P2.get()};
        p[1] = Pose{1, bones1, P1.get()};
        std::vector<ErSkinEntry> entries;
        std::vector<float> palette;
        uint32_t moved = 0;
        EXPECT(er_skin_pose_check(tab, K, 2, p.get(), entries, palette, moved, why) == 0);
        EXPECT(moved == 128 && entries.size() == 2 && palette.size() == (bones2 + bones1) * 12);
        EXPECT(entries[0].object == 2 && entries[0].start == 0 && entries[0].row == 63 && entries[0].pal == 0 && entries[0].bones == bones2);
        EXPECT(entries[1].object == 1 && entries[1].start == 65 && entries[1].row == 0 && entries[1].pal == bones2 && entries[1].bones == bones1);
        EXPECT(std::memcmp(&palette[bones2 * 12], P1.get(), bones1 * 48) == 0);
        EXPECT(poses_refused(tab, K, 0, p.get(), 1, "count 0"));
        EXPECT(poses_refused(tab, K, 2, (const Pose*)nullptr, 1, "without"));
        p[1].object = objects;
        EXPECT(poses_refused(tab, K, 2, p.get(), 1, "not below the object count"));
        p[1].object = 2;
        EXPECT(poses_refused(tab, K, 2, p.get(), 1, "listed twice"));
        p[1].object = 0;                                       // an object without a skin: a state error
        EXPECT(poses_refused(tab, K, 2, p.get(), 2, "no skin"));
        p[1].object = 1; p[1].bone_count = bones1 + 1;
        EXPECT(poses_refused(tab, K, 2, p.get(), 1, "bone_count"));
        p[1].bone_count = bones1; p[1].palette = nullptr;
        EXPECT(poses_refused(tab, K, 2, p.get(), 1, "without a palette"));
        p[1].palette = P1.get();
        const float keep = P1[12 + 6];
        P1[12 + 6] = std::numeric_limits<float>::quiet_NaN();   // the LAST bone is read too
        EXPECT(poses_refused(tab, K, 2, p.get(), 1, "not finite"));
        P1[12 + 6] = keep; P1[12] = -1.0f;
        EXPECT(poses_refused(tab, K, 2, p.get(), 1, "det(L)"));
        P1[12] = 1.0f; P1[12 + 3] = 2e37f;
        EXPECT(poses_refused(tab, K, 2, p.get(), 1, "float range"));
        P1[12 + 3] = 3.0f;
        P1[12] = ER_SKIN_MAX_LINEAR;                            // the bound on linear entries: at it, just beyond it
        EXPECT(er_skin_pose_check(tab, K, 2, p.get(), entries, palette, moved, why) == 0);
        P1[12] = std::nextafter(ER_SKIN_MAX_LINEAR, 1e30f);
        EXPECT(poses_refused(tab, K, 2, p.get(), 1, "linear entry"));
        P1[12] = 1.0f; P1[12 + 1] = -2.0f * ER_SKIN_MAX_LINEAR; // magnitudes count (det stays 1)
        EXPECT(poses_refused(tab, K, 2, p.get(), 1, "linear entry"));
        P1[12 + 1] = 0.0f;
        EXPECT(er_skin_pose_check(tab, K, 2, p.get(), entries, palette, moved, why) == 0);
    }

    {   // at the bound every intermediate of a corner stays finite: four bones of 2^14 everywhere it may be, weights of 1
        float P[12];
        for (int k = 0; k < 12; k++) P[k] = (k % 4 == 3) ? 0.0f : ((k % 5 == 0) ? ER_SKIN_MAX_LINEAR : -ER_SKIN_MAX_LINEAR);
        const uint32_t b[4] = {0, 0, 0, 0};
        const float w[4] = {1, 1, 1, 1}, x[3] = {1, 1, 1}, d[3] = {1e8f, -1e8f, 1e8f};
        float M[12], L[9], C[9], ox[3], on[3], ot[3];
        er_skin_blend(P, b, w, M);
        er_skin_linear(M, L, C);
        bool finite = true;
        for (int k = 0; k < 9; k++) finite = finite && std::isfinite(C[k]) && std::fabs(L[k]) == 4.0f * ER_SKIN_MAX_LINEAR;
        EXPECT(finite);
        er_skin_corner(P, b, w, x, d, d, ox, on, ot);
        for (int k = 0; k < 3; k++) EXPECT(std::isfinite(ox[k]) && std::isfinite(on[k]) && std::isfinite(ot[k]));
    }

    // what the host copy should become, from the arrays as they are now
    std::unique_ptr<float[]> v0(new float[(size_t)tri_count * 9]), n0(new float[(size_t)tri_count * 9]), t0(new float[(size_t)tri_count * 9]);
    std::memcpy(v0.get(), v.get(), (size_t)tri_count * 36); std::memcpy(n0.get(), n.get(), (size_t)tri_count * 36); std::memcpy(t0.get(), t.get(), (size_t)tri_count * 36);
    auto object_is = [&](uint32_t o, const float* ev, const float* en, const float* et) {      // [size][9] expectations against the copy
        bool ok = true;
        for (uint32_t j = first[o]; j < first[o + 1] && ok; j++) {
            const size_t at = (size_t)ids[j] * 9, from = (size_t)(j - first[o]) * 9;
            ok = std::memcmp(&v[at], ev + from, 36) == 0 && std::memcmp(&n[at], en + from, 36) == 0 && std::memcmp(&t[at], et + from, 36) == 0;
        }
        return ok;
    };
    auto others_untouched = [&](uint32_t a, uint32_t b) {
        std::vector<int> owner(tri_count, -1);
        for (uint32_t o = 0; o < objects; o++) for (uint32_t j = first[o]; j < first[o + 1]; j++) owner[ids[j]] = (int)o;
        bool ok = true;
        for (uint32_t id = 0; id < tri_count && ok; id++)
            if (owner[id] != (int)a && owner[id] != (int)b) ok = std::memcmp(&v[(size_t)id * 9], &v0[(size_t)id * 9], 36) == 0 && std::memcmp(&n[(size_t)id * 9], &n0[(size_t)id * 9], 36) == 0;
        return ok;
    };
    std::vector<float> ev(65 * 9), en(65 * 9), et(65 * 9);
    auto skinned2 = [&](const float* P) {
        for (uint32_t i = 0; i < 65; i++) {
            const size_t at = (size_t)ids[first[2] + i] * 9;
            er_skin_triangle(P, &b2[i * 12], &w2[i * 12], &v0[at], &n0[at], &t0[at], &ev[i * 9], &en[i * 9], &et[i * 9]);
        }
    };
    auto matrixed2 = [&](const float* m) {
        float N[9], T[9];
        EXPECT(er_xform_derive(m, N, T));
        for (uint32_t i = 0; i < 65; i++) {
            const size_t at = (size_t)ids[first[2] + i] * 9;
            er_xform_triangle(m, N, T, &v0[at], &n0[at], &t0[at], &ev[i * 9], &en[i * 9], &et[i * 9]);
        }
    };

    {   // transform -> skin -> transform on object 2, flushed after each and flushed once at the end: the LAST call wins, from the rest copy
        std::vector<ErSkinEntry> entries;
        std::vector<float> palette;
        std::vector<ErXformEntry> xe;
        uint32_t moved = 0;
        Pose p{2, bones2, P2.get()};
        Matrix m1, m2;
        m1.object = m2.object = 2;
        identity(m1.m); m1.m[0] = 2.0f; m1.m[7] = 5.0f;
        identity(m2.m); m2.m[5] = 0.5f; m2.m[11] = -3.0f;
        for (int lazy = 0; lazy < 2; lazy++) {
            EXPECT(er_xform_check(tab, 1, &m1, xe, moved, why));
            er_objects_mark(tab, xe.data(), 1);
            EXPECT(!er_skin_mark_matrix(K, xe.data(), 1));                 // it lay in a matrix pose (or none)
            if (!lazy) { er_skin_flush(tab, K, v.get(), n.get(), t.get()); matrixed2(m1.m); EXPECT(object_is(2, ev.data(), en.data(), et.data())); }
            EXPECT(er_skin_pose_check(tab, K, 1, &p, entries, palette, moved, why) == 0 && moved == 65);
            er_skin_mark(tab, K, entries.data(), 1, palette.data());
            EXPECT(tab.pending_count == 1 && tab.pending[2] && K.kind[2] == 1);
            er_skin_mark(tab, K, entries.data(), 1, palette.data());       // the same object again: counted once
            EXPECT(tab.pending_count == 1);
            if (!lazy) { er_skin_flush(tab, K, v.get(), n.get(), t.get()); skinned2(P2.get()); EXPECT(object_is(2, ev.data(), en.data(), et.data()) && tab.pending_count == 0); }
            EXPECT(er_xform_check(tab, 1, &m2, xe, moved, why));
            er_objects_mark(tab, xe.data(), 1);
            EXPECT(er_skin_mark_matrix(K, xe.data(), 1) && K.kind[2] == 0);  // it lay in a palette pose
            er_skin_flush(tab, K, v.get(), n.get(), t.get());
            matrixed2(m2.m);
            EXPECT(object_is(2, ev.data(), en.data(), et.data()) && tab.pending_count == 0 && !tab.pending[2]);
            EXPECT(others_untouched(2, 2));
        }
        // ... and a skin as the last word, with a matrix pending on ANOTHER object in the same flush
        Matrix m3;
        m3.object = 0;
        identity(m3.m); m3.m[3] = 9.0f;
        EXPECT(er_xform_check(tab, 1, &m3, xe, moved, why));
        er_objects_mark(tab, xe.data(), 1);
        er_skin_mark_matrix(K, xe.data(), 1);
        EXPECT(er_skin_pose_check(tab, K, 1, &p, entries, palette, moved, why) == 0);
        er_skin_mark(tab, K, entries.data(), 1, palette.data());
        EXPECT(tab.pending_count == 2);
        std::vector<float> before(v.get(), v.get() + (size_t)tri_count * 9);
        EXPECT(std::memcmp(before.data(), v.get(), (size_t)tri_count * 36) == 0);      // marking touches no triangle
        er_skin_flush(tab, K, v.get(), n.get(), t.get());
        skinned2(P2.get());
        EXPECT(object_is(2, ev.data(), en.data(), et.data()) && tab.pending_count == 0);
        EXPECT(v[(size_t)ids[0] * 9] == v0[(size_t)ids[0] * 9] + 9.0f && others_untouched(2, 0));
        // directions come out unit (these rest normals are not zero)
        bool unit_ok = true;
        for (size_t k = 0; k < en.size(); k += 3) unit_ok = unit_ok && std::fabs(std::sqrt((double)en[k] * en[k] + (double)en[k + 1] * en[k + 1] + (double)en[k + 2] * en[k + 2]) - 1.0) < 1e-6;
        EXPECT(unit_ok);
        // a second flush finds nothing
        std::vector<float> again(v.get(), v.get() + (size_t)tri_count * 9);
        er_skin_flush(tab, K, v.get(), n.get(), t.get());
        EXPECT(std::memcmp(again.data(), v.get(), (size_t)tri_count * 36) == 0);
    }

    {   // identities with one weight of 1 reproduce the rest vertices bit for bit (object 1's skin)
        std::vector<ErSkinEntry> entries;
        std::vector<float> palette;
        uint32_t moved = 0;
        for (uint32_t b = 0; b < bones1; b++) identity(&P1[b * 12]);
        Pose p{1, bones1, P1.get()};
        EXPECT(er_skin_pose_check(tab, K, 1, &p, entries, palette, moved, why) == 0 && moved == 63);
        er_skin_mark(tab, K, entries.data(), 1, palette.data());
        er_skin_flush(tab, K, v.get(), n.get(), t.get());
        bool same = true;
        for (uint32_t j = first[1]; j < first[2]; j++) same = same && std::memcmp(&v[(size_t)ids[j] * 9], &v0[(size_t)ids[j] * 9], 36) == 0;
        EXPECT(same);
    }

    {   // a skin replaced and removed; forget_pending with a palette pose pending; the drop on a table change
        er_skin_take(K, tab, Skin{1, 0, nullptr, nullptr});
        EXPECT(K.skinned == 1 && !K.has(1) && K.rows() == 65 && K.row_first[2] == 0);
        Pose p{1, bones1, P1.get()};
        EXPECT(poses_refused(tab, K, 1, &p, 2, "no skin"));
        std::vector<ErSkinEntry> entries;
        std::vector<float> palette;
        uint32_t moved = 0;
        Pose p2{2, bones2, P2.get()};
        EXPECT(er_skin_pose_check(tab, K, 1, &p2, entries, palette, moved, why) == 0 && entries[0].row == 0);
        er_skin_mark(tab, K, entries.data(), 1, palette.data());
        tab.forget_pending();                                   // (the arrays were replaced whole)
        std::vector<float> keep(v.get(), v.get() + (size_t)tri_count * 9);
        er_skin_flush(tab, K, v.get(), n.get(), t.get());
        EXPECT(tab.pending_count == 0 && std::memcmp(keep.data(), v.get(), (size_t)tri_count * 36) == 0);
        er_skin_mark(tab, K, entries.data(), 1, palette.data());
        er_skin_flush(tab, K, v.get(), n.get(), t.get());       // what er_objects_set does first ...
        const uint32_t f1[2] = {0, 2};
        er_objects_take(tab, 1, f1, ids.get(), v.get(), n.get(), t.get());
        er_skin_drop(K);                                        // ... and then: no skin survives
        EXPECT(K.skinned == 0 && K.rec.empty() && K.kind.empty() && K.rows() == 0 && !K.has(0));
        Pose p0{0, bones2, P2.get()};
        EXPECT(poses_refused(tab, K, 1, &p0, 2, "no skin"));
        Matrix m;
        m.object = 0;
        identity(m.m);
        std::vector<ErXformEntry> xe;
        EXPECT(er_xform_check(tab, 1, &m, xe, moved, why));
        er_objects_mark(tab, xe.data(), 1);
        EXPECT(!er_skin_mark_matrix(K, xe.data(), 1));          // an empty skin table: nothing to note
        er_skin_flush(tab, K, v.get(), n.get(), t.get());       // the matrix flush alone
        EXPECT(tab.pending_count == 0);
        er_skin_take(K, tab, Skin{0, bones2, b2.get(), w2.get()});      // a skin on the new table: its two rows of influences are read, no more
        EXPECT(K.skinned == 1 && K.rows() == 2 && K.rec[0].bones.size() == 24);
    }

    {   // er_skin_apply on arrays of exactly count triangles; refused influences write nothing
        const uint32_t count = 3;
        std::unique_ptr<float[]> rv(new float[count * 9]), rn(new float[count * 9]), rt(new float[count * 9]), ov(new float[count * 9]), on(new float[count * 9]), ot(new float[count * 9]);
        std::unique_ptr<uint16_t[]> b(new uint16_t[count * 12]);
        std::unique_ptr<float[]> w(new float[count * 12]);
        for (uint32_t i = 0; i < count * 9; i++) { rv[i] = (float)i; rn[i] = i < 9 ? 0.0f : 1.0f; rt[i] = 0.0f; ov[i] = on[i] = ot[i] = -7.0f; }
        for (uint32_t i = 0; i < count * 12; i++) { b[i] = (uint16_t)(i % bones2); w[i] = 0.25f; }
        b[count * 12 - 1] = bones2;
        EXPECT(!er_skin_apply(P2.get(), bones2, count, b.get(), w.get(), rv.get(), rn.get(), rt.get(), ov.get(), on.get(), ot.get(), why) && ov[0] == -7.0f);
        b[count * 12 - 1] = 0;
        EXPECT(er_skin_apply(P2.get(), bones2, count, b.get(), w.get(), rv.get(), rn.get(), rt.get(), ov.get(), on.get(), ot.get(), why) && ov[count * 9 - 1] != -7.0f);
        for (int k = 0; k < 9; k++) EXPECT(on[k] == 0.0f && ot[k] == 0.0f);      // zero directions stay zero
        EXPECT(er_skin_apply(P2.get(), bones2, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, why));
    }

    if (failures) return 1;
    std::printf("skin_host ok\n");
    return 0;
}
