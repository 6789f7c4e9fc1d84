// history_variance_host.cpp -- the routines of csrc/er_history_variance.h alone: the current per-sample variance, the pool, a capture
// pixel, the mean over the known taps, a resolve against captured planes of exactly x_res * y_res entries, the blend's variance and the
// filter's split, on heap arrays of exactly the sizes the contract names.  Built with -fsanitize=address,undefined by
// tests/test_history_variance_cpu.py: a tap read outside the captured SV plane, a read past the four words of a pixel or a write past the
// four of an output is reported.  Prints "history_variance_host ok" and returns 0, or says which expectation failed.
#include <cstdio>
#include <limits>
#include <memory>
#include <random>

#include "er_history_variance.h"

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); failures++; } } while (0)

static float word(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static ErReprojCam camera(float px, float py, float pz, float ax, float ay, float az) {
    ErReprojCam c;
    c.pos[0] = px; c.pos[1] = py; c.pos[2] = pz;
    c.sensor_w = 0.036f; c.sensor_h = 0.024f; c.focal = 0.05f;
    c.cx = std::cos(ax); c.sx = std::sin(ax); c.cy = std::cos(ay); c.sy = std::sin(ay); c.cz = std::cos(az); c.sz = std::sin(az);
    return c;
}

static void pixel_dir(const ErReprojCam& c, uint32_t x_res, uint32_t y_res, float x, float y, float* d) {
    const float dx = (x / (float)x_res - 0.5f) * c.sensor_w, dy = (y / (float)y_res - 0.5f) * c.sensor_h, dz = c.focal;
    const float Xx = dx, Xy = dy * c.cx - dz * c.sx, Xz = dy * c.sx + dz * c.cx;
    const float Yx = Xx * c.cy + Xz * c.sy, Yy = Xy, Yz = Xz * c.cy - Xx * c.sy;
    d[0] = Yx * c.cz - Yy * c.sz; d[1] = Yx * c.sz + Yy * c.cz; d[2] = Yz;
}

int main() {
    std::mt19937 gen(11);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    {   // the current variance: K of 0, 1, 2 and 9, a negative and a NaN M2, no state at all
        std::unique_ptr<float[]> m(new float[4]), s(new float[3]);
        m[0] = 4.0f; m[1] = -1.0f; m[2] = nan;
        for (uint32_t K : {0u, 1u}) {
            m[3] = word(K);
            EXPECT(er_hv_current_px(m.get(), s.get()) == 0u && s[0] == 0.0f && s[1] == 0.0f && s[2] == 0.0f);
        }
        m[3] = word(2u);
        EXPECT(er_hv_current_px(m.get(), s.get()) == 1u && s[0] == 4.0f && s[1] == 0.0f && s[2] == 0.0f);
        m[3] = word(9u);
        EXPECT(er_hv_current_px(m.get(), s.get()) == 1u && s[0] == 0.5f && s[1] == 0.0f && s[2] == 0.0f);
        EXPECT(er_hv_current_px(nullptr, s.get()) == 0u && s[0] == 0.0f);
        EXPECT(er_hv_samples_n(0u) == 0.0f && er_hv_samples_n(1u) == 0.0f && er_hv_samples_n(5u) == 4.0f);
    }
    {   // the pool: both, one (bit for bit), none
        std::unique_ptr<float[]> a(new float[3]), b(new float[3]), o(new float[3]);
        for (int c = 0; c < 3; c++) { a[c] = 1.0f + c; b[c] = 0.25f; }
        EXPECT(er_hv_pool_px(a.get(), 1u, 6.0f, b.get(), 1u, 2.0f, o.get()) == 1u && o[0] == (6.0f * 1.0f + 2.0f * 0.25f) / 8.0f);
        EXPECT(er_hv_pool_px(a.get(), 1u, 6.0f, b.get(), 0u, 2.0f, o.get()) == 1u && o[0] == 1.0f && o[2] == 3.0f);
        EXPECT(er_hv_pool_px(a.get(), 1u, 6.0f, b.get(), 1u, 0.0f, o.get()) == 1u && o[1] == 2.0f);
        EXPECT(er_hv_pool_px(a.get(), 1u, 0.0f, b.get(), 1u, 2.0f, o.get()) == 1u && o[0] == 0.25f);
        EXPECT(er_hv_pool_px(a.get(), 0u, 6.0f, b.get(), 1u, 2.0f, o.get()) == 1u && o[0] == 0.25f);
        EXPECT(er_hv_pool_px(a.get(), 1u, 0.0f, b.get(), 1u, 0.0f, o.get()) == 0u && o[0] == 0.0f && o[1] == 0.0f && o[2] == 0.0f);
        EXPECT(er_hv_pool_px(a.get(), 0u, 6.0f, b.get(), 0u, 2.0f, o.get()) == 0u && o[0] == 0.0f);
    }
    {   // a capture pixel and a blend pixel
        std::unique_ptr<float[]> m(new float[4]), hv(new float[4]), sv(new float[4]), vb(new float[4]);
        m[0] = 8.0f; m[1] = 8.0f; m[2] = 8.0f; m[3] = word(5u);      // s2 = 2
        EXPECT(er_hv_capture_px(m.get(), 9u, 0.0f, nullptr, sv.get()) == 1u && sv[0] == 2.0f && sv[3] == 1.0f);
        EXPECT(er_hv_capture_px(m.get(), 1u, 0.0f, nullptr, sv.get()) == 0u && sv[0] == 0.0f && sv[3] == 0.0f);      // n = 0: nothing to weigh
        EXPECT(er_hv_capture_px(nullptr, 9u, 0.0f, nullptr, sv.get()) == 0u && sv[3] == 0.0f);
        hv[0] = 1.0f; hv[1] = 1.0f; hv[2] = 1.0f; hv[3] = 1.0f;
        EXPECT(er_hv_capture_px(nullptr, 3u, 4.0f, hv.get(), sv.get()) == 1u && sv[0] == 1.0f && sv[3] == 1.0f);      // the history's alone, carried on
        EXPECT(er_hv_capture_px(m.get(), 3u, 6.0f, hv.get(), sv.get()) == 1u && sv[0] == (6.0f * 1.0f + 2.0f * 2.0f) / 8.0f);
        hv[3] = 0.0f;
        EXPECT(er_hv_capture_px(nullptr, 3u, 4.0f, hv.get(), sv.get()) == 0u && sv[0] == 0.0f);
        hv[3] = 1.0f;
        EXPECT(er_hv_blend_px(nullptr, 3u, 6.0f, hv.get(), vb.get()) == 1u && vb[0] == 1.0f / 8.0f && vb[3] == 1.0f);
        EXPECT(er_hv_blend_px(m.get(), 3u, 6.0f, nullptr, vb.get()) == 1u && vb[0] == 2.0f / 8.0f);
        EXPECT(er_hv_blend_px(nullptr, 3u, 6.0f, nullptr, vb.get()) == 0u && vb[0] == 0.0f && vb[3] == 0.0f);
        EXPECT(er_hv_blend_px(nullptr, 1u, 0.0f, hv.get(), vb.get()) == 0u && vb[0] == 0.0f);      // w + n = 0
        std::unique_ptr<float[]> bl(new float[4]), al(new float[3]), e(new float[4]), ve(new float[4]);
        bl[0] = 0.5f; bl[1] = 0.25f; bl[2] = 1.0f; bl[3] = 1.0f;
        al[0] = 0.49f; al[1] = 0.0f; al[2] = 0.99f;
        vb[0] = 0.125f; vb[1] = 0.125f; vb[2] = 0.125f; vb[3] = 1.0f;
        er_hv_split_px(bl.get(), vb.get(), al.get(), e.get(), ve.get());
        EXPECT(e[0] == 0.5f / (0.49f + 0.01f) && ve[1] == 0.125f / ((0.0f + 0.01f) * (0.0f + 0.01f)) && e[3] == 1.0f && ve[3] == 1.0f);
    }
    {   // the mean over the known taps: flags of 0 among valid taps, all taps invalid
        std::unique_ptr<int[]> st(new int[4]);
        std::unique_ptr<float[]> tw(new float[4]), out(new float[4]);
        std::unique_ptr<float[][4]> sv(new float[4][4]);
        for (int k = 0; k < 4; k++) { st[k] = ER_TAP_VALID; tw[k] = 0.25f; for (int c = 0; c < 4; c++) sv[k][c] = c == 3 ? 1.0f : (float)(k + 1); }
        EXPECT(er_hv_mean(st.get(), tw.get(), sv.get(), out.get()) == 1u && out[0] == 2.5f && out[3] == 1.0f);
        sv[3][3] = 0.0f; sv[2][3] = 0.0f;
        EXPECT(er_hv_mean(st.get(), tw.get(), sv.get(), out.get()) == 1u && out[0] == 1.5f);
        st[0] = ER_TAP_DEPTH;
        EXPECT(er_hv_mean(st.get(), tw.get(), sv.get(), out.get()) == 1u && out[0] == 2.0f);
        st[1] = ER_TAP_OUTSIDE;
        EXPECT(er_hv_mean(st.get(), tw.get(), sv.get(), out.get()) == 0u && out[0] == 0.0f && out[3] == 0.0f);
        for (int k = 0; k < 4; k++) st[k] = ER_TAP_OBJECT;
        EXPECT(er_hv_mean(st.get(), tw.get(), sv.get(), out.get()) == 0u && out[3] == 0.0f);
    }
    {   // a resolve against captured planes of exactly W x H entries: projections everywhere, the frame's edges among them
        const uint32_t W = 13, H = 9;
        const size_t npx = (size_t)W * H;
        std::unique_ptr<uint32_t[]> old_hit(new uint32_t[npx]), old_obj(new uint32_t[npx]);
        std::unique_ptr<float[]> old_dist(new float[npx]), old_cw(new float[npx * 4]), old_sv(new float[npx * 4]);
        const ErReprojCam c = camera(0.1f, -0.2f, 0.3f, 0.2f, -0.1f, 0.05f);
        auto band = [](long x) -> uint32_t { return x < 5 ? 0u : x < 9 ? 1u : ER_HISTORY_NONE; };
        for (size_t q = 0; q < npx; q++) {
            old_hit[q] = q / W < 7; old_obj[q] = band((long)(q % W)); old_dist[q] = q % W == 3 ? 2.2f : 2.0f;
            const bool known = gen() % 3 != 0;
            for (int k = 0; k < 4; k++) { old_cw[q * 4 + k] = 1.0f + U(gen); old_sv[q * 4 + k] = known ? (k == 3 ? 1.0f : 1.0f + U(gen)) : 0.0f; }
        }
        int with_hv = 0, without_hv = 0;
        for (int trial = 0; trial < 4000; trial++) {
            float x = -3.0f + (W + 6.0f) * 0.5f * (U(gen) + 1.0f), y = -3.0f + (H + 6.0f) * 0.5f * (U(gen) + 1.0f);
            if (trial % 5 == 0) { x = (float)(gen() % (W + 2)) - 1.0f; y = (float)(gen() % (H + 2)) - 1.0f; }
            float d[3];
            pixel_dir(c, W, H, x, y, d);
            const float len = er_rp_length(d[0], d[1], d[2]);
            ErHistoryKey k;
            k.hit = gen() % 5 != 0; k.object = gen() % 4 ? band((long)std::floor(x)) : gen() % 3; k.dist = 0.0f;
            const float t = 2.0f / len;
            for (int i = 0; i < 3; i++) k.P[i] = k.hit ? c.pos[i] + t * d[i] : d[i] / len;
            if (trial % 97 == 0) k.P[1] = nan;
            if (trial % 89 == 0) k.P[0] = 3e38f;
            std::unique_ptr<float[]> hist(new float[4]), hv(new float[4]), plain(new float[4]);
            std::unique_ptr<int[]> state(new int[4]), state2(new int[4]);
            const int cls = er_hv_resolve_px(k, nullptr, 0u, c, W, H, 0.02f, old_hit.get(), old_obj.get(), old_dist.get(), old_cw.get(), old_sv.get(), hist.get(), hv.get(), state.get());
            const int cls2 = er_history_resolve_px(k, nullptr, 0u, c, W, H, 0.02f, old_hit.get(), old_obj.get(), old_dist.get(), old_cw.get(), plain.get(), state2.get());
            EXPECT(cls == cls2 && memcmp(hist.get(), plain.get(), 16) == 0 && memcmp(state.get(), state2.get(), 16) == 0);      // the colour is the plain resolve's
            int valid = 0;
            for (int s = 0; s < 4; s++) valid += state[s] == ER_TAP_VALID;
            EXPECT(hv[3] == 0.0f || hv[3] == 1.0f);
            if (hv[3] != 0.0f) { with_hv++; EXPECT(valid > 0); for (int q = 0; q < 3; q++) EXPECT(hv[q] >= 0.0f && hv[q] <= 2.0f); }      // a mean lies between its terms
            else { without_hv++; for (int q = 0; q < 3; q++) EXPECT(hv[q] == 0.0f); }
        }
        EXPECT(with_hv > 100 && without_hv > 100);
    }
    if (failures) { std::printf("history_variance_host: %d expectation(s) failed\n", failures); return 1; }
    std::printf("history_variance_host ok\n");
    return 0;
}
