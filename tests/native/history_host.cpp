// history_host.cpp -- the host routines of csrc/er_reproject.h alone: projection, back matrix, the four taps and their bilinear mean, a
// capture pixel and a blend pixel, on heap arrays of exactly the sizes the contract names.  Built with -fsanitize=address,undefined by
// tests/test_history_cpu.py: a tap read outside the captured frame (a projection onto the last row or column, or far outside), a read
// past the three words of a point or a write past the four of an output is reported; so is a float -> int conversion out of range.
// Prints "history_host ok" and returns 0, or says which expectation failed.
#include <cstdio>
#include <limits>
#include <memory>
#include <random>

#include "er_reproject.h"

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); failures++; } } while (0)

static ErReprojCam camera(float px, float py, float pz, float ax, float ay, float az) {
    ErReprojCam c;
    c.pos[0] = px; c.pos[1] = py; c.pos[2] = pz;
    c.sensor_w = 0.036f; c.sensor_h = 0.024f; c.focal = 0.05f;
    c.cx = std::cos(ax); c.sx = std::sin(ax); c.cy = std::cos(ay); c.sy = std::sin(ay); c.cz = std::cos(az); c.sz = std::sin(az);
    return c;
}

// camera_ray's pinhole direction for continuous pixel coordinates (x, y): the three rotations forward
static void pixel_dir(const ErReprojCam& c, uint32_t x_res, uint32_t y_res, float x, float y, float* d) {
    const float dx = (x / (float)x_res - 0.5f) * c.sensor_w, dy = (y / (float)y_res - 0.5f) * c.sensor_h, dz = c.focal;
    const float Xx = dx, Xy = dy * c.cx - dz * c.sx, Xz = dy * c.sx + dz * c.cx;
    const float Yx = Xx * c.cy + Xz * c.sy, Yy = Xy, Yz = Xz * c.cy - Xx * c.sy;
    d[0] = Yx * c.cz - Yy * c.sz; d[1] = Yx * c.sz + Yy * c.cz; d[2] = Yz;
}

int main() {
    std::mt19937 gen(7);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    const uint32_t W = 13, H = 9;
    const size_t npx = (size_t)W * H;
    {   // projection: the inverse of the pinhole ray, and what it refuses
        for (int trial = 0; trial < 200; trial++) {
            const ErReprojCam c = camera(U(gen), U(gen), U(gen), U(gen), U(gen), U(gen));
            const float x = (U(gen) + 1.0f) * 0.5f * W, y = (U(gen) + 1.0f) * 0.5f * H, t = 1.0f + 5.0f * (U(gen) + 1.0f);
            float d[3];
            pixel_dir(c, W, H, x, y, d);
            std::unique_ptr<float[]> p(new float[3]), out(new float[2]);
            for (int i = 0; i < 3; i++) p[i] = c.pos[i] + t * d[i];
            EXPECT(er_history_project(c, W, H, p.get(), &out[0], &out[1]));
            EXPECT(std::fabs(out[0] - x) < 1e-2f && std::fabs(out[1] - y) < 1e-2f);
            for (int i = 0; i < 3; i++) p[i] = c.pos[i] - t * d[i];      // behind
            EXPECT(!er_history_project(c, W, H, p.get(), &out[0], &out[1]) && out[0] == 0.0f && out[1] == 0.0f);
            for (int i = 0; i < 3; i++) p[i] = c.pos[i];                // at the camera
            EXPECT(!er_history_project(c, W, H, p.get(), &out[0], &out[1]));
            p[0] = std::numeric_limits<float>::quiet_NaN();
            EXPECT(!er_history_project(c, W, H, p.get(), &out[0], &out[1]));
            p[0] = std::numeric_limits<float>::infinity(); p[1] = 0.0f; p[2] = 0.0f;
            EXPECT(!er_history_project(c, W, H, p.get(), &out[0], &out[1]));
        }
    }
    {   // back matrix: B M_now x = M_capture x, an identity pair, and what it refuses
        for (int trial = 0; trial < 100; trial++) {
            std::unique_ptr<float[]> a(new float[12]), b(new float[12]), B(new float[12]);
            for (int k = 0; k < 12; k++) { a[k] = U(gen) * 0.3f + (k % 5 == 0 ? 1.0f : 0.0f); b[k] = U(gen) * 0.3f + (k % 5 == 0 ? 1.0f : 0.0f); }
            EXPECT(er_history_back_matrix(a.get(), b.get(), B.get()));
            float x[3] = {U(gen), U(gen), U(gen)}, now[3], cap[3], got[3];
            er_xform_point(b.get(), x, now);
            er_xform_point(a.get(), x, cap);
            er_xform_point(B.get(), now, got);
            for (int i = 0; i < 3; i++) EXPECT(std::fabs(got[i] - cap[i]) < 1e-4f);
            EXPECT(er_history_same_pose(a.get(), a.get()) && !er_history_same_pose(a.get(), b.get()));
            EXPECT(er_history_back_matrix(a.get(), a.get(), B.get()));
            for (int k = 0; k < 12; k++) EXPECT(std::fabs(B[k] - (k % 5 == 0 ? 1.0f : 0.0f)) < 1e-5f);
            b[0] = -b[0]; b[4] = -b[4]; b[8] = -b[8];      // a mirror
            EXPECT(!er_history_back_matrix(a.get(), b.get(), B.get()));
            b[3] = std::numeric_limits<float>::infinity();
            EXPECT(!er_history_back_matrix(a.get(), b.get(), B.get()));
        }
    }
    {   // a resolve against a captured frame of exactly W x H entries: projections everywhere, the frame's edges among them
        std::unique_ptr<uint32_t[]> old_hit(new uint32_t[npx]), old_obj(new uint32_t[npx]);
        std::unique_ptr<float[]> old_dist(new float[npx]), old_cw(new float[npx * 4]);
        const ErReprojCam c = camera(0.1f, -0.2f, 0.3f, 0.2f, -0.1f, 0.05f);
        // a coherent frame: objects in column bands (0, 1, none), sky in the last two rows, one column further away
        auto band = [](long x) -> uint32_t { return x < 5 ? 0u : x < 9 ? 1u : ER_HISTORY_NONE; };
        for (size_t q = 0; q < npx; q++) {
            old_hit[q] = q / W < 7; old_obj[q] = band((long)(q % W)); old_dist[q] = q % W == 3 ? 2.2f : 2.0f;
            for (int k = 0; k < 4; k++) old_cw[q * 4 + k] = 1.0f + U(gen);
        }
        uint64_t classes[ER_HC_COUNT] = {0, 0, 0, 0, 0};
        for (int trial = 0; trial < 4000; trial++) {
            // continuous coordinates from well outside the frame to well inside, and exactly on pixels, the last row and column included
            float x = -3.0f + (W + 6.0f) * 0.5f * (U(gen) + 1.0f), y = -3.0f + (H + 6.0f) * 0.5f * (U(gen) + 1.0f);
            if (trial % 5 == 0) { x = (float)(gen() % (W + 2)) - 1.0f; y = (float)(gen() % (H + 2)) - 1.0f; }
            float d[3];
            pixel_dir(c, W, H, x, y, d);
            const float len = er_rp_length(d[0], d[1], d[2]);
            ErHistoryKey k;
            k.hit = gen() % 5 != 0; k.object = gen() % 4 ? band((long)std::floor(x)) : gen() % 3; k.dist = 0.0f;
            const float t = 2.0f / len;
            for (int i = 0; i < 3; i++) k.P[i] = k.hit ? c.pos[i] + t * d[i] : d[i] / len;
            if (trial % 97 == 0) k.P[1] = std::numeric_limits<float>::quiet_NaN();
            if (trial % 89 == 0) k.P[0] = 3e38f;
            std::unique_ptr<float[]> out(new float[4]);
            std::unique_ptr<int[]> state(new int[4]);
            const int cls = er_history_resolve_px(k, nullptr, 0u, c, W, H, 0.02f, old_hit.get(), old_obj.get(), old_dist.get(), old_cw.get(), out.get(), state.get());
            EXPECT(cls >= 0 && cls < ER_HC_COUNT);
            classes[cls]++;
            int valid = 0;
            for (int s = 0; s < 4; s++) valid += state[s] == ER_TAP_VALID;
            EXPECT((cls == ER_HC_SKY) == (k.hit == 0u));
            if (k.hit) EXPECT((cls == ER_HC_VALID) == (valid == 4) && (cls == ER_HC_PARTIAL) == (valid > 0 && valid < 4));
            if (valid == 0) for (int q = 0; q < 4; q++) EXPECT(out[q] == 0.0f);
            else if (out[3] != 0.0f) for (int q = 0; q < 4; q++) EXPECT(out[q] >= 0.0f && out[q] <= 2.0f);      // a mean lies between its terms
        }
        for (int q = 0; q < ER_HC_COUNT; q++) EXPECT(classes[q] > 0);
        // a moved object: the back matrix is read (12 floats exactly)
        std::unique_ptr<float[]> B(new float[12]);
        for (int k = 0; k < 12; k++) B[k] = k % 5 == 0 ? 1.0f : 0.0f;
        B[3] = 0.01f;
        ErHistoryKey k;
        k.hit = 1u; k.object = 1u; k.dist = 2.0f;
        float d[3];
        pixel_dir(c, W, H, 6.0f, 4.0f, d);
        for (int i = 0; i < 3; i++) k.P[i] = c.pos[i] + d[i] * (2.0f / er_rp_length(d[0], d[1], d[2]));
        float out[4];
        int state[4];
        er_history_resolve_px(k, B.get(), 1u, c, W, H, 0.02f, old_hit.get(), old_obj.get(), old_dist.get(), old_cw.get(), out, state);
    }
    {   // capture and blend pixels
        std::unique_ptr<float[]> b(new float[3]), h(new float[4]), out(new float[4]);
        b[0] = 0.5f; b[1] = 0.25f; b[2] = 1.0f;
        er_history_capture_px(b.get(), 1u, nullptr, 32.0f, out.get());      // only the setup sample: nothing to carry
        for (int q = 0; q < 4; q++) EXPECT(out[q] == 0.0f);
        er_history_capture_px(b.get(), 0u, nullptr, 32.0f, out.get());
        EXPECT(out[3] == 0.0f);
        er_history_capture_px(b.get(), 5u, nullptr, 32.0f, out.get());      // n = 4: m = b * 5 / 4, C = m
        EXPECT(out[0] == (4.0f * (0.5f * (5.0f / 4.0f))) / 4.0f && out[3] == 4.0f);
        h[0] = 1.0f; h[1] = 1.0f; h[2] = 1.0f; h[3] = 30.0f;
        er_history_capture_px(b.get(), 5u, h.get(), 32.0f, out.get());
        EXPECT(out[3] == 32.0f && out[0] > 0.625f && out[0] < 1.0f);      // the cap; between the two means
        er_history_blend_px(b.get(), 1u, h.get(), out.get());
        EXPECT(out[0] == 1.0f && out[3] == 1.0f);                           // history alone
        h[3] = 0.0f;
        er_history_blend_px(b.get(), 1u, h.get(), out.get());
        EXPECT(out[0] == 0.5f && out[1] == 0.25f && out[2] == 1.0f && out[3] == 1.0f);      // w + n = 0: the setup colour
    }
    if (failures) { std::printf("history_host: %d expectation(s) failed\n", failures); return 1; }
    std::printf("history_host ok\n");
    return 0;
}
