// variance_host.cpp -- the routines of csrc/er_variance.h alone: mark, fold, value, the split and one filter level, on heap arrays of
// exactly the sizes the contract names (a frame of x_res * y_res entries per plane, 12 words per pixel of state).  Built with
// -fsanitize=address,undefined by tests/test_variance_cpu.py: a tap read outside a plane (the 5 x 5 stencil at step 16 reaches 32 pixels
// beyond every edge of this frame, the 3 x 3 mean one pixel), a read or write past a pixel's 12 words or past the four of an output is
// reported; so is signed overflow in the tap coordinates.  Prints "variance_host ok" and returns 0, or says which expectation failed.
#include <cmath>
#include <cstdio>
#include <memory>
#include <random>

#include "er_variance.h"

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); failures++; } } while (0)

int main() {
    std::mt19937 gen(11);
    std::normal_distribution<float> N(0.0f, 1.0f);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    const int W = 13, H = 9;
    const size_t npx = (size_t)W * H;
    std::unique_ptr<float[]> beauty(new float[npx * 4]), state(new float[npx * ER_VARIANCE_WORDS]), value(new float[npx * 4]);
    std::unique_ptr<uint32_t[]> samples(new uint32_t[npx]);
    std::unique_ptr<float[]> sigma(new float[npx]);
    // the reference's recurrence from the setup state: I = 0, count 1
    for (size_t p = 0; p < npx; p++) {
        for (int c = 0; c < 4; c++) beauty[p * 4 + c] = c == 3 ? 1.0f : 0.0f;
        samples[p] = 1u;
        sigma[p] = 0.05f + U(gen);
        er_variance_mark_px(&beauty[p * 4], samples[p], &state[p * ER_VARIANCE_WORDS]);
        EXPECT(er_var_u(state[p * ER_VARIANCE_WORDS + 3]) == 1u && er_var_u(state[p * ER_VARIANCE_WORDS + 11]) == 0u);
    }
    const int pattern[6] = {1, 2, 3, 2, 4, 4};
    size_t frozen = 5;      // one pixel receives nothing in the third batch: its 12 words stay
    for (int b = 0; b < 6; b++) {
        for (size_t p = 0; p < npx; p++) {
            if (b == 2 && p == frozen) continue;
            for (int k = 0; k < pattern[b]; k++) {
                const float sa = (float)samples[p];
                for (int c = 0; c < 3; c++) {
                    const float L = 1.0f + sigma[p] * N(gen);
                    beauty[p * 4 + c] = beauty[p * 4 + c] * sa / (sa + 1.0f) + L / (sa + 1.0f);
                }
                samples[p]++;
            }
        }
        float before[ER_VARIANCE_WORDS];
        for (size_t p = 0; p < npx; p++) {
            for (int i = 0; i < ER_VARIANCE_WORDS; i++) before[i] = state[p * ER_VARIANCE_WORDS + i];
            const bool folded = er_variance_fold_px(&beauty[p * 4], samples[p], &state[p * ER_VARIANCE_WORDS]);
            if (b == 2 && p == frozen) {
                EXPECT(!folded);
                for (int i = 0; i < ER_VARIANCE_WORDS; i++) EXPECT(er_var_u(before[i]) == er_var_u(state[p * ER_VARIANCE_WORDS + i]));
            } else {
                EXPECT(folded);
                EXPECT(er_var_u(state[p * ER_VARIANCE_WORDS + 3]) == samples[p]);
            }
            er_variance_value_px(&state[p * ER_VARIANCE_WORDS], samples[p], &value[p * 4]);
            const uint32_t K = er_var_u(state[p * ER_VARIANCE_WORDS + 11]);
            EXPECT(value[p * 4 + 3] == (float)K);
            for (int c = 0; c < 3; c++) EXPECT(value[p * 4 + c] >= 0.0f && (K >= 2u || value[p * 4 + c] == 0.0f));
        }
    }
    // the estimate is near the truth: sum of v against the sum of sigma^2 (M - 1) / M^2; 6 standard deviations of 3 channels x npx pixels
    // with at least 4 degrees of freedom each (K is 6, 5 for the frozen pixel)
    double got = 0, want = 0;
    for (size_t p = 0; p < npx; p++) {
        const double M = samples[p];
        for (int c = 0; c < 3; c++) got += value[p * 4 + c];
        want += 3.0 * sigma[p] * sigma[p] * (M - 1.0) / (M * M);
    }
    EXPECT(std::fabs(got / want - 1.0) < 6.0 * std::sqrt(2.0 / (4.0 * 3.0 * (double)npx)));
    // a pixel at count 1 with two "batches" cannot exist, but the value must not divide by zero visibly: M = 1 gives 0
    {
        float st[ER_VARIANCE_WORDS] = {0}, out[4];
        st[8] = 1.0f; st[9] = 2.0f; st[10] = 3.0f; st[11] = er_var_f(2u);
        er_variance_value_px(st, 1u, out);
        EXPECT(out[0] == 0.0f && out[1] == 0.0f && out[2] == 0.0f && out[3] == 2.0f);
    }
    // the filter: planes of exactly npx float4, every level's step, both flags
    std::unique_ptr<float[]> e(new float[npx * 4]), ve(new float[npx * 4]), normal(new float[npx * 4]), albedo(new float[npx * 4]), depth(new float[npx * 4]);
    std::unique_ptr<float[]> oe(new float[npx * 4]), ov(new float[npx * 4]);
    for (size_t p = 0; p < npx; p++) {
        const float a[3] = {0.2f + 0.6f * U(gen), 0.2f + 0.6f * U(gen), 0.2f + 0.6f * U(gen)};
        for (int c = 0; c < 3; c++) {
            albedo[p * 4 + c] = a[c];
            e[p * 4 + c] = beauty[p * 4 + c] / (a[c] + 0.01f);
            normal[p * 4 + c] = c == 2 ? 1.0f : 0.0f;
        }
        if (p % 7 == 0) normal[p * 4 + 2] = 0.0f;      // sky: no normal
        albedo[p * 4 + 3] = normal[p * 4 + 3] = e[p * 4 + 3] = 1.0f;
        for (int c = 0; c < 4; c++) depth[p * 4 + c] = c == 3 ? 1.0f : 2.0f + (float)(p % W) * 0.01f;
        if (p % 5 == 0) value[p * 4 + 3] = 1.0f;      // K < 2: the centre takes wc = 1
        er_variance_split_px(&value[p * 4], &albedo[p * 4], &ve[p * 4]);
        EXPECT(ve[p * 4 + 3] == (p % 5 == 0 ? 0.0f : 1.0f));
    }
    const float kc = 1.0f / 9.0f, ka = 1.0f / (0.3f * 0.3f), kz = 1.0f / (0.2f * 0.2f);
    for (int step = 1; step <= 128; step *= 2) {
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t p = (size_t)y * W + x;
                er_variance_level_px(e.get(), ve.get(), normal.get(), 4, albedo.get(), depth.get(), W, H, x, y, step, kc, ka, kz, &oe[p * 4], &ov[p * 4]);
                for (int c = 0; c < 3; c++) EXPECT(std::isfinite(oe[p * 4 + c]) && ov[p * 4 + c] >= 0.0f);
                EXPECT(oe[p * 4 + 3] == e[p * 4 + 3] && ov[p * 4 + 3] == ve[p * 4 + 3]);
            }
        // the squares of normalised weights sum to at most 1: no propagated variance exceeds the largest one that went in
        float top = 0;
        for (size_t p = 0; p < npx; p++) top = ve[p * 4] > top ? ve[p * 4] : top;
        for (size_t p = 0; p < npx; p++) EXPECT(ov[p * 4] <= top * (1.0f + 1e-5f));
    }
    // a frame of one pixel: every tap is the centre
    {
        er_variance_level_px(e.get(), ve.get(), normal.get(), 4, albedo.get(), depth.get(), 1, 1, 0, 0, 16, kc, ka, kz, oe.get(), ov.get());
        for (int c = 0; c < 3; c++) EXPECT(std::fabs(oe[c] - e[c]) <= 1e-6f * std::fabs(e[c]));
    }
    if (failures) { std::printf("variance_host: %d expectations failed\n", failures); return 1; }
    std::printf("variance_host ok\n");
    return 0;
}
