// cutout_host.cpp -- the routines of csrc/er_cutout.h alone: the threshold parameter, the stop test and the continuation ray, on heap
// arrays of exactly three floats.  Built with -fsanitize=address,undefined by tests/test_first_hit_cpu.py: a read past a position or a
// direction, or a write past an output, is reported.  Prints "cutout_host ok" and returns 0, or says which expectation failed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>

#include "er_cutout.h"

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); failures++; } } while (0)

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // the parameter
    EXPECT(er_cutout_threshold_ok(0.0f) && er_cutout_threshold_ok(-0.0f) && er_cutout_threshold_ok(1.0f) && er_cutout_threshold_ok(1e-30f));
    EXPECT(!er_cutout_threshold_ok(nan) && !er_cutout_threshold_ok(-1e-30f) && !er_cutout_threshold_ok(std::nextafter(1.0f, 2.0f)) && !er_cutout_threshold_ok(inf) &&
           !er_cutout_threshold_ok(-inf));
    EXPECT(er_cutout_threshold(0.0f) == 0.5f && er_cutout_threshold(-0.0f) == 0.5f && er_cutout_threshold(0.25f) == 0.25f && er_cutout_threshold(1.0f) == 1.0f);
    // the stop test at its edges
    EXPECT(er_cutout_stops(0.5f, 0.5f) && !er_cutout_stops(std::nextafter(0.5f, 0.0f), 0.5f) && er_cutout_stops(std::nextafter(0.5f, 1.0f), 0.5f));
    EXPECT(!er_cutout_stops(nan, 0.5f) && !er_cutout_stops(nan, 1e-30f));
    EXPECT(!er_cutout_stops(0.0f, 0.5f) && !er_cutout_stops(-0.0f, 1e-30f) && !er_cutout_stops(-1.5f, 1e-30f) && !er_cutout_stops(-inf, 0.5f));
    EXPECT(er_cutout_stops(1.0f, 1.0f) && er_cutout_stops(2.5f, 1.0f) && er_cutout_stops(inf, 1.0f) && !er_cutout_stops(std::nextafter(1.0f, 0.0f), 1.0f));
    // the continuation: exactly three floats in, three and three out
    std::mt19937 gen(5);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    for (int i = 0; i < 1000; i++) {
        std::unique_ptr<float[]> p(new float[3]), d(new float[3]), o(new float[3]), n(new float[3]);
        for (int c = 0; c < 3; c++) { p[c] = 4.0f * U(gen); d[c] = U(gen); }
        if (i == 0) d[0] = d[1] = d[2] = 0.0f;      // a zero direction is kept, not divided
        er_cutout_continue(p.get(), d.get(), o.get(), n.get());
        const float l = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        for (int c = 0; c < 3; c++) {
            EXPECT(bits(o[c]) == bits(p[c] + d[c] * 0.001f));
            EXPECT(bits(n[c]) == bits(l != 0.0f ? d[c] / l : d[c]));
        }
        if (i == 0) EXPECT(n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f && bits(o[0]) == bits(p[0]));
        // in place: the outputs may be the inputs
        er_cutout_continue(p.get(), d.get(), p.get(), d.get());
        for (int c = 0; c < 3; c++) EXPECT(bits(p[c]) == bits(o[c]) && bits(d[c]) == bits(n[c]));
    }
    if (failures) { std::printf("cutout_host: %d expectation(s) failed\n", failures); return 1; }
    std::printf("cutout_host ok\n");
    return 0;
}
