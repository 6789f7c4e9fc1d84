// Stand-in for the SYCL header, written from the public SYCL 2020 names only (oracle/ref_shim/README.md): enough for a HOST
// compiler to build the reference's per-sample path serially.  Math: every sycl:: function forwards to <cmath>, except that with
// ER_REF_MATH_ER the six functions er_math.h implements forward to it (float overloads; the double overloads stay <cmath>).
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <exception>
#ifdef ER_REF_MATH_ER
#include "er_math.h"
#endif

#ifndef SYCL_EXTERNAL
#define SYCL_EXTERNAL
#endif

namespace sycl {

// IEEE operations and classification: the same in both builds
inline float sqrt(float x) { return std::sqrt(x); }
inline double sqrt(double x) { return std::sqrt(x); }
inline float floor(float x) { return std::floor(x); }
inline double floor(double x) { return std::floor(x); }
inline float abs(float x) { return std::fabs(x); }
inline double abs(double x) { return std::fabs(x); }
inline int abs(int x) { return std::abs(x); }
inline float fabs(float x) { return std::fabs(x); }
inline double fabs(double x) { return std::fabs(x); }
inline bool isnan(float x) { return std::isnan(x); }
inline bool isnan(double x) { return std::isnan(x); }
inline bool isinf(float x) { return std::isinf(x); }
inline bool isinf(double x) { return std::isinf(x); }

// elementary functions outside the six: libm in both builds
inline float exp(float x) { return std::exp(x); }
inline float tan(float x) { return std::tan(x); }
inline float asin(float x) { return std::asin(x); }
inline float atan(float x) { return std::atan(x); }
inline float fmod(float x, float y) { return std::fmod(x, y); }

// the six
#ifdef ER_REF_MATH_ER
inline float sin(float x) { return ermath::er_sin(x); }
inline float cos(float x) { return ermath::er_cos(x); }
inline float acos(float x) { return ermath::er_acos(x); }
inline float log(float x) { return ermath::er_log(x); }
inline float pow(float x, float y) { return ermath::er_pow(x, y); }
inline float atan2(float y, float x) { return ermath::er_atan2(y, x); }
#else
inline float sin(float x) { return std::sin(x); }
inline float cos(float x) { return std::cos(x); }
inline float acos(float x) { return std::acos(x); }
inline float log(float x) { return std::log(x); }
inline float pow(float x, float y) { return std::pow(x, y); }
inline float atan2(float y, float x) { return std::atan2(y, x); }
#endif
inline double sin(double x) { return std::sin(x); }
inline double cos(double x) { return std::cos(x); }
inline double acos(double x) { return std::acos(x); }
inline double log(double x) { return std::log(x); }
inline double pow(double x, double y) { return std::pow(x, y); }
inline double atan2(double y, double x) { return std::atan2(y, x); }

template <class T> T min(T a, T b) { return b < a ? b : a; }
template <class T> T max(T a, T b) { return a < b ? b : a; }
template <class T> T clamp(T x, T lo, T hi) { return x < lo ? lo : (hi < x ? hi : x); }

// a serial queue: parallel_for visits the global range in order on the calling thread
struct range {
    size_t dim[2];
    template <class A, class B> range(A a, B b) : dim{(size_t)a, (size_t)b} {}
    size_t operator[](int i) const { return dim[i]; }
};
struct nd_range {
    range global, local;
    nd_range(range g, range l) : global(g), local(l) {}
};
template <int Dims> struct nd_item {
    size_t id[2];
    size_t get_global_id(int i) const { return id[i]; }
};
struct handler {
    template <class KernelName = void, class F> void parallel_for(nd_range r, F f) {
        for (size_t i = 0; i < r.global[0]; i++)
            for (size_t j = 0; j < r.global[1]; j++) {
                nd_item<2> it{{i, j}};
                f(it);
            }
    }
};
struct event {
    void wait() {}
};
struct device {};
struct queue {
    template <class F> event submit(F f) {
        handler h;
        f(h);
        return event();
    }
};
template <class KernelName> bool is_compatible(const device&) { return true; }

}  // namespace sycl

namespace cl {
namespace sycl = ::sycl;
}
