// er_variance.hip -- the variance plane by batch means and the a-trous filter guided by it (include/eleven_hip.h er_variance_fold,
// er_variance_info, er_read_variance, er_denoise_variance).
//
// Every kernel here is one work item per pixel around a routine of er_variance.h, which states the arithmetic.  They read BEAUTY, the
// sample counts, NORMAL and the feature planes and write planes of their own and DENOISE: a render with folds, reads and the filter in
// between is, bit for bit, the render without them.
#include "er_variance.h"

#include "er_features.h"
#include "er_scene.h"

using namespace erh;

namespace {

// a pixel's 12 words through three 16-byte loads and stores
__device__ __forceinline__ void var_load(const float4* __restrict__ state, size_t npx, size_t p, float* st) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float4 v = state[(size_t)k * npx + p];
        st[4 * k] = v.x; st[4 * k + 1] = v.y; st[4 * k + 2] = v.z; st[4 * k + 3] = v.w;
    }
}
__device__ __forceinline__ void var_store(float4* __restrict__ state, size_t npx, size_t p, const float* st) {
#pragma unroll
    for (int k = 0; k < 3; k++) state[(size_t)k * npx + p] = make_float4(st[4 * k], st[4 * k + 1], st[4 * k + 2], st[4 * k + 3]);
}

}  // namespace

// mark: the snapshot from the planes as they lie, or -- passes NULL -- from a render that has just started ((0, 0, 0), count 1)
__global__ __launch_bounds__(256) void k_variance_mark(const float4* __restrict__ passes, const uint32_t* __restrict__ samples, size_t npx, float4* __restrict__ state) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npx) return;
    float rgb[3] = {0.0f, 0.0f, 0.0f}, st[ER_VARIANCE_WORDS];
    uint32_t M = 1u;
    if (passes) {
        const float4 b = passes[er_pass_index(npx, ER_PASS_BEAUTY, p)];
        rgb[0] = b.x; rgb[1] = b.y; rgb[2] = b.z;
        M = samples[p];
    }
    er_variance_mark_px(rgb, M, st);
    var_store(state, npx, p, st);
}

// fold: one batch per pixel that received samples since its snapshot; counts[0] pixels folded, counts[ER_VAR_COUNT_STRIDE] pixels with
// K >= 2 after it.  A bounded grid walks the frame with a grid stride: per step one ballot per wave and counter, summed in a register, and
// at the end one atomicAdd per wave and counter.  (One workgroup per 256 pixels with an add per wave took 0.75 ms at 1080p -- 64 800 adds
// on two addresses -- where this form takes 0.09: DESIGN.md 3m.)  The two counters lie 64 bytes apart.
#define ER_VAR_COUNT_STRIDE 16
__global__ __launch_bounds__(256) void k_variance_fold(const float4* __restrict__ passes, const uint32_t* __restrict__ samples, size_t npx, float4* __restrict__ state,
                                                       uint32_t* __restrict__ counts) {
    uint32_t nf = 0, nk = 0;
    // (every lane of a wave takes the same number of steps: the bound is on the wave's first pixel)
    for (size_t base = ((size_t)blockIdx.x * 256 + (threadIdx.x & ~63u)); base < npx; base += (size_t)gridDim.x * 256) {
        const size_t p = base + (threadIdx.x & 63u);
        bool folded = false, known = false;
        if (p < npx) {
            const float4 b = passes[er_pass_index(npx, ER_PASS_BEAUTY, p)];
            const float rgb[3] = {b.x, b.y, b.z};
            float st[ER_VARIANCE_WORDS];
            var_load(state, npx, p, st);
            folded = er_variance_fold_px(rgb, samples[p], st);
            if (folded) var_store(state, npx, p, st);      // (an untouched pixel keeps its words: nothing is written)
            known = er_var_u(st[11]) >= 2u;
        }
        nf += (uint32_t)__popcll(__ballot(folded));
        nk += (uint32_t)__popcll(__ballot(known));
    }
    const bool first = (threadIdx.x & 63u) == 0u;
    if (first && nf) atomicAdd(counts, nf);
    if (first && nk) atomicAdd(counts + ER_VAR_COUNT_STRIDE, nk);
}

// er_read_variance's plane
__global__ __launch_bounds__(256) void k_variance_value(const float4* __restrict__ state, const uint32_t* __restrict__ samples, size_t npx, float4* __restrict__ dst) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npx) return;
    const float4 m2 = state[2 * npx + p];
    float st[ER_VARIANCE_WORDS] = {0};
    st[8] = m2.x; st[9] = m2.y; st[10] = m2.z; st[11] = m2.w;
    float out[4];
    er_variance_value_px(st, samples[p], out);
    dst[p] = make_float4(out[0], out[1], out[2], out[3]);
}

// er_guided_split_kernel's demodulation and the demodulated variance beside it
__global__ __launch_bounds__(256) void er_variance_split_kernel(const float4* __restrict__ beauty, int beauty_stride, const float4* __restrict__ albedo,
                                                                 const float4* __restrict__ state, const uint32_t* __restrict__ samples, float4* __restrict__ e,
                                                                 float4* __restrict__ ve, size_t npx) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npx) return;
    const float4 b = beauty[i * beauty_stride], a = albedo[i], m2 = state[2 * npx + i];
    e[i] = make_float4(b.x / (a.x + 0.01f), b.y / (a.y + 0.01f), b.z / (a.z + 0.01f), b.w);
    float st[ER_VARIANCE_WORDS] = {0};
    st[8] = m2.x; st[9] = m2.y; st[10] = m2.z; st[11] = m2.w;
    float v[4], out[4];
    const float al[3] = {a.x, a.y, a.z};
    er_variance_value_px(st, samples[i], v);
    er_variance_split_px(v, al, out);
    ve[i] = make_float4(out[0], out[1], out[2], out[3]);
}

// one level: er_guided_level_kernel's launch (16 x 16 pixels per workgroup), er_variance_level_px per pixel
__global__ __launch_bounds__(256) void er_variance_level_kernel(const float4* __restrict__ src, const float4* __restrict__ vsrc, const float4* __restrict__ normal, int normal_stride,
                                                                 const float4* __restrict__ albedo, const float4* __restrict__ depth, float4* __restrict__ dst,
                                                                 float4* __restrict__ vdst, int w, int h, int step, float kc, float ka, float kz) {
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= w || y >= h) return;
    float oe[4], ov[4];
    er_variance_level_px((const float*)src, (const float*)vsrc, (const float*)normal, (size_t)normal_stride * 4, (const float*)albedo, (const float*)depth, w, h, x, y, step, kc, ka,
                         kz, oe, ov);
    const size_t p = (size_t)y * w + x;
    dst[p] = make_float4(oe[0], oe[1], oe[2], oe[3]);
    vdst[p] = make_float4(ov[0], ov[1], ov[2], ov[3]);
}

hipError_t er_probe_variance(const char** which) {
    hipFuncAttributes a;
    hipError_t e;
    *which = "k_variance_fold (er_variance.hip)";
    if ((e = hipFuncGetAttributes(&a, (const void*)k_variance_fold)) != hipSuccess) return e;
    *which = "er_variance_level_kernel";
    return hipFuncGetAttributes(&a, (const void*)er_variance_level_kernel);
}

// ---- the entry points (host side) ----
namespace {

int need_begun(ErScene* s, const char* who) {
    if (!s->begun) return fail(ER_ERR_STATE, std::string(who) + ": er_render_begin has not succeeded");
    if (s->params.world > 1) return fail(ER_ERR_STATE, std::string(who) + ": the frame is sharded over several ranks (variance on a sharded frame: not built)");
    return ER_OK;
}

unsigned px_blocks(size_t npx) { return (unsigned)((npx + 255) / 256); }

// the state planes exist and hold the snapshot of the last restart; the stream is idle or ordered before what follows
int ensure_state(ErScene* s) {
    ErVarianceState& V = s->var;
    const size_t npx = (size_t)s->x_res * s->y_res;
    int rc;
    if (V.d_state.n < 3 * npx) {
        if ((rc = upload(V.d_state, nullptr, 3 * npx, s->stream)) != ER_OK) return rc;
        V.restarted = true;
    }
    if (V.d_counts.n < 2 * ER_VAR_COUNT_STRIDE && (rc = upload(V.d_counts, nullptr, 2 * ER_VAR_COUNT_STRIDE, s->stream)) != ER_OK) return rc;
    if (V.restarted) {
        if (npx) hipLaunchKernelGGL(k_variance_mark, dim3(px_blocks(npx)), dim3(256), 0, s->stream, (const float4*)nullptr, (const uint32_t*)nullptr, npx, V.d_state.p);
        HIP_TRY(hipGetLastError());
        V.restarted = false;
    }
    return ER_OK;
}

int fold_impl(ErScene* s) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_variance_fold: NULL scene");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = need_begun(s, "er_variance_fold")) != ER_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));      // pending asynchronous work first
    ErVarianceState& V = s->var;
    const size_t npx = (size_t)s->x_res * s->y_res;
    if ((rc = ensure_state(s)) != ER_OK) return rc;
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(hipMemsetAsync(V.d_counts.p, 0, 2 * ER_VAR_COUNT_STRIDE * sizeof(uint32_t), s->stream));
    HIP_TRY(hipEventRecord(ev.a, s->stream));
    const unsigned blocks = std::min(px_blocks(npx), std::max(1u, s->kept.cus) * 4u);      // (four workgroups per CU, a grid stride beyond)
    if (npx)
        hipLaunchKernelGGL(k_variance_fold, dim3(blocks), dim3(256), 0, s->stream, (const float4*)s->d_passes.p, (const uint32_t*)s->d_samples.p, npx, V.d_state.p,
                           V.d_counts.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.b, s->stream));
    uint32_t counts[ER_VAR_COUNT_STRIDE + 1] = {0};
    HIP_TRY(hipMemcpyAsync(counts, V.d_counts.p, sizeof(counts), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipEventElapsedTime(&V.fold_ms, ev.a, ev.b));
    V.folds++;
    V.pixels_folded = counts[0];
    V.pixels_known = counts[ER_VAR_COUNT_STRIDE];
    return er_scene_stream_status(s, "er_variance_fold");
}

int info_impl(ErScene* s, ErVarianceInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_variance_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = need_begun(s, "er_variance_info")) != ER_OK) return rc;
    const ErVarianceState& V = s->var;
    *out = ErVarianceInfo{};
    out->folds = V.folds;
    out->pixels_folded = V.pixels_folded;
    out->pixels_known = V.pixels_known;
    out->fold_ms = V.fold_ms;
    out->filter_ms = V.filter_ms;
    return ER_OK;
}

int read_impl(ErScene* s, float* dst) {
    if (!s || !dst) return fail(ER_ERR_INVALID_ARG, "er_read_variance: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = need_begun(s, "er_read_variance")) != ER_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t npx = (size_t)s->x_res * s->y_res;
    if ((rc = ensure_state(s)) != ER_OK) return rc;
    // the staging plane of er_read_pass: the lock is held from the kernel to the end of the copy
    if (s->d_plane.n < npx && (rc = upload(s->d_plane, nullptr, npx, s->stream)) != ER_OK) return rc;
    if (npx) hipLaunchKernelGGL(k_variance_value, dim3(px_blocks(npx)), dim3(256), 0, s->stream, (const float4*)s->var.d_state.p, (const uint32_t*)s->d_samples.p, npx, s->d_plane.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dst, s->d_plane.p, npx * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return er_scene_stream_status(s, "er_read_variance");
}

int denoise_impl(ErScene* s, const ErDenoiseVariance* p) {
    if (!s || !p) return fail(ER_ERR_INVALID_ARG, "er_denoise_variance: NULL argument");
    uint32_t levels;
    float kc, ka, kz;      // kc is NOT tightened per level: the propagated variance shrinks instead
    int prc;
    if ((prc = er_variance_filter_params(p, "er_denoise_variance", &levels, &kc, &ka, &kz)) != ER_OK) return prc;
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = need_begun(s, "er_denoise_variance")) != ER_OK) return rc;
    if (!s->feat.valid) return fail(ER_ERR_STATE, "er_denoise_variance: no feature planes of this scene state (er_render_features)");
    ErVarianceState& V = s->var;
    if (V.folds < 2) return fail(ER_ERR_STATE, "er_denoise_variance: fewer than two folds since the render last started over (er_variance_fold)");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t npx = (size_t)s->x_res * s->y_res;
    const int w = (int)s->x_res, h = (int)s->y_res;
    ScopedDevBuf<float4> tmp;      // four planes: colour and variance go back and forth
    if ((rc = upload(tmp, (const void*)nullptr, 4 * npx, s->stream)) != ER_OK) return rc;
    const float4* beauty = s->d_passes.p + er_pass_index(npx, ER_PASS_BEAUTY, 0);      // (interleaved passes: stride 4, er_device.h)
    const float4* normal = s->d_passes.p + er_pass_index(npx, ER_PASS_NORMAL, 0);
    float4* out = s->d_passes.p + er_pass_index(npx, ER_PASS_DENOISE, 0);
    const float4 *alb = s->d_feat.p + (size_t)ER_FEATURE_ALBEDO * npx, *dep = s->d_feat.p + (size_t)ER_FEATURE_DEPTH * npx;
    float4 *bufs[2] = {tmp.p, tmp.p + npx}, *vbufs[2] = {tmp.p + 2 * npx, tmp.p + 3 * npx};
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(hipEventRecord(ev.a, s->stream));
    if (npx) {
        hipLaunchKernelGGL(er_variance_split_kernel, dim3(px_blocks(npx)), dim3(256), 0, s->stream, beauty, 4, alb, (const float4*)V.d_state.p, (const uint32_t*)s->d_samples.p, bufs[0],
                           vbufs[0], npx);
        er_launch_variance_levels(bufs, vbufs, normal, 4, alb, dep, w, h, levels, kc, ka, kz, s->stream);
        er_launch_guided_join(bufs[levels & 1u], alb, beauty, 4, out, w, h, s->stream);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.b, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipEventElapsedTime(&V.filter_ms, ev.a, ev.b));
    return er_scene_stream_status(s, "er_denoise_variance");
}

}  // namespace

int er_variance_filter_params(const ErDenoiseVariance* p, const char* who, uint32_t* levels_out, float* kc, float* ka, float* kz) {
    uint32_t levels = p->levels;
    float sc = p->colour_sigma, sa = p->albedo_sigma, sz = p->depth_sigma;
    if (levels > 8) return fail(ER_ERR_INVALID_ARG, std::string(who) + ": at most 8 levels");
    if (!(sc >= 0) || !(sa >= 0) || !(sz >= 0)) return fail(ER_ERR_INVALID_ARG, std::string(who) + ": the sigmas must be >= 0 (and not NaN)");
    if (levels == 0) levels = 5;
    if (sc == 0) sc = 6.0f;      // (in standard errors of the pixel: the colour difference is divided by the variance; DESIGN.md 3m has the sweep)
    if (sa == 0) sa = 0.3f;
    if (sz == 0) sz = 0.2f;
    *levels_out = levels;
    *kc = 1.0f / (sc * sc); *ka = 1.0f / (sa * sa); *kz = 1.0f / (sz * sz);
    return ER_OK;
}

void er_launch_variance_levels(float4* const bufs[2], float4* const vbufs[2], const float4* normal, int normal_stride, const float4* albedo, const float4* depth, int w, int h,
                               uint32_t levels, float kc, float ka, float kz, hipStream_t stream) {
    for (uint32_t k = 0; k < levels; k++)
        hipLaunchKernelGGL(er_variance_level_kernel, dim3((w + 15) / 16, (h + 15) / 16), dim3(256), 0, stream, (const float4*)bufs[k & 1u], (const float4*)vbufs[k & 1u], normal,
                           normal_stride, albedo, depth, bufs[(k + 1) & 1u], vbufs[(k + 1) & 1u], w, h, 1 << k, kc, ka, kz);
}

int er_variance_mark_imported(ErScene* s) {
    ErVarianceState& V = s->var;
    V.reset();
    if (!s->begun || s->params.world > 1) return ER_OK;
    const size_t npx = (size_t)s->x_res * s->y_res;
    int rc;
    if (V.d_state.n < 3 * npx && (rc = upload(V.d_state, nullptr, 3 * npx, s->stream)) != ER_OK) return rc;
    if (npx) hipLaunchKernelGGL(k_variance_mark, dim3(px_blocks(npx)), dim3(256), 0, s->stream, (const float4*)s->d_passes.p, (const uint32_t*)s->d_samples.p, npx, V.d_state.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    V.restarted = false;
    return ER_OK;
}

extern "C" {
int er_variance_fold(ErScene* s) { return guarded("er_variance_fold", [&]() -> int { return fold_impl(s); }); }
int er_variance_info(ErScene* s, ErVarianceInfo* out) { return guarded("er_variance_info", [&]() -> int { return info_impl(s, out); }); }
int er_read_variance(ErScene* s, float* dst) { return guarded("er_read_variance", [&]() -> int { return read_impl(s, dst); }); }
int er_denoise_variance(ErScene* s, const ErDenoiseVariance* p) { return guarded("er_denoise_variance", [&]() -> int { return denoise_impl(s, p); }); }

// ---- include/eleven_hip_debug.h: the header's routines on caller arrays, no device ----
int er_debug_variance_mark(uint32_t count, const float* beauty, const uint32_t* samples, float* state) {
    return guarded("er_debug_variance_mark", [&]() -> int {
        if (count && (!beauty || !samples || !state)) return fail(ER_ERR_INVALID_ARG, "er_debug_variance_mark: NULL argument");
        for (size_t i = 0; i < count; i++) er_variance_mark_px(beauty + 4 * i, samples[i], state + ER_VARIANCE_WORDS * i);
        return ER_OK;
    });
}
int er_debug_variance_fold(uint32_t count, const float* beauty, const uint32_t* samples, float* state, uint32_t* folded) {
    return guarded("er_debug_variance_fold", [&]() -> int {
        if (count && (!beauty || !samples || !state)) return fail(ER_ERR_INVALID_ARG, "er_debug_variance_fold: NULL argument");
        for (size_t i = 0; i < count; i++) {
            const bool f = er_variance_fold_px(beauty + 4 * i, samples[i], state + ER_VARIANCE_WORDS * i);
            if (folded) folded[i] = f ? 1u : 0u;
        }
        return ER_OK;
    });
}
int er_debug_variance_value(uint32_t count, const float* state, const uint32_t* samples, float* out) {
    return guarded("er_debug_variance_value", [&]() -> int {
        if (count && (!state || !samples || !out)) return fail(ER_ERR_INVALID_ARG, "er_debug_variance_value: NULL argument");
        for (size_t i = 0; i < count; i++) er_variance_value_px(state + ER_VARIANCE_WORDS * i, samples[i], out + 4 * i);
        return ER_OK;
    });
}
int er_debug_variance_split(uint32_t count, const float* value, const float* albedo, float* ve) {
    return guarded("er_debug_variance_split", [&]() -> int {
        if (count && (!value || !albedo || !ve)) return fail(ER_ERR_INVALID_ARG, "er_debug_variance_split: NULL argument");
        for (size_t i = 0; i < count; i++) er_variance_split_px(value + 4 * i, albedo + 4 * i, ve + 4 * i);
        return ER_OK;
    });
}
int er_debug_variance_level_px(uint32_t w, uint32_t h, uint32_t step, float kc, float ka, float kz, const float* e, const float* ve, const float* normal, const float* albedo,
                               const float* depth, float* out_e, float* out_ve) {
    return guarded("er_debug_variance_level_px", [&]() -> int {
        if (!e || !ve || !normal || !albedo || !depth || !out_e || !out_ve) return fail(ER_ERR_INVALID_ARG, "er_debug_variance_level_px: NULL argument");
        if (w == 0 || h == 0 || w > 32768 || h > 32768 || step == 0 || step > 128) return fail(ER_ERR_INVALID_ARG, "er_debug_variance_level_px: the frame or the step is out of range");
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) {
                const size_t p = (size_t)y * w + x;
                er_variance_level_px(e, ve, normal, 4, albedo, depth, (int)w, (int)h, (int)x, (int)y, (int)step, kc, ka, kz, out_e + 4 * p, out_ve + 4 * p);
            }
        return ER_OK;
    });
}
}  // extern "C"
