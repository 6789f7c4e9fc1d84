// er_history_variance.hip -- the variance carried through the reprojection history, the variance of the blend and the filter of the
// blended frame (include/eleven_hip.h er_history_variance_info, er_read_history_variance, er_read_blended_variance, er_denoise_blended;
// DESIGN.md 3n).
//
// Every kernel here is one work item per pixel around a routine of er_history_variance.h, which states the arithmetic; every plane is
// read and written as float4.  The kernels that count walk the frame with k_variance_fold's bounded grid stride: one ballot per wave and
// step summed in a register, one atomicAdd per wave and counter at the end, the counters 64 bytes apart.  They read BEAUTY, the sample
// counts, the variance state, the feature planes and the history's own planes and write planes of their own and DENOISE: a render with
// any of it in between is, bit for bit, the render without.
#include "er_history_variance.h"

#include "er_features.h"
#include "er_scene.h"

using namespace erh;

namespace {

__device__ __forceinline__ void load4(const float4* __restrict__ plane, size_t p, float* out) {
    const float4 v = plane[p];
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
}

// the pixels of one grid-stride step of a wave: false for the lanes beyond the frame (every lane of a wave takes the same number of steps)
#define ER_HV_WALK(base, npx) for (size_t base = ((size_t)blockIdx.x * 256 + (threadIdx.x & ~63u)); base < (npx); base += (size_t)gridDim.x * 256)

}  // namespace

// capture: SV of every pixel from the variance state's third plane (NULL: K = 0), the sample counts and the resolved (hist, hv) (NULL: none)
__global__ __launch_bounds__(256) void k_history_variance_capture(const float4* __restrict__ m2k, const uint32_t* __restrict__ samples, const float4* __restrict__ hist,
                                                                  const float4* __restrict__ hv, size_t npx, float4* __restrict__ sv, uint32_t* __restrict__ known) {
    uint32_t nk = 0;
    ER_HV_WALK(base, npx) {
        const size_t p = base + (threadIdx.x & 63u);
        bool k = false;
        if (p < npx) {
            // (a plane that is not there reads as zeros: K = 0, w = 0, flag 0 -- what the header makes of a NULL)
            float st[4] = {0.0f, 0.0f, 0.0f, 0.0f}, h[4] = {0.0f, 0.0f, 0.0f, 0.0f}, v[4] = {0.0f, 0.0f, 0.0f, 0.0f}, out[4];
            if (m2k) load4(m2k, p, st);
            if (hist) load4(hist, p, h);
            if (hv) load4(hv, p, v);
            k = er_hv_capture_px(st, samples[p], h[3], v, out) != 0u;
            sv[p] = make_float4(out[0], out[1], out[2], out[3]);
        }
        nk += (uint32_t)__popcll(__ballot(k));
    }
    if ((threadIdx.x & 63u) == 0u && nk) atomicAdd(known, nk);
}

// resolve with the carried plane: k_history_resolve's pixel with the taps taken once for (C, W) and SV; the five classes and the pixels
// whose HV flag is set are counted in registers
__global__ __launch_bounds__(256) void k_history_resolve_variance(const uint32_t* __restrict__ key_now, const uint32_t* __restrict__ key_old, const float4* __restrict__ cw,
                                                                  const float4* __restrict__ sv, const float* __restrict__ back, uint32_t objects, ErReprojCam cam,
                                                                  uint32_t x_res, uint32_t y_res, float tol, float4* __restrict__ hist, float4* __restrict__ hv,
                                                                  unsigned long long* __restrict__ counts, uint32_t* __restrict__ known) {
    const size_t npx = (size_t)x_res * y_res;
    uint32_t nc[ER_HC_COUNT] = {0u, 0u, 0u, 0u, 0u}, nk = 0;
    ER_HV_WALK(base, npx) {
        const size_t p = base + (threadIdx.x & 63u);
        int cls = -1;
        bool k = false;
        if (p < npx) {
            const float* kf = (const float*)key_now;
            ErHistoryKey key;
            key.hit = key_now[p];
            key.object = key_now[npx + p];
            key.dist = kf[2 * npx + p];
            key.P[0] = kf[3 * npx + p * 3]; key.P[1] = kf[3 * npx + p * 3 + 1]; key.P[2] = kf[3 * npx + p * 3 + 2];
            const bool listed = key.hit && key.object < objects;      // (ER_ID_NONE is not below any count)
            const float* B = listed ? back + (size_t)key.object * 13 : nullptr;
            const uint32_t moved = listed ? __builtin_bit_cast(uint32_t, B[12]) : 0u;
            int state[4];
            float tw[4], c4[4][4], s4[4][4], oh[4], ov[4];
            size_t q[4];
            er_history_tap_set(key, B, moved, cam, x_res, y_res, tol, key_old, key_old + npx, (const float*)key_old + 2 * npx, state, tw, q);
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const bool v = state[t] == ER_TAP_VALID;      // (q[t] is a pixel of the frame for every tap that is valid)
#pragma unroll
                for (int c = 0; c < 4; c++) { c4[t][c] = 0.0f; s4[t][c] = 0.0f; }
                if (v) { load4(cw, q[t], c4[t]); load4(sv, q[t], s4[t]); }
            }
            er_history_mean(state, tw, c4, oh);
            k = er_hv_mean(state, tw, s4, ov) != 0u;
            cls = er_history_class(key.hit, state);
            hist[p] = make_float4(oh[0], oh[1], oh[2], oh[3]);
            hv[p] = make_float4(ov[0], ov[1], ov[2], ov[3]);
        }
#pragma unroll
        for (int c = 0; c < ER_HC_COUNT; c++) nc[c] += (uint32_t)__popcll(__ballot(cls == c));
        nk += (uint32_t)__popcll(__ballot(k));
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int c = 0; c < ER_HC_COUNT; c++)
            if (nc[c]) atomicAdd(counts + c, (unsigned long long)nc[c]);
        if (nk) atomicAdd(known, nk);
    }
}

// er_read_blended_variance's plane
__global__ __launch_bounds__(256) void k_history_variance_blend(const float4* __restrict__ m2k, const uint32_t* __restrict__ samples, const float4* __restrict__ hist,
                                                                const float4* __restrict__ hv, size_t npx, float4* __restrict__ dst, uint32_t* __restrict__ known) {
    uint32_t nk = 0;
    ER_HV_WALK(base, npx) {
        const size_t p = base + (threadIdx.x & 63u);
        bool k = false;
        if (p < npx) {
            float st[4] = {0.0f, 0.0f, 0.0f, 0.0f}, h[4], v[4] = {0.0f, 0.0f, 0.0f, 0.0f}, out[4];      // (zeros for a plane that is not there, as in the capture)
            if (m2k) load4(m2k, p, st);
            load4(hist, p, h);
            if (hv) load4(hv, p, v);
            k = er_hv_blend_px(st, samples[p], h[3], v, out) != 0u;
            dst[p] = make_float4(out[0], out[1], out[2], out[3]);
        }
        nk += (uint32_t)__popcll(__ballot(k));
    }
    if ((threadIdx.x & 63u) == 0u && nk) atomicAdd(known, nk);
}

// the filter's split of the blended frame: the blend (the join's colour source), e and ve
__global__ __launch_bounds__(256) void k_history_blended_split(const float4* __restrict__ passes, const float4* __restrict__ m2k, const uint32_t* __restrict__ samples,
                                                               const float4* __restrict__ hist, const float4* __restrict__ hv, const float4* __restrict__ albedo, size_t npx,
                                                               float4* __restrict__ blend, float4* __restrict__ e, float4* __restrict__ ve, uint32_t* __restrict__ known) {
    uint32_t nk = 0;
    ER_HV_WALK(base, npx) {
        const size_t p = base + (threadIdx.x & 63u);
        bool k = false;
        if (p < npx) {
            float b[4], st[4] = {0.0f, 0.0f, 0.0f, 0.0f}, h[4], v[4] = {0.0f, 0.0f, 0.0f, 0.0f}, a[4], bl[4], vb[4], oe[4], ov[4];
            load4(passes, er_pass_index(npx, ER_PASS_BEAUTY, p), b);
            if (m2k) load4(m2k, p, st);
            load4(hist, p, h);
            if (hv) load4(hv, p, v);
            load4(albedo, p, a);
            const uint32_t n = samples[p];
            er_history_blend_px(b, n, h, bl);
            k = er_hv_blend_px(st, n, h[3], v, vb) != 0u;
            er_hv_split_px(bl, vb, a, oe, ov);
            blend[p] = make_float4(bl[0], bl[1], bl[2], bl[3]);
            e[p] = make_float4(oe[0], oe[1], oe[2], oe[3]);
            ve[p] = make_float4(ov[0], ov[1], ov[2], ov[3]);
        }
        nk += (uint32_t)__popcll(__ballot(k));
    }
    if ((threadIdx.x & 63u) == 0u && nk) atomicAdd(known, nk);
}

hipError_t er_probe_history_variance(const char** which) {
    hipFuncAttributes a;
    hipError_t e;
    *which = "k_history_resolve_variance (er_history_variance.hip)";
    if ((e = hipFuncGetAttributes(&a, (const void*)k_history_resolve_variance)) != hipSuccess) return e;
    *which = "k_history_blended_split (er_history_variance.hip)";
    return hipFuncGetAttributes(&a, (const void*)k_history_blended_split);
}

void er_launch_history_variance_capture(const float4* m2k, const uint32_t* samples, const float4* hist, const float4* hv, size_t npx, float4* sv, uint32_t* known, unsigned blocks,
                                        hipStream_t stream) {
    if (!npx || !blocks) return;
    hipLaunchKernelGGL(k_history_variance_capture, dim3(blocks), dim3(256), 0, stream, m2k, samples, hist, hv, npx, sv, known);
}

void er_launch_history_resolve_variance(const uint32_t* key_now, const uint32_t* key_old, const float4* cw, const float4* sv, const float* back, uint32_t objects,
                                        const ErReprojCam& cam, uint32_t x_res, uint32_t y_res, float tol, float4* hist, float4* hv, unsigned long long* counts, uint32_t* known,
                                        unsigned blocks, hipStream_t stream) {
    if (!x_res || !y_res || !blocks) return;
    hipLaunchKernelGGL(k_history_resolve_variance, dim3(blocks), dim3(256), 0, stream, key_now, key_old, cw, sv, back, objects, cam, x_res, y_res, tol, hist, hv, counts, known);
}

// ---- the entry points (host side) ----
namespace {

int need_begun(ErScene* s, const char* who) {
    if (!s->begun) return fail(ER_ERR_STATE, std::string(who) + ": er_render_begin has not succeeded");
    if (s->params.world > 1) return fail(ER_ERR_STATE, std::string(who) + ": the frame is sharded over several ranks (history on a sharded frame: not built)");
    return ER_OK;
}

unsigned bounded_blocks(const ErScene* s, size_t npx) { return std::min((unsigned)((npx + 255) / 256), std::max(1u, s->kept.cus) * 4u); }

// the current moments, or NULL where they count as K = 0: never allocated, or a restart that has not reached the planes yet
const float4* current_m2k(const ErScene* s, size_t npx) {
    const ErVarianceState& V = s->var;
    return (V.d_state.n >= 3 * npx && !V.restarted) ? (const float4*)V.d_state.p + 2 * npx : nullptr;
}

int info_impl(ErScene* s, ErHistoryVarianceInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_history_variance_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = need_begun(s, "er_history_variance_info")) != ER_OK) return rc;
    const ErHistoryState& H = s->hist;
    *out = ErHistoryVarianceInfo{};
    out->captured = H.captured && H.sv_captured ? 1u : 0u;
    out->resolved = H.resolved && H.hv_resolved ? 1u : 0u;
    if (out->captured) out->pixels_known_captured = H.known_captured;
    if (out->resolved) out->pixels_known_history = H.known_history;
    if (H.resolved) {
        out->pixels_known_blended = H.known_blended;
        out->filter_ms = H.blended_filter_ms;
    }
    return ER_OK;
}

// the counter of the blended pixels exists whether or not a capture carried anything
int ensure_known(ErScene* s) {
    ErHistoryState& H = s->hist;
    const size_t words = (size_t)ER_HV_KNOWN_COUNT * ER_HV_COUNT_STRIDE;
    return H.d_known.n < words ? upload(H.d_known, nullptr, words, s->stream) : ER_OK;
}

int read_impl(ErScene* s, float* dst, bool blended, const char* who) {
    if (!s || !dst) return fail(ER_ERR_INVALID_ARG, std::string(who) + ": NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = need_begun(s, who)) != ER_OK) return rc;
    ErHistoryState& H = s->hist;
    if (!H.resolved) return fail(ER_ERR_STATE, std::string(who) + ": no resolved history of this scene state (er_history_resolve)");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t npx = (size_t)s->x_res * s->y_res;
    if (!blended) {
        if (!H.hv_resolved) { memset(dst, 0, npx * sizeof(float4)); return ER_OK; }      // the capture carried nothing
        HIP_TRY(hipMemcpyAsync(dst, H.d_hv.p, npx * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        return er_scene_stream_status(s, who);
    }
    // the staging plane of er_read_pass: the lock is held from the kernel to the end of the copy
    if (s->d_plane.n < npx && (rc = upload(s->d_plane, nullptr, npx, s->stream)) != ER_OK) return rc;
    if ((rc = ensure_known(s)) != ER_OK) return rc;
    uint32_t* d_known = H.d_known.p + ER_HV_KNOWN_BLENDED * ER_HV_COUNT_STRIDE;
    uint32_t known = 0;
    HIP_TRY(hipMemsetAsync(d_known, 0, sizeof(uint32_t), s->stream));
    if (npx)
        hipLaunchKernelGGL(k_history_variance_blend, dim3(bounded_blocks(s, npx)), dim3(256), 0, s->stream, current_m2k(s, npx), (const uint32_t*)s->d_samples.p,
                           (const float4*)H.d_hist.p, H.hv_resolved ? (const float4*)H.d_hv.p : (const float4*)nullptr, npx, s->d_plane.p, d_known);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dst, s->d_plane.p, npx * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(&known, d_known, sizeof(known), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    H.known_blended = known;
    return er_scene_stream_status(s, who);
}

int denoise_impl(ErScene* s, const ErDenoiseVariance* p) {
    const char* who = "er_denoise_blended";
    if (!s || !p) return fail(ER_ERR_INVALID_ARG, "er_denoise_blended: NULL argument");
    uint32_t levels;
    float kc, ka, kz;
    int rc;
    if ((rc = er_variance_filter_params(p, who, &levels, &kc, &ka, &kz)) != ER_OK) return rc;
    std::lock_guard<std::mutex> lk(s->mtx);
    if ((rc = need_begun(s, who)) != ER_OK) return rc;
    ErHistoryState& H = s->hist;
    if (!H.resolved) return fail(ER_ERR_STATE, "er_denoise_blended: no resolved history of this scene state (er_history_resolve)");
    if (!s->feat.valid) return fail(ER_ERR_STATE, "er_denoise_blended: no feature planes of this scene state (er_render_features)");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t npx = (size_t)s->x_res * s->y_res;
    const int w = (int)s->x_res, h = (int)s->y_res;
    ScopedDevBuf<float4> tmp;      // five planes: the blend, and colour and variance going back and forth
    if ((rc = upload(tmp, (const void*)nullptr, 5 * npx, s->stream)) != ER_OK) return rc;
    if ((rc = ensure_known(s)) != ER_OK) return rc;
    const float4* normal = s->d_passes.p + er_pass_index(npx, ER_PASS_NORMAL, 0);      // (interleaved passes: stride 4, er_device.h)
    float4* out = s->d_passes.p + er_pass_index(npx, ER_PASS_DENOISE, 0);
    const float4 *alb = s->d_feat.p + (size_t)ER_FEATURE_ALBEDO * npx, *dep = s->d_feat.p + (size_t)ER_FEATURE_DEPTH * npx;
    float4 *bufs[2] = {tmp.p, tmp.p + npx}, *vbufs[2] = {tmp.p + 2 * npx, tmp.p + 3 * npx}, *blend = tmp.p + 4 * npx;
    uint32_t* d_known = H.d_known.p + ER_HV_KNOWN_BLENDED * ER_HV_COUNT_STRIDE;
    uint32_t known = 0;
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(hipMemsetAsync(d_known, 0, sizeof(uint32_t), s->stream));
    HIP_TRY(hipEventRecord(ev.a, s->stream));
    if (npx) {
        hipLaunchKernelGGL(k_history_blended_split, dim3(bounded_blocks(s, npx)), dim3(256), 0, s->stream, (const float4*)s->d_passes.p, current_m2k(s, npx),
                           (const uint32_t*)s->d_samples.p, (const float4*)H.d_hist.p, H.hv_resolved ? (const float4*)H.d_hv.p : (const float4*)nullptr, alb, npx, blend, bufs[0],
                           vbufs[0], d_known);
        er_launch_variance_levels(bufs, vbufs, normal, 4, alb, dep, w, h, levels, kc, ka, kz, s->stream);
        er_launch_guided_join(bufs[levels & 1u], alb, blend, 1, out, w, h, s->stream);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.b, s->stream));
    HIP_TRY(hipMemcpyAsync(&known, d_known, sizeof(known), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipEventElapsedTime(&H.blended_filter_ms, ev.a, ev.b));
    H.known_blended = known;
    return er_scene_stream_status(s, who);
}

}  // namespace

extern "C" {
int er_history_variance_info(ErScene* s, ErHistoryVarianceInfo* out) { return guarded("er_history_variance_info", [&]() -> int { return info_impl(s, out); }); }
int er_read_history_variance(ErScene* s, float* dst) { return guarded("er_read_history_variance", [&]() -> int { return read_impl(s, dst, false, "er_read_history_variance"); }); }
int er_read_blended_variance(ErScene* s, float* dst) { return guarded("er_read_blended_variance", [&]() -> int { return read_impl(s, dst, true, "er_read_blended_variance"); }); }
int er_denoise_blended(ErScene* s, const ErDenoiseVariance* p) { return guarded("er_denoise_blended", [&]() -> int { return denoise_impl(s, p); }); }

// ---- include/eleven_hip_debug.h: the header's routines on caller arrays, no device ----
int er_debug_history_variance_current(uint32_t count, const float* state, float* out) {
    return guarded("er_debug_history_variance_current", [&]() -> int {
        if (count && (!state || !out)) return fail(ER_ERR_INVALID_ARG, "er_debug_history_variance_current: NULL argument");
        for (size_t i = 0; i < count; i++) out[4 * i + 3] = er_hv_current_px(state + 12 * i + 8, out + 4 * i) ? 1.0f : 0.0f;
        return ER_OK;
    });
}
int er_debug_history_variance_pool(uint32_t count, const float* s_h, const float* w, const float* s_c, const float* n, float* out) {
    return guarded("er_debug_history_variance_pool", [&]() -> int {
        if (count && (!s_h || !w || !s_c || !n || !out)) return fail(ER_ERR_INVALID_ARG, "er_debug_history_variance_pool: NULL argument");
        for (size_t i = 0; i < count; i++)
            out[4 * i + 3] = er_hv_pool_px(s_h + 4 * i, s_h[4 * i + 3] != 0.0f ? 1u : 0u, w[i], s_c + 4 * i, s_c[4 * i + 3] != 0.0f ? 1u : 0u, n[i], out + 4 * i) ? 1.0f : 0.0f;
        return ER_OK;
    });
}
int er_debug_history_variance_capture(uint32_t count, const float* state, const uint32_t* samples, const float* hist, const float* hv, float* out) {
    return guarded("er_debug_history_variance_capture", [&]() -> int {
        if (count && (!samples || !out)) return fail(ER_ERR_INVALID_ARG, "er_debug_history_variance_capture: NULL argument");
        for (size_t i = 0; i < count; i++) er_hv_capture_px(state ? state + 12 * i + 8 : nullptr, samples[i], hist ? hist[4 * i + 3] : 0.0f, hv ? hv + 4 * i : nullptr, out + 4 * i);
        return ER_OK;
    });
}
int er_debug_history_variance_mean(uint32_t count, const uint32_t* tap_state, const float* tap_w, const float* tap_sv, float* out) {
    return guarded("er_debug_history_variance_mean", [&]() -> int {
        if (count && (!tap_state || !tap_w || !tap_sv || !out)) return fail(ER_ERR_INVALID_ARG, "er_debug_history_variance_mean: NULL argument");
        for (size_t i = 0; i < count; i++) {
            int state[4];
            for (int t = 0; t < 4; t++) state[t] = (int)tap_state[4 * i + t];
            er_hv_mean(state, tap_w + 4 * i, (const float(*)[4])(tap_sv + 16 * i), out + 4 * i);
        }
        return ER_OK;
    });
}
int er_debug_history_variance_taps(const float* cam, uint32_t x_res, uint32_t y_res, float tol, uint32_t count, const uint32_t* hit, const uint32_t* object, const float* P,
                                   const uint32_t* moved, const float* back, const uint32_t* old_hit, const uint32_t* old_object, const float* old_dist, const float* old_cw,
                                   const float* old_sv, float* out_rgbw, float* out_hv, uint32_t* out_state, uint32_t* out_class) {
    return guarded("er_debug_history_variance_taps", [&]() -> int {
        if (!cam || !old_hit || !old_object || !old_dist || !old_cw || !old_sv ||
            (count && (!hit || !object || !P || !moved || !back || !out_rgbw || !out_hv || !out_state || !out_class)))
            return fail(ER_ERR_INVALID_ARG, "er_debug_history_variance_taps: NULL argument");
        if (x_res == 0 || y_res == 0) return fail(ER_ERR_INVALID_ARG, "er_debug_history_variance_taps: an empty frame");
        ErReprojCam c;
        memcpy(&c, cam, sizeof(c));
        for (size_t i = 0; i < count; i++) {
            ErHistoryKey k;
            k.hit = hit[i]; k.object = object[i]; k.dist = 0.0f;
            for (int j = 0; j < 3; j++) k.P[j] = P[3 * i + j];
            int state[4];
            out_class[i] = (uint32_t)er_hv_resolve_px(k, back + 12 * i, moved[i], c, x_res, y_res, tol, old_hit, old_object, old_dist, old_cw, old_sv, out_rgbw + 4 * i,
                                                      out_hv + 4 * i, state);
            for (int t = 0; t < 4; t++) out_state[4 * i + t] = (uint32_t)state[t];
        }
        return ER_OK;
    });
}
int er_debug_history_variance_blend(uint32_t count, const float* state, const uint32_t* samples, const float* hist, const float* hv, float* out) {
    return guarded("er_debug_history_variance_blend", [&]() -> int {
        if (count && (!samples || !hist || !out)) return fail(ER_ERR_INVALID_ARG, "er_debug_history_variance_blend: NULL argument");
        for (size_t i = 0; i < count; i++) er_hv_blend_px(state ? state + 12 * i + 8 : nullptr, samples[i], hist[4 * i + 3], hv ? hv + 4 * i : nullptr, out + 4 * i);
        return ER_OK;
    });
}
int er_debug_history_variance_split(uint32_t count, const float* blend, const float* vb, const float* albedo, float* e, float* ve) {
    return guarded("er_debug_history_variance_split", [&]() -> int {
        if (count && (!blend || !vb || !albedo || !e || !ve)) return fail(ER_ERR_INVALID_ARG, "er_debug_history_variance_split: NULL argument");
        for (size_t i = 0; i < count; i++) er_hv_split_px(blend + 4 * i, vb + 4 * i, albedo + 4 * i, e + 4 * i, ve + 4 * i);
        return ER_OK;
    });
}
}  // extern "C"
