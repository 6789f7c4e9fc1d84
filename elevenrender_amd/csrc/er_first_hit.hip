// er_first_hit.hip -- the mode of the first-hit camera pass (include/eleven_hip.h er_first_hit_set, er_first_hit_info),
// the ray-level hook that runs FirstHit::visible on a caller's rays (er_debug_first_hit_rays) and er_cutout.h's routines on a caller's
// arrays (er_debug_cutout_*).  The pass itself is er_first_hit.h; its four consumers keep their kernels (er_features.hip, er_ids.hip,
// er_history.hip).
#include "er_first_hit.h"

#include "../../include/eleven_hip_debug.h"

using namespace erd;
using namespace erh;

// 64 rays per workgroup, one per lane; a bounded grid walks the groups of 64 with a grid stride, so the scene's spill area serves
// (first_hit_lane: one slice per workgroup).  Nothing is counted.
__global__ __launch_bounds__(64) void er_first_hit_rays_kernel(DevScene S, const float* __restrict__ o, const float* __restrict__ d, uint32_t n, float threshold,
                                                               int32_t* __restrict__ tri_out, uint32_t* __restrict__ layers_out, float* __restrict__ dist_out,
                                                               float* __restrict__ pos_out, uint2* spill_base) {
    const FirstHit fh = first_hit_lane(S, spill_base);
    const uint32_t groups = (n + 63u) / 64u;
    for (uint32_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const uint32_t i = g * 64u + threadIdx.x;
        if (i >= n) continue;
        Ray ray;
        ray.o = f3(o[3 * (size_t)i], o[3 * (size_t)i + 1], o[3 * (size_t)i + 2]);
        ray.d = f3(d[3 * (size_t)i], d[3 * (size_t)i + 1], d[3 * (size_t)i + 2]);
        HitFull hit;
        uint32_t layers;
        bool capped;
        const int slot = fh.visible(ray, threshold, hit, layers, capped);
        F3 P = f3s(0.0f);
        float dist = 0.0f;
        if (slot >= 0) { P = hit.position; dist = length(hit.position - ray.o); }
        tri_out[i] = slot >= 0 ? (int32_t)slot_triangle(S, (uint32_t)slot) : -1;
        layers_out[i] = layers;
        dist_out[i] = dist;
        pos_out[3 * (size_t)i] = P.x; pos_out[3 * (size_t)i + 1] = P.y; pos_out[3 * (size_t)i + 2] = P.z;
    }
}

hipError_t er_probe_first_hit(const char** which) {
    hipFuncAttributes a;
    *which = "er_first_hit_rays_kernel";
    return hipFuncGetAttributes(&a, (const void*)er_first_hit_rays_kernel);
}

// ---- the entry points (host side) ----
namespace {

int set_impl(ErScene* s, const ErFirstHitParams* p) {
    if (!s || !p) return fail(ER_ERR_INVALID_ARG, "er_first_hit_set: NULL argument");
    if (p->cutouts > 1u) return fail(ER_ERR_INVALID_ARG, "er_first_hit_set: cutouts must be 0 or 1");
    if (!er_cutout_threshold_ok(p->opacity_threshold)) return fail(ER_ERR_INVALID_ARG, "er_first_hit_set: opacity_threshold must be 0 (for 0.5) or lie in (0, 1] (and not NaN)");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_first_hit_set: er_render_begin has not succeeded");
    const float t = er_cutout_threshold(p->opacity_threshold);
    if (p->cutouts == s->first_hit.cutouts && t == s->first_hit.threshold) return ER_OK;      // nothing changes, nothing is invalidated
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));      // pending asynchronous work first
    s->first_hit.cutouts = p->cutouts;
    s->first_hit.threshold = t;
    for (auto& c : s->first_hit.counts) c = 0;
    // planes and keys made under the other rule: a capture keyed under one cannot be resolved under the other
    s->feat.valid = false;
    for (auto& u : s->unpacked_feat) u.clear();
    s->ids_invalidate();
    s->history_invalidate();
    return ER_OK;
}

int info_impl(ErScene* s, ErFirstHitInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_first_hit_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_first_hit_info: er_render_begin has not succeeded");
    *out = ErFirstHitInfo{};
    out->cutouts = s->first_hit.cutouts;
    out->opacity_threshold = s->first_hit.threshold;
    if (s->first_hit.cutouts) {
        out->rays = s->first_hit.counts[ER_FH_RAYS];
        out->rays_through = s->first_hit.counts[ER_FH_THROUGH];
        out->layers_skipped = s->first_hit.counts[ER_FH_LAYERS];
        out->rays_capped = s->first_hit.counts[ER_FH_CAPPED];
        out->rays_through_to_miss = s->first_hit.counts[ER_FH_TO_MISS];
    }
    return ER_OK;
}

int rays_impl(ErScene* s, const float* origins, const float* dirs, uint32_t n, float threshold, int32_t* tri_out, uint32_t* layers_out, float* dist_out, float* pos_out) {
    if (!s || !origins || !dirs || !tri_out || !layers_out || !dist_out || !pos_out) return fail(ER_ERR_INVALID_ARG, "er_debug_first_hit_rays: NULL argument");
    if (!er_cutout_threshold_ok(threshold)) return fail(ER_ERR_INVALID_ARG, "er_debug_first_hit_rays: threshold must be 0 (for 0.5) or lie in (0, 1] (and not NaN)");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_debug_first_hit_rays: er_render_begin has not succeeded");
    if (n == 0) return ER_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));      // pending asynchronous work first
    ScopedDevBuf<float> d_o, d_d, d_pos, d_dist;
    ScopedDevBuf<int32_t> d_tri;
    ScopedDevBuf<uint32_t> d_layers;
    int rc;
    uint32_t blocks;
    if ((rc = er_first_hit_blocks(s, &blocks)) != ER_OK) return rc;
    blocks = std::min(blocks, (n + 63u) / 64u);
    if ((rc = upload(d_o, origins, (size_t)n * 3, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_d, dirs, (size_t)n * 3, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_pos, nullptr, (size_t)n * 3, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_dist, nullptr, (size_t)n, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_tri, nullptr, (size_t)n, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_layers, nullptr, (size_t)n, s->stream)) != ER_OK) return rc;
    hipLaunchKernelGGL(er_first_hit_rays_kernel, dim3(blocks), dim3(64), 0, s->stream, s->dev, (const float*)d_o.p, (const float*)d_d.p, n, er_cutout_threshold(threshold), d_tri.p,
                       d_layers.p, d_dist.p, d_pos.p, s->d_first_hit_spill.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(tri_out, d_tri.p, (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(layers_out, d_layers.p, (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(dist_out, d_dist.p, (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(pos_out, d_pos.p, (size_t)n * 12, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return er_scene_stream_status(s, "er_debug_first_hit_rays");
}

}  // namespace

extern "C" {
int er_first_hit_set(ErScene* s, const ErFirstHitParams* p) { return guarded("er_first_hit_set", [&]() -> int { return set_impl(s, p); }); }
int er_first_hit_info(ErScene* s, ErFirstHitInfo* out) { return guarded("er_first_hit_info", [&]() -> int { return info_impl(s, out); }); }
int er_debug_first_hit_rays(ErScene* s, const float* origins, const float* dirs, uint32_t n, float threshold, int32_t* tri_out, uint32_t* layers_out, float* dist_out,
                            float* pos_out) {
    return guarded("er_debug_first_hit_rays", [&]() -> int { return rays_impl(s, origins, dirs, n, threshold, tri_out, layers_out, dist_out, pos_out); });
}
int er_debug_cutout_threshold(uint32_t count, const float* t, uint32_t* ok, float* resolved) {
    return guarded("er_debug_cutout_threshold", [&]() -> int {
        if (count && (!t || !ok || !resolved)) return fail(ER_ERR_INVALID_ARG, "er_debug_cutout_threshold: NULL argument");
        for (uint32_t i = 0; i < count; i++) { ok[i] = er_cutout_threshold_ok(t[i]) ? 1u : 0u; resolved[i] = er_cutout_threshold(t[i]); }
        return ER_OK;
    });
}
int er_debug_cutout_stops(uint32_t count, const float* opacity, const float* threshold, uint32_t* out) {
    return guarded("er_debug_cutout_stops", [&]() -> int {
        if (count && (!opacity || !threshold || !out)) return fail(ER_ERR_INVALID_ARG, "er_debug_cutout_stops: NULL argument");
        for (uint32_t i = 0; i < count; i++) out[i] = er_cutout_stops(opacity[i], threshold[i]) ? 1u : 0u;
        return ER_OK;
    });
}
int er_debug_cutout_continue(uint32_t count, const float* position, const float* d, float* o_out, float* d_out) {
    return guarded("er_debug_cutout_continue", [&]() -> int {
        if (count && (!position || !d || !o_out || !d_out)) return fail(ER_ERR_INVALID_ARG, "er_debug_cutout_continue: NULL argument");
        for (uint32_t i = 0; i < count; i++) er_cutout_continue(position + 3 * (size_t)i, d + 3 * (size_t)i, o_out + 3 * (size_t)i, d_out + 3 * (size_t)i);
        return ER_OK;
    });
}
}  // extern "C"
