// er_history.hip -- temporal reprojection: the key pass, the capture, the resolve and the blend (include/eleven_hip.h er_history_capture,
// er_history_resolve, er_history_info, er_read_history, er_read_blended).
//
// The key pass is the first-hit camera pass (er_first_hit.h) with one pinhole ray per pixel and the hit's position kept: the walker, the
// traversal and the id accessors of the feature and id passes, nothing of the render written.  The other three kernels are one work item
// per pixel around the routines of er_reproject.h.  So a render with a capture, a resolve and the reads in between is, bit for bit, the
// render without them.
#include "er_history.h"

#include "er_first_hit.h"

using namespace erd;
using namespace erh;

// first_hit_walk's geometry (one wave per 8x8 tile, one lane per pixel, a grid stride over the owned tiles; world == 1: all of them).
// One ray per lane: camera_ray with r1 = r2 = 0.5 and bokeh taken as 0, on the handle's trig.
// key: [0, npx) hit, [npx, 2 npx) object, [2 npx, 3 npx) dist, then P as [npx][3].
// CUTOUTS = true (er_first_hit_set): x = (threshold, counters); the hit is FirstHit::visible's, dist still from the camera ray's origin, and
// a ray that passes and then leaves the scene (or is capped) is keyed as a miss: P = the camera ray's direction.
template <bool CUTOUTS, class... X>
__global__ __launch_bounds__(64) void er_history_key_kernel(DevScene S, const uint32_t* __restrict__ tri_object, uint32_t* __restrict__ key, size_t npx, uint2* spill_base, X... x) {
    static_assert(sizeof...(X) == (CUTOUTS ? 2 : 0), "the mode's threshold and counters are arguments of the mode-on instance only");
    Cutouts<CUTOUTS> co{x...};
    ErCamera cam = S.cam;
    cam.bokeh = 0;
    float* const kf = (float*)key;
    first_hit_walk(S, spill_base, [&](uint32_t px, uint32_t py, const FirstHit& fh) {
        const size_t idx = (size_t)py * S.x_res + px;
        const Ray ray = camera_ray(cam, (int)px, (int)py, S.x_res, S.y_res, 0.5f, 0.5f, 0.0f, 0.0f, 0.0f, &fh.trig);
        HitFull h;
        int slot;
        if constexpr (CUTOUTS) slot = co.visible(fh, ray, h);
        else slot = fh.closest(ray);
        uint32_t hit = 0u, object = ER_ID_NONE;
        float dist = 0.0f;
        F3 P = ray.d;
        if (slot >= 0) {
            if constexpr (!CUTOUTS) full_hit(S, (uint32_t)slot, ray, h);
            hit = 1u;
            object = triangle_object(S, tri_object, slot_triangle(S, (uint32_t)slot));
            dist = length(h.position - ray.o);
            P = h.position;
        }
        key[idx] = hit;
        key[npx + idx] = object;
        kf[2 * npx + idx] = dist;
        kf[3 * npx + idx * 3 + 0] = P.x;
        kf[3 * npx + idx * 3 + 1] = P.y;
        kf[3 * npx + idx * 3 + 2] = P.z;
    });
    co.flush();      // (every lane arrives: the walk has no early return)
}

// capture: (C.rgb, W) of every pixel from BEAUTY, the sample counts and, if `hist` is not NULL, the resolved history
__global__ __launch_bounds__(256) void k_history_capture(const float4* __restrict__ passes, const uint32_t* __restrict__ samples, const float4* __restrict__ hist, float max_weight,
                                                         size_t npx, float4* __restrict__ cw) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npx) return;
    const float4 b = passes[er_pass_index(npx, ER_PASS_BEAUTY, p)];
    const float rgb[3] = {b.x, b.y, b.z};
    float h[4] = {0.0f, 0.0f, 0.0f, 0.0f}, out[4];
    if (hist) { const float4 v = hist[p]; h[0] = v.x; h[1] = v.y; h[2] = v.z; h[3] = v.w; }
    er_history_capture_px(rgb, samples[p], h, max_weight, out);      // (no history is (0, 0, 0, 0): the same arithmetic as NULL)
    cw[p] = make_float4(out[0], out[1], out[2], out[3]);
}

// resolve: the history of every pixel and the five class counts (one ballot per class and wave, one atomicAdd per wave and counter)
__global__ __launch_bounds__(256) void k_history_resolve(const uint32_t* __restrict__ key_now, const uint32_t* __restrict__ key_old, const float4* __restrict__ cw,
                                                         const float* __restrict__ back, uint32_t objects, ErReprojCam cam, uint32_t x_res, uint32_t y_res, float tol,
                                                         float4* __restrict__ hist, unsigned long long* __restrict__ counts) {
    const size_t npx = (size_t)x_res * y_res;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = p < npx;
    int cls = -1;
    if (in) {
        const float* kf = (const float*)key_now;
        ErHistoryKey k;
        k.hit = key_now[p];
        k.object = key_now[npx + p];
        k.dist = kf[2 * npx + p];
        k.P[0] = kf[3 * npx + p * 3]; k.P[1] = kf[3 * npx + p * 3 + 1]; k.P[2] = kf[3 * npx + p * 3 + 2];
        const bool listed = k.hit && k.object < objects;      // (ER_ID_NONE is not below any count)
        const float* B = listed ? back + (size_t)k.object * 13 : nullptr;
        const uint32_t moved = listed ? __builtin_bit_cast(uint32_t, B[12]) : 0u;
        float out[4];
        cls = er_history_resolve_px(k, B, moved, cam, x_res, y_res, tol, key_old, key_old + npx, (const float*)key_old + 2 * npx, (const float*)cw, out, nullptr);
        hist[p] = make_float4(out[0], out[1], out[2], out[3]);
    }
    const bool first = (threadIdx.x & 63u) == 0u;      // (every lane of the wave is here: no early return above)
#pragma unroll
    for (int c = 0; c < ER_HC_COUNT; c++) {
        const unsigned long long m = __ballot(cls == c);
        if (first && m) atomicAdd(counts + c, (unsigned long long)__popcll(m));
    }
}

// blend: er_read_blended's plane
__global__ __launch_bounds__(256) void k_history_blend(const float4* __restrict__ passes, const uint32_t* __restrict__ samples, const float4* __restrict__ hist, size_t npx,
                                                       float4* __restrict__ dst) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npx) return;
    const float4 b = passes[er_pass_index(npx, ER_PASS_BEAUTY, p)], v = hist[p];
    const float rgb[3] = {b.x, b.y, b.z}, h[4] = {v.x, v.y, v.z, v.w};
    float out[4];
    er_history_blend_px(rgb, samples[p], h, out);
    dst[p] = make_float4(out[0], out[1], out[2], out[3]);
}

hipError_t er_probe_history(const char** which) {
    hipFuncAttributes a;
    hipError_t e;
    *which = "er_history_key_kernel";
    if ((e = hipFuncGetAttributes(&a, (const void*)er_history_key_kernel<false>)) != hipSuccess) return e;
    *which = "er_history_key_kernel (cut-outs)";
    if ((e = hipFuncGetAttributes(&a, (const void*)er_history_key_kernel<true, float, unsigned long long*>)) != hipSuccess) return e;
    *which = "k_history_resolve (er_history.hip)";
    return hipFuncGetAttributes(&a, (const void*)k_history_resolve);
}

// ---- the entry points (host side) ----
namespace {

ErReprojCam reproj_cam(const ErCamera& c) {
    const CamTrig t = camera_trig(c);
    ErReprojCam r;
    r.pos[0] = c.position.x; r.pos[1] = c.position.y; r.pos[2] = c.position.z;
    r.sensor_w = c.sensor_width; r.sensor_h = c.sensor_height; r.focal = c.focal_length;
    r.cx = t.cx; r.sx = t.sx; r.cy = t.cy; r.sy = t.sy; r.cz = t.cz; r.sz = t.sz;
    return r;
}

int need_begun(ErScene* s, const char* who) {
    if (!s->begun) return fail(ER_ERR_STATE, std::string(who) + ": er_render_begin has not succeeded");
    if (s->params.world > 1) return fail(ER_ERR_STATE, std::string(who) + ": the frame is sharded over several ranks (history needs the old pixels of other ranks: not built)");
    return ER_OK;
}

size_t key_words(size_t npx) { return 6 * npx; }

// k_variance_fold's grid: four workgroups per CU, a grid stride beyond
unsigned bounded_blocks(const ErScene* s, size_t npx) { return std::min((unsigned)((npx + 255) / 256), std::max(1u, s->kept.cus) * 4u); }

// the key plane of the scene as it is now into key[now]; the stream is idle
int make_key(ErScene* s) {
    ErHistoryState& H = s->hist;
    int rc;
    const size_t npx = (size_t)s->x_res * s->y_res;
    uint32_t blocks;
    H.key_valid = false;
    if ((rc = er_first_hit_blocks(s, &blocks)) != ER_OK || (rc = er_id_prepare(s)) != ER_OK) return rc;
    const bool cutouts = er_first_hit_cutouts(s);
    if (cutouts && (rc = er_first_hit_counts_begin(s)) != ER_OK) return rc;
    if (s->dev.owned_tile_count) {
        if (cutouts)
            hipLaunchKernelGGL((er_history_key_kernel<true, float, unsigned long long*>), dim3(blocks), dim3(64), 0, s->stream, s->dev, er_id_map(s), H.d_key[H.now].p, npx,
                               s->d_first_hit_spill.p, s->first_hit.threshold, s->d_first_hit_counts.p);
        else
            hipLaunchKernelGGL(er_history_key_kernel<false>, dim3(blocks), dim3(64), 0, s->stream, s->dev, er_id_map(s), H.d_key[H.now].p, npx, s->d_first_hit_spill.p);
    }
    HIP_TRY(hipGetLastError());
    if (cutouts && (rc = er_first_hit_counts_end(s)) != ER_OK) return rc;      // (waits for the pass; with the mode off nothing waits here)
    H.key_cam = s->camera;
    H.key_m = s->objects.last_m;
    H.key_valid = true;
    return ER_OK;
}

bool key_current(const ErScene* s) {
    const ErHistoryState& H = s->hist;
    return H.key_valid && memcmp(&H.key_cam, &s->camera, sizeof(ErCamera)) == 0 && H.key_m.size() == s->objects.last_m.size() &&
           (H.key_m.empty() || memcmp(H.key_m.data(), s->objects.last_m.data(), H.key_m.size() * sizeof(float)) == 0);
}

int capture_impl(ErScene* s, const ErHistoryParams* p) {
    if (!s || !p) return fail(ER_ERR_INVALID_ARG, "er_history_capture: NULL argument");
    if (!(p->depth_tolerance >= 0) || !(p->max_weight >= 0)) return fail(ER_ERR_INVALID_ARG, "er_history_capture: a parameter is negative or NaN");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = need_begun(s, "er_history_capture")) != ER_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));      // pending asynchronous work first
    ErHistoryState& H = s->hist;
    const size_t npx = (size_t)s->x_res * s->y_res;
    for (int k = 0; k < 2; k++)
        if (H.d_key[k].n < key_words(npx) && (rc = upload(H.d_key[k], nullptr, key_words(npx), s->stream)) != ER_OK) return rc;
    if (H.d_cw.n < npx && (rc = upload(H.d_cw, nullptr, npx, s->stream)) != ER_OK) return rc;
    if (H.d_hist.n < npx && (rc = upload(H.d_hist, nullptr, npx, s->stream)) != ER_OK) return rc;
    if (H.d_counts.n < ER_HC_COUNT && (rc = upload(H.d_counts, nullptr, ER_HC_COUNT, s->stream)) != ER_OK) return rc;
    // the carried variance (er_history_variance.hip): only a scene whose variance state exists pays for the two planes and the kernel
    const bool carry = s->var.d_state.n >= 3 * npx && npx > 0;
    if (carry) {
        if (H.d_sv.n < npx && (rc = upload(H.d_sv, nullptr, npx, s->stream)) != ER_OK) return rc;
        if (H.d_hv.n < npx && (rc = upload(H.d_hv, nullptr, npx, s->stream)) != ER_OK) return rc;
        if (H.d_known.n < ER_HV_KNOWN_COUNT * ER_HV_COUNT_STRIDE && (rc = upload(H.d_known, nullptr, ER_HV_KNOWN_COUNT * ER_HV_COUNT_STRIDE, s->stream)) != ER_OK) return rc;
    }
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    H.captured = false;
    H.sv_captured = false;
    HIP_TRY(hipEventRecord(ev.a, s->stream));
    if (!key_current(s) && (rc = make_key(s)) != ER_OK) return rc;
    if (npx)
        hipLaunchKernelGGL(k_history_capture, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s->stream, (const float4*)s->d_passes.p, (const uint32_t*)s->d_samples.p,
                           H.resolved ? (const float4*)H.d_hist.p : (const float4*)nullptr, p->max_weight > 0 ? p->max_weight : 32.0f, npx, H.d_cw.p);
    uint32_t known = 0;
    if (carry) {
        // a pending restart has not reached the planes yet: they hold the moments of the frame before the edit, and K = 0 is what counts
        const float4* m2k = s->var.restarted ? (const float4*)nullptr : (const float4*)s->var.d_state.p + 2 * npx;
        uint32_t* d_known = H.d_known.p + ER_HV_KNOWN_CAPTURED * ER_HV_COUNT_STRIDE;
        HIP_TRY(hipMemsetAsync(d_known, 0, sizeof(uint32_t), s->stream));
        er_launch_history_variance_capture(m2k, (const uint32_t*)s->d_samples.p, H.resolved ? (const float4*)H.d_hist.p : (const float4*)nullptr,
                                           H.resolved && H.hv_resolved ? (const float4*)H.d_hv.p : (const float4*)nullptr, npx, H.d_sv.p, d_known, bounded_blocks(s, npx), s->stream);
        HIP_TRY(hipMemcpyAsync(&known, d_known, sizeof(known), hipMemcpyDeviceToHost, s->stream));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.b, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipEventElapsedTime(&H.capture_ms, ev.a, ev.b));
    H.sv_captured = carry;
    H.known_captured = known;
    H.hv_resolved = false;
    H.known_history = H.known_blended = 0;
    // the key made for "now" becomes the captured one: the next resolve writes the other plane
    H.now = 1 - H.now;
    H.key_valid = false;
    H.cap_cam = s->camera;
    H.cap_m = s->objects.last_m;
    H.tol = p->depth_tolerance > 0 ? p->depth_tolerance : 0.02f;
    H.max_weight = p->max_weight > 0 ? p->max_weight : 32.0f;
    H.resolved = false;      // (the history went into C: it is of the frame before this capture)
    H.captured = true;
    return er_scene_stream_status(s, "er_history_capture");
}

int resolve_impl(ErScene* s) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_history_resolve: NULL scene");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = need_begun(s, "er_history_resolve")) != ER_OK) return rc;
    ErHistoryState& H = s->hist;
    if (!H.captured) return fail(ER_ERR_STATE, "er_history_resolve: no capture is held (er_history_capture; a geometry, look, topology or object-table edit drops it)");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t npx = (size_t)s->x_res * s->y_res;
    // the back matrices: one small table per resolve
    const uint32_t objects = s->objects.objects();
    if (H.cap_m.size() != (size_t)objects * 12) return fail(ER_ERR_STATE, "er_history_resolve: the object table is not the captured one");
    std::vector<float> table((size_t)objects * 13, 0.0f);
    uint32_t moved_objects = 0;
    for (uint32_t o = 0; o < objects; o++) {
        const float *mc = &H.cap_m[(size_t)o * 12], *mn = &s->objects.last_m[(size_t)o * 12];
        const bool moved = !er_history_same_pose(mc, mn);
        if (moved && !er_history_back_matrix(mc, mn, &table[(size_t)o * 13])) return fail(ER_ERR_STATE, "er_history_resolve: a pose of object " + std::to_string(o) + " cannot be inverted");
        const uint32_t flag = moved ? 1u : 0u;
        memcpy(&table[(size_t)o * 13 + 12], &flag, 4);
        moved_objects += flag;
    }
    if (objects && (H.d_back.n < table.size()) && (rc = upload(H.d_back, nullptr, table.size(), s->stream)) != ER_OK) return rc;
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    H.resolved = false;
    H.hv_resolved = false;
    const bool carry = H.sv_captured && npx > 0;      // the held capture carries SV: one kernel takes the taps once for both planes
    uint32_t* d_known = carry ? H.d_known.p + ER_HV_KNOWN_HISTORY * ER_HV_COUNT_STRIDE : nullptr;
    HIP_TRY(hipEventRecord(ev.a, s->stream));
    if (objects) HIP_TRY(hipMemcpyAsync(H.d_back.p, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemsetAsync(H.d_counts.p, 0, ER_HC_COUNT * sizeof(unsigned long long), s->stream));
    if (carry) HIP_TRY(hipMemsetAsync(d_known, 0, sizeof(uint32_t), s->stream));
    if ((rc = make_key(s)) != ER_OK) return rc;
    if (carry)
        er_launch_history_resolve_variance((const uint32_t*)H.d_key[H.now].p, (const uint32_t*)H.d_key[1 - H.now].p, (const float4*)H.d_cw.p, (const float4*)H.d_sv.p,
                                           (const float*)H.d_back.p, objects, reproj_cam(H.cap_cam), s->x_res, s->y_res, H.tol, H.d_hist.p, H.d_hv.p, H.d_counts.p, d_known,
                                           bounded_blocks(s, npx), s->stream);
    else if (npx)
        hipLaunchKernelGGL(k_history_resolve, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s->stream, (const uint32_t*)H.d_key[H.now].p, (const uint32_t*)H.d_key[1 - H.now].p,
                           (const float4*)H.d_cw.p, (const float*)H.d_back.p, objects, reproj_cam(H.cap_cam), s->x_res, s->y_res, H.tol, H.d_hist.p, H.d_counts.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.b, s->stream));
    unsigned long long counts[ER_HC_COUNT] = {0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(counts, H.d_counts.p, sizeof(counts), hipMemcpyDeviceToHost, s->stream));
    uint32_t known = 0;
    if (carry) HIP_TRY(hipMemcpyAsync(&known, d_known, sizeof(known), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));      // (`table` goes out of scope)
    HIP_TRY(hipEventElapsedTime(&H.resolve_ms, ev.a, ev.b));
    for (int c = 0; c < ER_HC_COUNT; c++) H.classes[c] = counts[c];
    H.moved_objects = moved_objects;
    H.resolved = true;
    H.hv_resolved = carry;
    H.known_history = known;
    H.known_blended = 0;
    return er_scene_stream_status(s, "er_history_resolve");
}

int info_impl(ErScene* s, ErHistoryInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_history_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = need_begun(s, "er_history_info")) != ER_OK) return rc;
    const ErHistoryState& H = s->hist;
    *out = ErHistoryInfo{};
    out->captured = H.captured ? 1u : 0u;
    out->resolved = H.resolved ? 1u : 0u;
    if (H.captured) out->capture_ms = H.capture_ms;
    if (H.resolved) {
        out->moved_objects = H.moved_objects;
        out->pixels_valid = H.classes[ER_HC_VALID]; out->pixels_partial = H.classes[ER_HC_PARTIAL]; out->pixels_offscreen = H.classes[ER_HC_OFFSCREEN];
        out->pixels_rejected = H.classes[ER_HC_REJECTED]; out->pixels_sky = H.classes[ER_HC_SKY];
        out->resolve_ms = H.resolve_ms;
    }
    return ER_OK;
}

int read_impl(ErScene* s, float* dst, bool blended, const char* who) {
    if (!s || !dst) return fail(ER_ERR_INVALID_ARG, std::string(who) + ": NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = need_begun(s, who)) != ER_OK) return rc;
    ErHistoryState& H = s->hist;
    if (!H.resolved) return fail(ER_ERR_STATE, std::string(who) + ": no resolved history of this scene state (er_history_resolve)");
    HIP_TRY(hipSetDevice(s->device));
    const size_t npx = (size_t)s->x_res * s->y_res;
    const float4* src = H.d_hist.p;
    if (blended) {
        // the staging plane of er_read_pass: the lock is held from the kernel to the end of the copy
        if (s->d_plane.n < npx && (rc = upload(s->d_plane, nullptr, npx, s->stream)) != ER_OK) return rc;
        if (npx)
            hipLaunchKernelGGL(k_history_blend, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s->stream, (const float4*)s->d_passes.p, (const uint32_t*)s->d_samples.p,
                               (const float4*)H.d_hist.p, npx, s->d_plane.p);
        HIP_TRY(hipGetLastError());
        src = s->d_plane.p;
    }
    HIP_TRY(hipMemcpyAsync(dst, src, npx * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return er_scene_stream_status(s, who);
}

}  // namespace

extern "C" {
int er_history_capture(ErScene* s, const ErHistoryParams* p) { return guarded("er_history_capture", [&]() -> int { return capture_impl(s, p); }); }
int er_history_resolve(ErScene* s) { return guarded("er_history_resolve", [&]() -> int { return resolve_impl(s); }); }
int er_history_info(ErScene* s, ErHistoryInfo* out) { return guarded("er_history_info", [&]() -> int { return info_impl(s, out); }); }
int er_read_history(ErScene* s, float* dst) { return guarded("er_read_history", [&]() -> int { return read_impl(s, dst, false, "er_read_history"); }); }
int er_read_blended(ErScene* s, float* dst) { return guarded("er_read_blended", [&]() -> int { return read_impl(s, dst, true, "er_read_blended"); }); }

// ---- include/eleven_hip_debug.h: the header's routines on caller arrays, no device ----
int er_debug_history_camera(const void* camera, float* out) {
    return guarded("er_debug_history_camera", [&]() -> int {
        if (!camera || !out) return fail(ER_ERR_INVALID_ARG, "er_debug_history_camera: NULL argument");
        const ErReprojCam c = reproj_cam(*(const ErCamera*)camera);
        memcpy(out, &c, sizeof(c));
        return ER_OK;
    });
}
int er_debug_history_project(const float* cam, uint32_t x_res, uint32_t y_res, uint32_t count, const float* points, float* out_xy, uint32_t* out_ok) {
    return guarded("er_debug_history_project", [&]() -> int {
        if (!cam || (count && (!points || !out_xy || !out_ok))) return fail(ER_ERR_INVALID_ARG, "er_debug_history_project: NULL argument");
        ErReprojCam c;
        memcpy(&c, cam, sizeof(c));
        for (size_t i = 0; i < count; i++) out_ok[i] = er_history_project(c, x_res, y_res, points + 3 * i, out_xy + 2 * i, out_xy + 2 * i + 1) ? 1u : 0u;
        return ER_OK;
    });
}
int er_debug_history_back_matrix(const float* m_capture, const float* m_now, float* out) {
    return guarded("er_debug_history_back_matrix", [&]() -> int {
        if (!m_capture || !m_now || !out) return fail(ER_ERR_INVALID_ARG, "er_debug_history_back_matrix: NULL argument");
        if (!er_history_back_matrix(m_capture, m_now, out)) return fail(ER_ERR_INVALID_ARG, "er_debug_history_back_matrix: an entry is not finite, or det(L_now) is not > 0");
        return ER_OK;
    });
}
int er_debug_history_taps(const float* cam, uint32_t x_res, uint32_t y_res, float tol, uint32_t count, const uint32_t* hit, const uint32_t* object, const float* P,
                          const uint32_t* moved, const float* back, const uint32_t* old_hit, const uint32_t* old_object, const float* old_dist, const float* old_cw,
                          float* out_rgbw, uint32_t* out_state, uint32_t* out_class) {
    return guarded("er_debug_history_taps", [&]() -> int {
        if (!cam || !old_hit || !old_object || !old_dist || !old_cw || (count && (!hit || !object || !P || !moved || !back || !out_rgbw || !out_state || !out_class)))
            return fail(ER_ERR_INVALID_ARG, "er_debug_history_taps: NULL argument");
        if (x_res == 0 || y_res == 0) return fail(ER_ERR_INVALID_ARG, "er_debug_history_taps: an empty frame");
        ErReprojCam c;
        memcpy(&c, cam, sizeof(c));
        for (size_t i = 0; i < count; i++) {
            ErHistoryKey k;
            k.hit = hit[i]; k.object = object[i]; k.dist = 0.0f;
            for (int j = 0; j < 3; j++) k.P[j] = P[3 * i + j];
            int state[4];
            out_class[i] = (uint32_t)er_history_resolve_px(k, back + 12 * i, moved[i], c, x_res, y_res, tol, old_hit, old_object, old_dist, old_cw, out_rgbw + 4 * i, state);
            for (int t = 0; t < 4; t++) out_state[4 * i + t] = (uint32_t)state[t];
        }
        return ER_OK;
    });
}
int er_debug_history_capture(uint32_t count, const float* beauty, const uint32_t* samples, const float* hist, float max_weight, float* out) {
    return guarded("er_debug_history_capture", [&]() -> int {
        if (count && (!beauty || !samples || !out)) return fail(ER_ERR_INVALID_ARG, "er_debug_history_capture: NULL argument");
        for (size_t i = 0; i < count; i++) er_history_capture_px(beauty + 4 * i, samples[i], hist ? hist + 4 * i : nullptr, max_weight, out + 4 * i);
        return ER_OK;
    });
}
int er_debug_history_blend(uint32_t count, const float* beauty, const uint32_t* samples, const float* hist, float* out) {
    return guarded("er_debug_history_blend", [&]() -> int {
        if (count && (!beauty || !samples || !hist || !out)) return fail(ER_ERR_INVALID_ARG, "er_debug_history_blend: NULL argument");
        for (size_t i = 0; i < count; i++) er_history_blend_px(beauty + 4 * i, samples[i], hist + 4 * i, out + 4 * i);
        return ER_OK;
    });
}
}  // extern "C"
