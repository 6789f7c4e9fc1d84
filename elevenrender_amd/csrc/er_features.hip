// er_features.hip -- first-hit feature planes (albedo, depth) and the a-trous filter guided by them (include/eleven_hip.h
// er_render_features, er_read_feature, er_gather_feature, er_feature_info, er_denoise_guided).
//
// The render kernels are untouched: the planes come from the stateless first-hit camera pass (er_first_hit.h, which the id pass, the
// pick and the history's key share) -- n camera rays per owned pixel through the production wide traversal -- shaded here into two
// planes of their own.  The pass neither reads nor writes the progressive state (passes, samples, RNG, counters), so a render with a
// feature pass in between is, bit for bit, the render without it.
#include "er_features.h"

#include "er_first_hit.h"
#include "er_shade.h"

using namespace erd;
using namespace erh;

// One wave per 8x8 tile, one lane per pixel; a fixed number of workgroups walks the owned tiles with a grid stride (no workgroup
// waits for or talks to another): first_hit_walk, whose handle gives the ray and its closest hit.  Per pixel idx = py * x_res + px,
// exactly these operations (-ffp-contract=off; tests/test_gpu_features.py replays them in numpy float32 from the oracle, bit for bit):
//     rs = jenkins_u32(idx + 1)                                 the value er_setup_kernel gives DevScene::rng -- which is not touched
//     A = (0, 0, 0), D = 0, hits = 0
//     for k = 0 .. n - 1:
//         c1 .. c5 = rng_next(rs), five draws, left to right     (src/kernel.cpp:492-493)
//         ray = camera_ray(cam, px, py, x_res, y_res, c1 .. c5)
//         slot = closest hit of ray through trav_run_closest (wide traversal, exact fallback: the production result)
//         hit:  full_hit; a = the albedo generate_hit_data gives (fused texel, constant, or the albedo texture through its filter),
//               then the albedo_shader_id override of er_bounce.inc; d = length(Hit.position - ray.o); hits += 1; D = D + d
//         miss: a = (1, 1, 1)
//         A_c = A_c + a_c                                        c = R, G, B
//     albedo[idx] = (A_R / (float)n, A_G / (float)n, A_B / (float)n, (float)hits / (float)n)
//     z = hits ? D / (float)hits : 0;  depth[idx] = (z, z, z, (float)hits / (float)n)
// No opacity draw is taken.  CUTOUTS = false (the default mode): the first hit counts whatever its opacity -- a path that passes
// through a cut-out shades what lies behind it, the feature planes show the cut-out's own albedo and distance.  CUTOUTS = true
// (er_first_hit_set): `slot` and `hit` are FirstHit::visible's -- the first hit whose opacity reaches the threshold x =
// (threshold, counters), or a miss -- and d is still measured from the camera ray's origin; everything else above is unchanged.
template <bool CUTOUTS, class... X>
__global__ __launch_bounds__(64) void er_features_kernel(DevScene S, uint32_t n, float4* __restrict__ albedo, float4* __restrict__ depth, uint2* spill_base, X... x) {
    static_assert(sizeof...(X) == (CUTOUTS ? 2 : 0), "the mode's threshold and counters are arguments of the mode-on instance only");
    Cutouts<CUTOUTS> co{x...};
    const float fn = (float)n;
    first_hit_walk(S, spill_base, [&](uint32_t px, uint32_t py, const FirstHit& fh) {
        const uint32_t idx = py * S.x_res + px;
        uint32_t rs = jenkins_u32(idx + 1u);
        F3 A = f3s(0.0f);
        float D = 0.0f;
        uint32_t hits = 0;
        for (uint32_t k = 0; k < n; k++) {
            const Ray ray = fh.sample_ray(px, py, rs);
            HitFull hit;
            int slot;
            if constexpr (CUTOUTS) slot = co.visible(fh, ray, hit);
            else slot = fh.closest(ray);
            F3 a = f3s(1.0f);
            if (slot >= 0) {
                if constexpr (!CUTOUTS) full_hit(S, (uint32_t)slot, ray, hit);
                const ErMaterial& mat = S.materials[hit.material];
                // the albedo branch of generate_hit_data (er_device.h) ...
                DevFused fu = {0, 0, 0, 0};
                if (S.fused_any) fu = S.mat_fused[hit.material];
                if (fu.width > 0) { F3 rm; fused_fetch(S, fu, hit.tu, hit.tv, a, rm); }
                else if (mat.albedo_tex < 0) a = f3(mat.albedo.x, mat.albedo.y, mat.albedo.z);
                else a = tex_filtered(S, S.textures[mat.albedo_tex], hit.tu, hit.tv);
                // ... and the asl_shade placeholder of er_bounce.inc
                const int shader = mat.albedo_shader_id;
                if (shader != -1) {
                    a = f3s(0.0f);
                    if (shader >= 0 && shader < 4) a = f3(1.0f, 1.0f, 0.0f);
                }
                D = D + length(hit.position - ray.o);
                hits++;
            }
            A = A + a;
        }
        const float cov = (float)hits / fn;
        const float z = hits ? D / (float)hits : 0.0f;
        albedo[idx] = make_float4(A.x / fn, A.y / fn, A.z / fn, cov);
        depth[idx] = make_float4(z, z, z, cov);
    });
    co.flush();      // (every lane arrives: the walk has no early return)
}

// pixels of the listed tiles of a row-major plane <-> compact buffer [tile][64] (er_pack_kernel / er_unpack_kernel on a plane pointer)
__global__ __launch_bounds__(64) void er_pack_plane_kernel(DevScene S, const uint32_t* __restrict__ tiles, const float4* __restrict__ plane, float4* __restrict__ dst) {
    const uint32_t lane = threadIdx.x, tile = tiles[blockIdx.x];
    const uint32_t px = (tile % S.tiles_x) * ER_TILE + (lane & 7u), py = (tile / S.tiles_x) * ER_TILE + (lane >> 3);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (px < S.x_res && py < S.y_res) v = plane[(size_t)py * S.x_res + px];
    dst[(size_t)blockIdx.x * 64 + lane] = v;
}
__global__ __launch_bounds__(64) void er_unpack_plane_kernel(DevScene S, const uint32_t* __restrict__ tiles, float4* __restrict__ plane, const float4* __restrict__ src) {
    const uint32_t lane = threadIdx.x, tile = tiles[blockIdx.x];
    const uint32_t px = (tile % S.tiles_x) * ER_TILE + (lane & 7u), py = (tile / S.tiles_x) * ER_TILE + (lane >> 3);
    if (px < S.x_res && py < S.y_res) plane[(size_t)py * S.x_res + px] = src[(size_t)blockIdx.x * 64 + lane];
}

// ---- the guided filter.  er_atrous_kernel (er_kernels.hip) on the DEMODULATED signal, with two more edge stops.  Plain IEEE float32
// and rational weights, so tests/test_gpu_features.py replays it in numpy bit for bit.  With a' = albedo.xyz + 0.01f per channel:
//     split:  e0 = (beauty.x / a'.x, beauty.y / a'.y, beauty.z / a'.z, beauty.w)
//     level k (step = 2^k, kc = 1.0f / (sc * sc) * (float)2^k, ka = 1.0f / (sa * sa), kz = 1.0f / (sz * sz), all evaluated on the host in float32),
//     per tap q of the 5x5 B3 stencil with clamped coordinates, in the order j = -2..2 (rows), i = -2..2:
//         d2 = (dx * dx + dy * dy) + dz * dz  of e - e_q          wc = 1 / (1 + kc * d2)
//         nd = the normal term of er_atrous_kernel (dot clamped at 0; 1 when both normals are zero)
//         a2 = (ax * ax + ay * ay) + az * az  of albedo - albedo_q (NOT offset)      wa = 1 / (1 + a2 * ka)
//         r  = (z - z_q) / (fmaxf(z, z_q) + 1e-6f)                wz = 1 / (1 + (r * r) * kz)
//         wgt = ((((kernel[i] * kernel[j]) * wc) * (nd * nd)) * wa) * wz
//         s_c = s_c + e_q.c * wgt;  sw = sw + wgt
//     dst = (sx / sw, sy / sw, sz / sw, e.w)
//     join:   out = (e.x * a'.x, e.y * a'.y, e.z * a'.z, beauty.w) ----
__global__ __launch_bounds__(256) void er_guided_split_kernel(const float4* __restrict__ beauty, int beauty_stride, const float4* __restrict__ albedo, float4* __restrict__ e,
                                                               size_t npx) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npx) return;
    const float4 b = beauty[i * beauty_stride], a = albedo[i];
    e[i] = make_float4(b.x / (a.x + 0.01f), b.y / (a.y + 0.01f), b.z / (a.z + 0.01f), b.w);
}
__global__ __launch_bounds__(256) void er_guided_join_kernel(const float4* __restrict__ e, const float4* __restrict__ albedo, const float4* __restrict__ beauty, int beauty_stride,
                                                              float4* __restrict__ out, size_t npx) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npx) return;
    const float4 v = e[i], a = albedo[i];
    out[i] = make_float4(v.x * (a.x + 0.01f), v.y * (a.y + 0.01f), v.z * (a.z + 0.01f), beauty[i * beauty_stride].w);
}
__global__ __launch_bounds__(256) void er_guided_level_kernel(const float4* __restrict__ src, const float4* __restrict__ normal, int normal_stride,
                                                               const float4* __restrict__ albedo, const float4* __restrict__ depth, float4* __restrict__ dst, int w, int h,
                                                               int step, float kc, float ka, float kz) {
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= w || y >= h) return;
    const float kernel[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const size_t p = (size_t)y * w + x;
    const float4 c = src[p], n = normal[p * normal_stride], a = albedo[p];
    const float z = depth[p].x;
    float sx = 0, sy = 0, sz = 0, sw = 0;
    for (int j = -2; j <= 2; j++)
        for (int i = -2; i <= 2; i++) {
            int qx = x + i * step, qy = y + j * step;
            qx = qx < 0 ? 0 : (qx >= w ? w - 1 : qx);
            qy = qy < 0 ? 0 : (qy >= h ? h - 1 : qy);
            const size_t q = (size_t)qy * w + qx;
            const float4 cq = src[q], nq = normal[q * normal_stride], aq = albedo[q];
            const float zq = depth[q].x;
            const float dx = c.x - cq.x, dy = c.y - cq.y, dz = c.z - cq.z;
            const float d2 = dx * dx + dy * dy + dz * dz;
            const float wc = 1.0f / (1.0f + kc * d2);
            float nd = n.x * nq.x + n.y * nq.y + n.z * nq.z;
            const bool none = (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f), noneq = (nq.x == 0.0f && nq.y == 0.0f && nq.z == 0.0f);
            nd = (none && noneq) ? 1.0f : (nd < 0.0f ? 0.0f : nd);
            const float ax = a.x - aq.x, ay = a.y - aq.y, az = a.z - aq.z;
            const float a2 = ax * ax + ay * ay + az * az;
            const float wa = 1.0f / (1.0f + a2 * ka);
            const float r = (z - zq) / (__builtin_fmaxf(z, zq) + 1e-6f);
            const float wz = 1.0f / (1.0f + (r * r) * kz);
            const float wgt = kernel[i + 2] * kernel[j + 2] * wc * (nd * nd) * wa * wz;
            sx = sx + cq.x * wgt; sy = sy + cq.y * wgt; sz = sz + cq.z * wgt; sw = sw + wgt;
        }
    dst[p] = make_float4(sx / sw, sy / sw, sz / sw, c.w);
}

hipError_t er_probe_features(const char** which) {
    hipFuncAttributes a;
    hipError_t e;
    *which = "er_features_kernel";
    if ((e = hipFuncGetAttributes(&a, (const void*)er_features_kernel<false>)) != hipSuccess) return e;
    *which = "er_features_kernel (cut-outs)";
    if ((e = hipFuncGetAttributes(&a, (const void*)er_features_kernel<true, float, unsigned long long*>)) != hipSuccess) return e;
    *which = "er_guided_level_kernel";
    return hipFuncGetAttributes(&a, (const void*)er_guided_level_kernel);
}

void er_launch_features(const DevScene& S, uint32_t n, float4* albedo, float4* depth, uint32_t blocks, uint2* spill, hipStream_t stream) {
    if (S.owned_tile_count == 0 || n == 0 || blocks == 0) return;
    hipLaunchKernelGGL(er_features_kernel<false>, dim3(blocks), dim3(64), 0, stream, S, n, albedo, depth, spill);
}
void er_launch_features_cutouts(const DevScene& S, uint32_t n, float4* albedo, float4* depth, uint32_t blocks, uint2* spill, float threshold, unsigned long long* counts,
                                hipStream_t stream) {
    if (S.owned_tile_count == 0 || n == 0 || blocks == 0) return;
    hipLaunchKernelGGL((er_features_kernel<true, float, unsigned long long*>), dim3(blocks), dim3(64), 0, stream, S, n, albedo, depth, spill, threshold, counts);
}
void er_launch_pack_plane(const DevScene& S, const uint32_t* tiles, uint32_t ntiles, const float4* plane, void* dst, hipStream_t stream) {
    if (ntiles == 0) return;
    hipLaunchKernelGGL(er_pack_plane_kernel, dim3(ntiles), dim3(64), 0, stream, S, tiles, plane, (float4*)dst);
}
void er_launch_unpack_plane(const DevScene& S, const uint32_t* tiles, uint32_t ntiles, float4* plane, const void* src, hipStream_t stream) {
    if (ntiles == 0) return;
    hipLaunchKernelGGL(er_unpack_plane_kernel, dim3(ntiles), dim3(64), 0, stream, S, tiles, plane, (const float4*)src);
}
void er_launch_guided_split(const float4* beauty, int beauty_stride, const float4* albedo, float4* e, int w, int h, hipStream_t stream) {
    const size_t npx = (size_t)w * h;
    if (npx == 0) return;
    hipLaunchKernelGGL(er_guided_split_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, stream, beauty, beauty_stride, albedo, e, npx);
}
void er_launch_guided_level(const float4* src, const float4* normal, int normal_stride, const float4* albedo, const float4* depth, float4* dst, int w, int h,
                            int step, float kc, float ka, float kz, hipStream_t stream) {
    hipLaunchKernelGGL(er_guided_level_kernel, dim3((w + 15) / 16, (h + 15) / 16), dim3(256), 0, stream, src, normal, normal_stride, albedo, depth, dst, w, h, step, kc, ka, kz);
}
void er_launch_guided_join(const float4* e, const float4* albedo, const float4* beauty, int beauty_stride, float4* out, int w, int h, hipStream_t stream) {
    const size_t npx = (size_t)w * h;
    if (npx == 0) return;
    hipLaunchKernelGGL(er_guided_join_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, stream, e, albedo, beauty, beauty_stride, out, npx);
}

// ---- the entry points (host side) ----
namespace {

const char* const k_feature_name[ER_FEATURE_COUNT] = {"ALBEDO", "DEPTH"};

float4* feature_plane(ErScene* s, int feature) { return s->d_feat.p + (size_t)feature * s->x_res * s->y_res; }

int features_impl(ErScene* s, uint32_t n) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_render_features: NULL scene");
    if (n > 64) return fail(ER_ERR_INVALID_ARG, "er_render_features: at most 64 samples");
    if (n == 0) n = 4;
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_render_features: er_render_begin has not succeeded");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));      // pending asynchronous work first
    int rc;
    const size_t npx = (size_t)s->x_res * s->y_res;
    uint32_t blocks;
    s->feat.valid = false;
    for (auto& u : s->unpacked_feat) u.clear();      // other ranks' pixels gathered earlier are overwritten below
    if (s->d_feat.n < 2 * npx && (rc = upload(s->d_feat, nullptr, 2 * npx, s->stream)) != ER_OK) return rc;
    if ((rc = er_first_hit_blocks(s, &blocks)) != ER_OK) return rc;
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    // pixels of other ranks read as zero until they are gathered
    HIP_TRY(hipMemsetAsync(s->d_feat.p, 0, 2 * npx * sizeof(float4), s->stream));
    const bool cutouts = er_first_hit_cutouts(s);
    if (cutouts && (rc = er_first_hit_counts_begin(s)) != ER_OK) return rc;
    HIP_TRY(hipEventRecord(ev.a, s->stream));
    if (cutouts)
        er_launch_features_cutouts(s->dev, n, feature_plane(s, ER_FEATURE_ALBEDO), feature_plane(s, ER_FEATURE_DEPTH), blocks, s->d_first_hit_spill.p, s->first_hit.threshold,
                                   s->d_first_hit_counts.p, s->stream);
    else
        er_launch_features(s->dev, n, feature_plane(s, ER_FEATURE_ALBEDO), feature_plane(s, ER_FEATURE_DEPTH), blocks, s->d_first_hit_spill.p, s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.b, s->stream));
    HIP_TRY(hipEventSynchronize(ev.b));
    if (cutouts && (rc = er_first_hit_counts_end(s)) != ER_OK) return rc;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    s->feat = {true, n, s->owned_pixels() * n, ms};      // (one camera ray per sample and owned pixel inside the frame)
    return ER_OK;
}

int feature_info_impl(ErScene* s, ErFeatureInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_feature_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_feature_info: er_render_begin has not succeeded");
    *out = ErFeatureInfo{};
    out->valid = s->feat.valid ? 1u : 0u;
    if (s->feat.valid) { out->samples = s->feat.samples; out->rays = s->feat.rays; out->ms = s->feat.ms; }
    return ER_OK;
}

int read_feature_impl(ErScene* s, int feature, float* dst) {
    if (feature < 0 || feature >= ER_FEATURE_COUNT) return fail(ER_ERR_INVALID_ARG, "er_read_feature: feature out of range");
    if (!s || !dst) return fail(ER_ERR_INVALID_ARG, "er_read_feature: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_read_feature: er_render_begin has not succeeded");
    if (!s->feat.valid) return fail(ER_ERR_STATE, "er_read_feature: no feature planes of this scene state (er_render_features)");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpyAsync(dst, feature_plane(s, feature), (size_t)s->x_res * s->y_res * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return er_scene_stream_status(s, "er_read_feature");
}

int denoise_guided_impl(ErScene* s, const ErDenoiseGuided* p) {
    if (!s || !p) return fail(ER_ERR_INVALID_ARG, "er_denoise_guided: NULL argument");
    uint32_t levels = p->levels;
    float sc = p->colour_sigma, sa = p->albedo_sigma, sz = p->depth_sigma;
    if (levels > 8) return fail(ER_ERR_INVALID_ARG, "er_denoise_guided: at most 8 levels");
    if (!(sc >= 0) || !(sa >= 0) || !(sz >= 0)) return fail(ER_ERR_INVALID_ARG, "er_denoise_guided: the sigmas must be >= 0 (and not NaN)");
    if (levels == 0) levels = 5;
    if (sc == 0) sc = 4.0f;      // (of the demodulated signal, which is up to 6 x the radiance: not er_denoise's 1)
    if (sa == 0) sa = 0.3f;
    if (sz == 0) sz = 0.2f;
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_denoise_guided: er_render_begin has not succeeded");
    if (!s->feat.valid) return fail(ER_ERR_STATE, "er_denoise_guided: no feature planes of this scene state (er_render_features)");
    if (s->params.world > 1) {      // a sharded frame: only where all four guides are whole (er_denoise)
        std::string missing;
        const uint32_t need = s->params.world - 1;
        if (s->unpacked[ER_PASS_BEAUTY].size() < need) missing += " BEAUTY";
        if (s->unpacked[ER_PASS_NORMAL].size() < need) missing += " NORMAL";
        for (int f = 0; f < ER_FEATURE_COUNT; f++)
            if (s->unpacked_feat[f].size() < need) missing += std::string(" ") + k_feature_name[f];
        if (!missing.empty())
            return fail(ER_ERR_STATE, "er_denoise_guided: the frame is sharded over several ranks; gather to this rank first (er_gather_pass, er_gather_feature):" + missing);
    }
    HIP_TRY(hipSetDevice(s->device));
    const size_t npx = (size_t)s->x_res * s->y_res;
    const int w = (int)s->x_res, h = (int)s->y_res;
    ScopedDevBuf<float4> tmp;      // two planes: the levels go back and forth
    int rc;
    if ((rc = upload(tmp, (const void*)nullptr, 2 * npx, s->stream)) != ER_OK) return rc;
    const float4* beauty = s->d_passes.p + er_pass_index(npx, ER_PASS_BEAUTY, 0);      // (interleaved passes: stride 4, er_device.h)
    const float4* normal = s->d_passes.p + er_pass_index(npx, ER_PASS_NORMAL, 0);
    float4* out = s->d_passes.p + er_pass_index(npx, ER_PASS_DENOISE, 0);
    const float4 *alb = feature_plane(s, ER_FEATURE_ALBEDO), *dep = feature_plane(s, ER_FEATURE_DEPTH);
    const float ka = 1.0f / (sa * sa), kz = 1.0f / (sz * sz);
    float4* bufs[2] = {tmp.p, tmp.p + npx};
    er_launch_guided_split(beauty, 4, alb, bufs[0], w, h, s->stream);
    for (uint32_t k = 0; k < levels; k++) {
        const float kc = 1.0f / (sc * sc) * (float)(1u << k);      // the colour edge-stop tightens with the level, as in er_denoise
        er_launch_guided_level(bufs[k & 1u], normal, 4, alb, dep, bufs[(k + 1) & 1u], w, h, 1 << k, kc, ka, kz, s->stream);
    }
    er_launch_guided_join(bufs[levels & 1u], alb, beauty, 4, out, w, h, s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    return er_scene_stream_status(s, "er_denoise_guided");
}

}  // namespace

extern "C" {
int er_render_features(ErScene* s, uint32_t n) { return guarded("er_render_features", [&]() -> int { return features_impl(s, n); }); }
int er_feature_info(ErScene* s, ErFeatureInfo* out) { return guarded("er_feature_info", [&]() -> int { return feature_info_impl(s, out); }); }
int er_read_feature(ErScene* s, int feature, float* dst) { return guarded("er_read_feature", [&]() -> int { return read_feature_impl(s, feature, dst); }); }
int er_denoise_guided(ErScene* s, const ErDenoiseGuided* p) { return guarded("er_denoise_guided", [&]() -> int { return denoise_guided_impl(s, p); }); }
}  // extern "C"
