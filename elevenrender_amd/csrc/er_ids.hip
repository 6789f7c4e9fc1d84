// er_ids.hip -- the first-hit id pass and its three consumers (include/eleven_hip.h er_render_ids, er_id_info, er_read_ids,
// er_id_matte, er_pick_rect, er_pick; er_gather_ids is er_collective.cpp's).
//
// The pass is the first-hit camera pass (er_first_hit.h) with the ids of the hits kept: the rays of the feature pass (er_features.hip),
// nothing of the render read or written.  So a render with an id pass, a matte, a selection or a pick in between is, bit for bit, the
// render without them.
#include "er_ids.h"

#include "er_first_hit.h"

using namespace erd;
using namespace erh;

#define ER_ID_MAX_RAYS 64u
static_assert(ER_ID_SLOTS == 4, "a pixel's slots are one uint4 per plane");

// first_hit_walk and FirstHit's two operations (er_first_hit.h) RESTATED: as a body of the walker this kernel had the same loops,
// registers and LDS and ran 1.7-2.3 % slower at 1080p (profiles/first_hit_refactor_ab.log; cause not found), so it keeps its own text
// and shares the trig, the id accessors and the constants.  Whoever changes the walker, sample_ray or closest changes this kernel with
// them (tests/test_gpu_first_hit.py and test_gpu_ids.py compare them bit for bit).  Per pixel idx = py * x_res + px the feature pass's rays:
//     rs = jenkins_u32(idx + 1);  for k = 0 .. n - 1:  c1 .. c5 = rng_next(rs);  ray = camera_ray(...);  slot = trav_run_closest(ray)
// A lane keeps the record slots of its rays that hit in its own column of s_slot ([k][lane]: 16 KB, conflict-free, and no other lane
// ever touches the column, so no barrier).  Once its n rays are traced the exact routine's stack (s_stack2, ER_STACK words per lane in
// the same [k][lane] layout) is idle: the lane writes the ids of one kind there and ranks them with er_id_rank (er_ids.h), kind after
// kind.  planes: [2 * kind] ids, [2 * kind + 1] counts, npx uint4 each.
// CUTOUTS = true (er_first_hit_set): x = (threshold, counters) and FirstHit::visible RESTATED too -- the ray goes on through hits whose
// opacity is below the threshold by er_cutout.h's two routines, at most S.max_bounces hits; the slot kept is the stopping hit's.
template <bool CUTOUTS, class... X>
__global__ __launch_bounds__(64) void er_ids_kernel(DevScene S, uint32_t n, const uint32_t* __restrict__ tri_object, uint4* __restrict__ planes, size_t npx,
                                                    uint32_t* __restrict__ overflow, uint2* spill_base, X... x) {
    static_assert(sizeof...(X) == (CUTOUTS ? 2 : 0), "the mode's threshold and counters are arguments of the mode-on instance only");
    Cutouts<CUTOUTS> co{x...};
    __shared__ uint2 s_stack[WF_LDS_STACK * 64];
    __shared__ int s_stack2[ER_STACK * 64];
    __shared__ uint32_t s_slot[ER_ID_MAX_RAYS * 64];
    const uint32_t lane = threadIdx.x;
    uint2* stack = s_stack + lane;
    uint2* spill = spill_base + (size_t)blockIdx.x * ER_FIRST_HIT_SPILL_PER_BLOCK + lane;
    int* stack2 = s_stack2 + lane;
    uint32_t* slots = s_slot + lane;
    static_assert(ER_STACK >= (int)ER_ID_MAX_RAYS, "er_ids_kernel ranks a lane's ids in the exact routine's stack words, one per ray");
    uint32_t* col = (uint32_t*)s_stack2 + lane;
    CamTrig trig;
    scene_cam_trig(S, trig);
    if (n > ER_ID_MAX_RAYS) n = ER_ID_MAX_RAYS;      // (the entry point refuses more: the columns hold this many)
    for (uint32_t t = blockIdx.x; t < S.owned_tile_count; t += gridDim.x) {
        const uint32_t tile = S.owned_tiles[t];
        const uint32_t px = (tile % S.tiles_x) * ER_TILE + (lane & 7u), py = (tile / S.tiles_x) * ER_TILE + (lane >> 3);
        if (px >= S.x_res || py >= S.y_res) continue;
        const uint32_t idx = py * S.x_res + px;
        uint32_t rs = jenkins_u32(idx + 1u);
        uint32_t m = 0;
        for (uint32_t k = 0; k < n; k++) {
            const float c1 = rng_next(rs), c2 = rng_next(rs), c3 = rng_next(rs), c4 = rng_next(rs), c5 = rng_next(rs);
            const Ray ray = camera_ray(S.cam, (int)px, (int)py, S.x_res, S.y_res, c1, c2, c3, c4, c5, &trig);
            int info;
            unsigned cn = 0, ct = 0;
            int slot;
            if constexpr (CUTOUTS) {
                Ray seg = ray;
                uint32_t layers = 0;
                bool capped = true;
                slot = -1;
                for (uint32_t b = 0; b < S.max_bounces; b++) {
                    const int found = trav_run_closest<false>(S, stack, spill, stack2, seg, __builtin_inff(), info, cn, ct);
                    if (found < 0) { capped = false; break; }
                    HitFull hit;
                    full_hit(S, (uint32_t)found, seg, hit);
                    if (er_cutout_stops(hit_opacity(S, hit), co.threshold)) { slot = found; capped = false; break; }
                    layers++;
                    seg = cutout_continue(hit, seg);
                }
                co.tally(slot, layers, capped);
            } else {
                slot = trav_run_closest<false>(S, stack, spill, stack2, ray, __builtin_inff(), info, cn, ct);
            }
            if (slot >= 0) { slots[m * 64] = (uint32_t)slot; m++; }
        }
        uint32_t oi[ER_ID_SLOTS], oc[ER_ID_SLOTS];
        // TRIANGLE
        for (uint32_t j = 0; j < m; j++) col[j * 64] = slot_triangle(S, slots[j * 64]);
        uint32_t distinct = er_id_rank(col, 64, m, oi, oc);
        planes[(size_t)(2 * ER_ID_TRIANGLE) * npx + idx] = make_uint4(oi[0], oi[1], oi[2], oi[3]);
        planes[(size_t)(2 * ER_ID_TRIANGLE + 1) * npx + idx] = make_uint4(oc[0], oc[1], oc[2], oc[3]);
        if (distinct > ER_ID_SLOTS) atomicAdd(overflow + ER_ID_TRIANGLE, 1u);
        // OBJECT: the column holds the triangles
        for (uint32_t j = 0; j < m; j++) col[j * 64] = triangle_object(S, tri_object, col[j * 64]);
        distinct = er_id_rank(col, 64, m, oi, oc);
        planes[(size_t)(2 * ER_ID_OBJECT) * npx + idx] = make_uint4(oi[0], oi[1], oi[2], oi[3]);
        planes[(size_t)(2 * ER_ID_OBJECT + 1) * npx + idx] = make_uint4(oc[0], oc[1], oc[2], oc[3]);
        if (distinct > ER_ID_SLOTS) atomicAdd(overflow + ER_ID_OBJECT, 1u);
        // MATERIAL
        for (uint32_t j = 0; j < m; j++) col[j * 64] = slot_material(S, slots[j * 64]);
        distinct = er_id_rank(col, 64, m, oi, oc);
        planes[(size_t)(2 * ER_ID_MATERIAL) * npx + idx] = make_uint4(oi[0], oi[1], oi[2], oi[3]);
        planes[(size_t)(2 * ER_ID_MATERIAL + 1) * npx + idx] = make_uint4(oc[0], oc[1], oc[2], oc[3]);
        if (distinct > ER_ID_SLOTS) atomicAdd(overflow + ER_ID_MATERIAL, 1u);
    }
    co.flush();      // (every lane arrives: the loop above has no early return)
}

// er_pick: ray 0 of pixel (px, py) on lane 0 of one wave; `out` takes the ten words of an ErPick.  CUTOUTS = true: x = (threshold), the
// hit is FirstHit::visible's, the distance still from the camera ray's origin; nothing is counted.
template <bool CUTOUTS, class... X>
__global__ __launch_bounds__(64) void er_pick_kernel(DevScene S, uint32_t px, uint32_t py, const uint32_t* __restrict__ tri_object, uint32_t* __restrict__ out, uint2* spill_base,
                                                     X... x) {
    static_assert(sizeof...(X) == (CUTOUTS ? 1 : 0), "the mode's threshold is an argument of the mode-on instance only");
    if (threadIdx.x != 0 || px >= S.x_res || py >= S.y_res) return;
    const FirstHit fh = first_hit_lane(S, spill_base);      // (lane 0 of workgroup 0: the first column of the one slice)
    uint32_t rs = jenkins_u32(py * S.x_res + px + 1u);
    const Ray ray = fh.sample_ray(px, py, rs);
    HitFull hit;
    int slot;
    if constexpr (CUTOUTS) {
        Cutouts<true> co{x...};
        slot = co.visible(fh, ray, hit);
    } else {
        slot = fh.closest(ray);
    }
    uint32_t w[10] = {0u, ER_ID_NONE, ER_ID_NONE, ER_ID_NONE, 0u, 0u, 0u, 0u, 0u, 0u};
    if (slot >= 0) {
        if constexpr (!CUTOUTS) full_hit(S, (uint32_t)slot, ray, hit);
        w[0] = 1u;
        w[1] = slot_triangle(S, (uint32_t)slot);
        w[2] = triangle_object(S, tri_object, w[1]);
        w[3] = (uint32_t)hit.material;
        w[4] = __builtin_bit_cast(uint32_t, length(hit.position - ray.o));
        w[5] = __builtin_bit_cast(uint32_t, hit.position.x);
        w[6] = __builtin_bit_cast(uint32_t, hit.position.y);
        w[7] = __builtin_bit_cast(uint32_t, hit.position.z);
        w[8] = __builtin_bit_cast(uint32_t, hit.tu);
        w[9] = __builtin_bit_cast(uint32_t, hit.tv);
    }
    for (int i = 0; i < 10; i++) out[i] = w[i];
}
static_assert(sizeof(ErPick) == 10 * 4, "er_pick_kernel writes an ErPick word by word");

// tri -> object: the map is ER_ID_NONE everywhere (hipMemset 0xFF), then one work item per listed id; the table is disjoint, so every
// word has one writer
__global__ __launch_bounds__(256) void k_id_map_scatter(uint32_t total, uint32_t objects, const uint32_t* __restrict__ first, const uint32_t* __restrict__ tri_ids,
                                                        uint32_t tri_count, uint32_t* __restrict__ map) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    const uint32_t tri = tri_ids[j];
    if (tri < tri_count) map[tri] = er_id_object_of(first, objects, j);
}

// er_id_matte: one work item per pixel, membership by bisection over the ascending, duplicate-free list
__global__ __launch_bounds__(256) void k_id_matte(const uint4* __restrict__ ids, const uint4* __restrict__ counts, size_t npx, const uint32_t* __restrict__ list, uint32_t count,
                                                  uint32_t n, float* __restrict__ dst) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npx) return;
    const uint4 a = ids[p], c = counts[p];
    const uint32_t si[ER_ID_SLOTS] = {a.x, a.y, a.z, a.w}, sc[ER_ID_SLOTS] = {c.x, c.y, c.z, c.w};
    dst[p] = er_id_matte_px(si, sc, list, count, n);
}

// ---- er_pick_rect: mark, block counts, exclusive scan, ordered write.  The marks cover the kind's ids 0 .. domain - 1 and, at index
// `domain`, ER_ID_NONE: ascending order of the indices is ascending order of the ids as unsigned.  Plain stores only: every writer of a
// mark stores the same 1. ----
__global__ __launch_bounds__(256) void k_id_mark(const uint4* __restrict__ ids, const uint4* __restrict__ counts, uint32_t x_res, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                                 uint32_t domain, uint32_t* __restrict__ mark) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)w * h) return;
    const size_t p = (size_t)(y0 + (uint32_t)(i / w)) * x_res + (x0 + (uint32_t)(i % w));
    const uint4 a = ids[p], c = counts[p];
    const uint32_t si[ER_ID_SLOTS] = {a.x, a.y, a.z, a.w}, sc[ER_ID_SLOTS] = {c.x, c.y, c.z, c.w};
    for (int s = 0; s < ER_ID_SLOTS; s++) {
        if (!sc[s]) continue;
        const uint32_t at = si[s] == ER_ID_NONE ? domain : si[s];
        if (at <= domain) mark[at] = 1u;      // (an id beyond the domain cannot come out of the pass; it would be out of bounds here)
    }
}
// the marks of block b's 256 indices: each thread's rank among them and the block's count
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t& block_total) {
    __shared__ uint32_t s_wave[4];
    const unsigned long long mask = __ballot(flag);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t v = 0; v < 4; v++) { if (v < wave) before += s_wave[v]; total += s_wave[v]; }
    block_total = total;
    return before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}
__global__ __launch_bounds__(256) void k_id_block_count(const uint32_t* __restrict__ mark, uint32_t total, uint32_t* __restrict__ block_count) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t sum;
    block_rank(i < total && mark[i] != 0u, sum);
    if (threadIdx.x == 0) block_count[blockIdx.x] = sum;
}
// one workgroup: block_offset[b] = the marks before block b, block_offset[nb] = all of them
__global__ __launch_bounds__(256) void k_id_scan(const uint32_t* __restrict__ block_count, uint32_t nb, uint32_t* __restrict__ block_offset) {
    __shared__ uint32_t s_sum[256];
    const uint32_t chunk = (nb + 255u) / 256u, lo = threadIdx.x * chunk, hi = lo + chunk < nb ? lo + chunk : nb;
    uint32_t sum = 0;
    for (uint32_t b = lo; b < hi; b++) sum += block_count[b];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t t = 0; t < 256; t++) { const uint32_t v = s_sum[t]; s_sum[t] = run; run += v; }
        block_offset[nb] = run;
    }
    __syncthreads();
    uint32_t run = s_sum[threadIdx.x];
    for (uint32_t b = lo; b < hi; b++) { block_offset[b] = run; run += block_count[b]; }
}
__global__ __launch_bounds__(256) void k_id_write(const uint32_t* __restrict__ mark, uint32_t total, uint32_t domain, const uint32_t* __restrict__ block_offset,
                                                  uint32_t* __restrict__ out, uint32_t capacity) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool flag = i < total && mark[i] != 0u;
    uint32_t sum;
    const uint32_t at = block_offset[blockIdx.x] + block_rank(flag, sum);
    if (flag && at < capacity) out[at] = i == domain ? ER_ID_NONE : i;
}

hipError_t er_probe_ids(const char** which) {
    hipFuncAttributes a;
    hipError_t e;
    *which = "er_ids_kernel";
    if ((e = hipFuncGetAttributes(&a, (const void*)er_ids_kernel<false>)) != hipSuccess) return e;
    *which = "er_ids_kernel (cut-outs)";
    if ((e = hipFuncGetAttributes(&a, (const void*)er_ids_kernel<true, float, unsigned long long*>)) != hipSuccess) return e;
    *which = "er_pick_kernel";
    if ((e = hipFuncGetAttributes(&a, (const void*)er_pick_kernel<false>)) != hipSuccess) return e;
    *which = "er_pick_kernel (cut-outs)";
    if ((e = hipFuncGetAttributes(&a, (const void*)er_pick_kernel<true, float>)) != hipSuccess) return e;
    *which = "k_id_write (er_ids.hip)";
    return hipFuncGetAttributes(&a, (const void*)k_id_write);
}

// ---- the entry points (host side) ----
namespace {

const char* const k_kind_name[ER_ID_KIND_COUNT] = {"TRIANGLE", "OBJECT", "MATERIAL"};

uint4* id_plane(ErScene* s, int kind, int counts) { return (uint4*)s->d_id_planes.p + (size_t)(2 * kind + counts) * s->x_res * s->y_res; }

bool kind_ok(int kind) { return kind >= 0 && kind < ER_ID_KIND_COUNT; }

int need_planes(ErScene* s, const char* who) {
    if (!s->begun) return fail(ER_ERR_STATE, std::string(who) + ": er_render_begin has not succeeded");
    if (!s->ids.valid) return fail(ER_ERR_STATE, std::string(who) + ": no id planes of this scene state (er_render_ids)");
    return ER_OK;
}

// the tri -> object map of the current table; the stream is idle
int id_prepare(ErScene* s) {
    int rc;
    const uint32_t objects = s->objects.objects();
    if (s->id_map_valid || objects == 0) return ER_OK;      // (no table: the kernels take a NULL map and answer ER_ID_NONE)
    const uint32_t total = (uint32_t)s->objects.ids.size();
    if (s->d_id_map.n < s->tri_count && (rc = upload(s->d_id_map, nullptr, s->tri_count, s->stream)) != ER_OK) return rc;
    ScopedDevBuf<uint32_t> d_first, d_ids;
    if ((rc = upload(d_first, s->objects.first.data(), (size_t)objects + 1, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_ids, s->objects.ids.data(), total, s->stream)) != ER_OK) return rc;
    HIP_TRY(hipMemsetAsync(s->d_id_map.p, 0xFF, (size_t)s->tri_count * 4, s->stream));
    if (total) hipLaunchKernelGGL(k_id_map_scatter, dim3((total + 255) / 256), dim3(256), 0, s->stream, total, objects, (const uint32_t*)d_first.p, (const uint32_t*)d_ids.p, s->tri_count, s->d_id_map.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));      // the two uploads go out of scope
    s->id_map_valid = true;
    return ER_OK;
}
const uint32_t* id_map(ErScene* s) { return s->objects.objects() ? s->d_id_map.p : nullptr; }

int render_ids_impl(ErScene* s, uint32_t n) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_render_ids: NULL scene");
    if (n > ER_ID_MAX_RAYS) return fail(ER_ERR_INVALID_ARG, "er_render_ids: at most 64 samples");
    if (n == 0) n = 4;
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_render_ids: er_render_begin has not succeeded");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));      // pending asynchronous work first
    int rc;
    const size_t npx = (size_t)s->x_res * s->y_res, nplanes = 2 * ER_ID_KIND_COUNT;
    uint32_t blocks;
    s->ids.valid = false;
    if ((rc = er_first_hit_blocks(s, &blocks)) != ER_OK || (rc = id_prepare(s)) != ER_OK) return rc;
    if (s->d_id_planes.n < nplanes * npx && (rc = upload(s->d_id_planes, nullptr, nplanes * npx, s->stream)) != ER_OK) return rc;
    if (s->d_id_over.n < ER_ID_KIND_COUNT && (rc = upload(s->d_id_over, nullptr, ER_ID_KIND_COUNT, s->stream)) != ER_OK) return rc;
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    // every slot empty -- id planes all ones (ER_ID_NONE), count planes zero: what pixels of other ranks read as until they are gathered
    for (int k = 0; k < ER_ID_KIND_COUNT; k++) {
        HIP_TRY(hipMemsetAsync(id_plane(s, k, 0), 0xFF, npx * sizeof(uint4), s->stream));
        HIP_TRY(hipMemsetAsync(id_plane(s, k, 1), 0, npx * sizeof(uint4), s->stream));
    }
    HIP_TRY(hipMemsetAsync(s->d_id_over.p, 0, ER_ID_KIND_COUNT * 4, s->stream));
    const bool cutouts = er_first_hit_cutouts(s);
    if (cutouts && (rc = er_first_hit_counts_begin(s)) != ER_OK) return rc;
    HIP_TRY(hipEventRecord(ev.a, s->stream));
    if (s->dev.owned_tile_count) {
        if (cutouts)
            hipLaunchKernelGGL((er_ids_kernel<true, float, unsigned long long*>), dim3(blocks), dim3(64), 0, s->stream, s->dev, n, id_map(s), (uint4*)s->d_id_planes.p, npx,
                               s->d_id_over.p, s->d_first_hit_spill.p, s->first_hit.threshold, s->d_first_hit_counts.p);
        else
            hipLaunchKernelGGL(er_ids_kernel<false>, dim3(blocks), dim3(64), 0, s->stream, s->dev, n, id_map(s), (uint4*)s->d_id_planes.p, npx, s->d_id_over.p, s->d_first_hit_spill.p);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.b, s->stream));
    HIP_TRY(hipMemcpyAsync(s->ids_overflow, s->d_id_over.p, ER_ID_KIND_COUNT * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (cutouts && (rc = er_first_hit_counts_end(s)) != ER_OK) return rc;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    s->ids = {true, n, s->owned_pixels() * n, ms};      // (one camera ray per sample and owned pixel inside the frame)
    s->ids_objects = s->objects.objects();
    return ER_OK;
}

int id_info_impl(ErScene* s, ErIdInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_id_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_id_info: er_render_begin has not succeeded");
    *out = ErIdInfo{};
    out->valid = s->ids.valid ? 1u : 0u;
    if (s->ids.valid) {
        out->samples = s->ids.samples; out->rays = s->ids.rays; out->ms = s->ids.ms; out->objects = s->ids_objects;
        for (int k = 0; k < ER_ID_KIND_COUNT; k++) out->overflow_pixels[k] = s->ids_overflow[k];
    }
    return ER_OK;
}

int read_ids_impl(ErScene* s, int kind, uint32_t* ids, uint32_t* counts) {
    if (!s || (!ids && !counts)) return fail(ER_ERR_INVALID_ARG, "er_read_ids: NULL argument");
    if (!kind_ok(kind)) return fail(ER_ERR_INVALID_ARG, "er_read_ids: kind out of range");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = need_planes(s, "er_read_ids")) != ER_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t bytes = (size_t)s->x_res * s->y_res * sizeof(uint4);
    if (ids) HIP_TRY(hipMemcpyAsync(ids, id_plane(s, kind, 0), bytes, hipMemcpyDeviceToHost, s->stream));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, id_plane(s, kind, 1), bytes, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return er_scene_stream_status(s, "er_read_ids");
}

int id_matte_impl(ErScene* s, int kind, const uint32_t* ids, uint32_t count, float* dst) {
    if (!s || !ids || !dst) return fail(ER_ERR_INVALID_ARG, "er_id_matte: NULL argument");
    if (count == 0) return fail(ER_ERR_INVALID_ARG, "er_id_matte: an empty list");
    if (!kind_ok(kind)) return fail(ER_ERR_INVALID_ARG, "er_id_matte: kind out of range");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    if ((rc = need_planes(s, "er_id_matte")) != ER_OK) return rc;
    host_reserve((uint64_t)count * 4);
    const std::vector<uint32_t> list = er_id_list_prepare(ids, count);
    HIP_TRY(hipSetDevice(s->device));
    const size_t npx = (size_t)s->x_res * s->y_res;
    // the scene's work words hold the plane, then the list (kept from call to call: a matte per frame allocates nothing)
    const size_t words = npx + list.size();
    if (s->d_id_work.n < words && (rc = upload(s->d_id_work, nullptr, words, s->stream)) != ER_OK) return rc;
    float* const d_dst = (float*)s->d_id_work.p;
    uint32_t* const d_list = s->d_id_work.p + npx;
    HIP_TRY(hipMemcpyAsync(d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice, s->stream));
    if (npx)
        hipLaunchKernelGGL(k_id_matte, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s->stream, (const uint4*)id_plane(s, kind, 0), (const uint4*)id_plane(s, kind, 1), npx,
                           (const uint32_t*)d_list, (uint32_t)list.size(), s->ids.samples, d_dst);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dst, d_dst, npx * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));      // (`list` goes out of scope)
    return er_scene_stream_status(s, "er_id_matte");
}

int pick_rect_impl(ErScene* s, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, int kind, uint32_t* ids, uint32_t capacity, uint32_t* count) {
    if (!s || !count || (capacity && !ids)) return fail(ER_ERR_INVALID_ARG, "er_pick_rect: NULL argument");
    if (!kind_ok(kind)) return fail(ER_ERR_INVALID_ARG, "er_pick_rect: kind out of range");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (x0 >= x1 || y0 >= y1 || x1 > s->x_res || y1 > s->y_res) return fail(ER_ERR_INVALID_ARG, "er_pick_rect: the rectangle is empty or leaves the frame");
    int rc;
    if ((rc = need_planes(s, "er_pick_rect")) != ER_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    // the ids the kind can show: 0 .. domain - 1 and ER_ID_NONE
    const uint64_t domain64 = kind == ER_ID_TRIANGLE ? s->tri_count : kind == ER_ID_OBJECT ? s->ids_objects : s->materials.size();
    if (domain64 >= 0xFFFFFF00ull) return fail(ER_ERR_INVALID_ARG, std::string("er_pick_rect: too many ids of kind ") + k_kind_name[kind]);
    const uint32_t domain = (uint32_t)domain64, total = domain + 1u, nb = (total + 255u) / 256u, cap = std::min(capacity, total);
    const size_t words = (size_t)total + nb + (nb + 1u) + cap;
    if (s->d_id_work.n < words && (rc = upload(s->d_id_work, nullptr, words, s->stream)) != ER_OK) return rc;
    uint32_t *mark = s->d_id_work.p, *bcount = mark + total, *boff = bcount + nb, *out = boff + nb + 1u;
    const uint32_t w = x1 - x0, h = y1 - y0;
    HIP_TRY(hipMemsetAsync(mark, 0, (size_t)total * 4, s->stream));
    hipLaunchKernelGGL(k_id_mark, dim3((unsigned)(((size_t)w * h + 255) / 256)), dim3(256), 0, s->stream, (const uint4*)id_plane(s, kind, 0), (const uint4*)id_plane(s, kind, 1), s->x_res,
                       x0, y0, w, h, domain, mark);
    hipLaunchKernelGGL(k_id_block_count, dim3(nb), dim3(256), 0, s->stream, (const uint32_t*)mark, total, bcount);
    hipLaunchKernelGGL(k_id_scan, dim3(1), dim3(256), 0, s->stream, (const uint32_t*)bcount, nb, boff);
    hipLaunchKernelGGL(k_id_write, dim3(nb), dim3(256), 0, s->stream, (const uint32_t*)mark, total, domain, (const uint32_t*)boff, out, cap);
    HIP_TRY(hipGetLastError());
    uint32_t found = 0;
    HIP_TRY(hipMemcpyAsync(&found, boff + nb, 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const uint32_t give = std::min(found, cap);
    if (give) HIP_TRY(hipMemcpy(ids, out, (size_t)give * 4, hipMemcpyDeviceToHost));
    *count = found;
    return er_scene_stream_status(s, "er_pick_rect");
}

int pick_impl(ErScene* s, uint32_t x, uint32_t y, ErPick* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_pick: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (x >= s->x_res || y >= s->y_res) return fail(ER_ERR_INVALID_ARG, "er_pick: the pixel is outside the frame");
    if (!s->begun) return fail(ER_ERR_STATE, "er_pick: er_render_begin has not succeeded");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));      // pending asynchronous work first
    int rc;
    if ((rc = er_first_hit_spill(s, 1)) != ER_OK || (rc = id_prepare(s)) != ER_OK) return rc;
    if (s->d_id_work.n < sizeof(ErPick) / 4 && (rc = upload(s->d_id_work, nullptr, sizeof(ErPick) / 4, s->stream)) != ER_OK) return rc;
    if (er_first_hit_cutouts(s))
        hipLaunchKernelGGL((er_pick_kernel<true, float>), dim3(1), dim3(64), 0, s->stream, s->dev, x, y, id_map(s), s->d_id_work.p, s->d_first_hit_spill.p, s->first_hit.threshold);
    else
        hipLaunchKernelGGL(er_pick_kernel<false>, dim3(1), dim3(64), 0, s->stream, s->dev, x, y, id_map(s), s->d_id_work.p, s->d_first_hit_spill.p);
    HIP_TRY(hipGetLastError());
    ErPick got{};
    HIP_TRY(hipMemcpyAsync(&got, s->d_id_work.p, sizeof(ErPick), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    *out = got;
    return er_scene_stream_status(s, "er_pick");
}

}  // namespace

// what er_history.hip shares with the pass: the tri -> object map
int er_id_prepare(ErScene* s) { return id_prepare(s); }
const uint32_t* er_id_map(ErScene* s) { return id_map(s); }

extern "C" {
int er_render_ids(ErScene* s, uint32_t n) { return guarded("er_render_ids", [&]() -> int { return render_ids_impl(s, n); }); }
int er_id_info(ErScene* s, ErIdInfo* out) { return guarded("er_id_info", [&]() -> int { return id_info_impl(s, out); }); }
int er_read_ids(ErScene* s, int kind, uint32_t* ids, uint32_t* counts) { return guarded("er_read_ids", [&]() -> int { return read_ids_impl(s, kind, ids, counts); }); }
int er_id_matte(ErScene* s, int kind, const uint32_t* ids, uint32_t count, float* dst) { return guarded("er_id_matte", [&]() -> int { return id_matte_impl(s, kind, ids, count, dst); }); }
int er_pick_rect(ErScene* s, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, int kind, uint32_t* ids, uint32_t capacity, uint32_t* count) {
    return guarded("er_pick_rect", [&]() -> int { return pick_rect_impl(s, x0, y0, x1, y1, kind, ids, capacity, count); });
}
int er_pick(ErScene* s, uint32_t x, uint32_t y, ErPick* out) { return guarded("er_pick", [&]() -> int { return pick_impl(s, x, y, out); }); }
}  // extern "C"
