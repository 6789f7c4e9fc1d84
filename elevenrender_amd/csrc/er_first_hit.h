// er_first_hit.h -- the stateless first-hit camera pass, stated once for its four consumers: er_features_kernel (er_features.hip),
// er_ids_kernel and er_pick_kernel (er_ids.hip), er_history_key_kernel (er_history.hip).  Camera rays of the owned pixels through the
// production wide traversal; nothing of the render is read or written.  Each consumer keeps a kernel and a per-pixel body of its own;
// what their bit-exact contracts with one another rest on is here: the LDS stacks, the spill slice, the camera's trig, the walk over
// the owned tiles, the sample ray and the closest-hit query.  ONE EXCEPTION: er_ids_kernel restates all but the trig (see there).
//
// The pass has two modes (include/eleven_hip.h er_first_hit_set).  Off, the default: the first hit counts whatever its
// opacity -- closest().  On: the ray goes on through hits whose opacity is below a threshold, as the render's path goes on through a
// hit that fails its opacity draw -- visible(), around the rule of er_cutout.h.  The consumers' kernels take the mode as a template
// parameter: the mode-off instances have the arguments and the code they had before the mode existed.
#pragma once
#include "er_cutout.h"
#include "er_scene.h"
#include "er_trav.h"

// Workgroups (one wave each) of the pass per CU: the grid is bounded -- the tiles are walked with a grid stride -- so that the
// traversal's spill area (ER_FIRST_HIT_SPILL_PER_BLOCK uint2 per workgroup, 16 KB) stays at 4 MB per 64 CUs whatever the frame.
#define ER_FIRST_HIT_BLOCKS_PER_CU 4u
#define ER_FIRST_HIT_SPILL_PER_BLOCK ((size_t)ER_STACK8 * 64)
// The counters of the mode that sees through cut-outs (ErFirstHitInfo): 64-bit words, 64 bytes apart.
enum { ER_FH_RAYS = 0, ER_FH_THROUGH = 1, ER_FH_LAYERS = 2, ER_FH_CAPPED = 3, ER_FH_TO_MISS = 4, ER_FH_COUNTERS = 5 };
#define ER_FH_COUNT_STRIDE 8u

namespace erd {

// the three ids of the record in `slot`, and the object of a triangle (tri_object: the map of er_id_map, or NULL without a table)
ERD uint32_t slot_triangle(const DevScene& S, uint32_t slot) { return __builtin_bit_cast(uint32_t, S.tri_isect[(size_t)slot * 3].w); }
ERD uint32_t slot_material(const DevScene& S, uint32_t slot) { return __builtin_bit_cast(uint32_t, S.tri_attr[(size_t)slot * ER_ATTR_PIECES + 6].x); }
ERD uint32_t triangle_object(const DevScene& S, const uint32_t* __restrict__ tri_object, uint32_t tri) {
    return (tri_object && tri < S.tri_count) ? tri_object[tri] : ER_ID_NONE;
}

// the opacity generate_hit_data (er_device.h) gives a hit: the material's constant, or the first channel of its opacity texture
ERD float hit_opacity(const DevScene& S, const HitFull& hit) {
    const ErMaterial& mat = S.materials[hit.material];
    return mat.opacity_tex < 0 ? mat.opacity : tex_filtered(S, S.textures[mat.opacity_tex], hit.tu, hit.tv).x;
}
// the render's ray past a hit it passes through (er_bounce.inc), by er_cutout.h
ERD Ray cutout_continue(const HitFull& hit, const Ray& ray) {
    const float p[3] = {hit.position.x, hit.position.y, hit.position.z}, d[3] = {ray.d.x, ray.d.y, ray.d.z};
    float o2[3], d2[3];
    er_cutout_continue(p, d, o2, d2);
    Ray r;
    r.o = f3(o2[0], o2[1], o2[2]);
    r.d = f3(d2[0], d2[1], d2[2]);
    return r;
}

// What a lane traces with: its columns of the workgroup's two LDS stacks, its column of the workgroup's spill slice and the camera's six
// sines and cosines.  stack2 -- ER_STACK words per lane, [k][lane] -- is the exact routine's and idle between two closest() calls.
struct FirstHit {
    const DevScene& S;
    uint2 *stack, *spill;
    int* stack2;      // (er_ids_kernel ranks a lane's ids in these words)
    CamTrig trig;
    // the next sample ray of pixel (px, py): five draws from rs, left to right (src/kernel.cpp:492-493), then camera_ray
    ERD Ray sample_ray(uint32_t px, uint32_t py, uint32_t& rs) const {
        const float c1 = rng_next(rs), c2 = rng_next(rs), c3 = rng_next(rs), c4 = rng_next(rs), c5 = rng_next(rs);
        return camera_ray(S.cam, (int)px, (int)py, S.x_res, S.y_res, c1, c2, c3, c4, c5, &trig);
    }
    // the record slot of the ray's closest hit (wide traversal, exact fallback: the production result), or -1
    ERD int closest(const Ray& ray) const {
        int info;
        unsigned cn = 0, ct = 0;
        return trav_run_closest<false>(S, stack, spill, stack2, ray, __builtin_inff(), info, cn, ct);
    }
    // Mode on: the record slot of the first hit along `ray` whose opacity is >= threshold, with its HitFull in `hit` (of the segment
    // that found it: position, uv and material are the ones the render would shade), or -1.  At most S.max_bounces hits are examined,
    // as a path of the render ends there: `capped` says that all of them passed.  layers: the hits passed.  trav_run_closest is
    // lane-local (no ballot, no barrier), so the lanes of a wave leave the loop one by one.
    ERD int visible(Ray ray, float threshold, HitFull& hit, uint32_t& layers, bool& capped) const {
        layers = 0;
        capped = false;
        for (uint32_t k = 0; k < S.max_bounces; k++) {
            const int slot = closest(ray);
            if (slot < 0) return -1;
            full_hit(S, (uint32_t)slot, ray, hit);
            if (er_cutout_stops(hit_opacity(S, hit), threshold)) return slot;
            layers++;
            ray = cutout_continue(hit, ray);
        }
        capped = true;
        return -1;
    }
};

// What a consumer's kernel holds of the mode.  Off: nothing -- no argument, no register.  On: the threshold, the counter words and the
// lane's own sums over its whole walk, which flush() adds up over the wave (every lane of it must call; five sums by six exchanges) and
// gives to the counters with one atomicAdd per wave and counter: k_variance_fold's pattern, no atomic inside the walk.
template <bool CUTOUTS>
struct Cutouts {
    ERD void flush() const {}
};
template <>
struct Cutouts<true> {
    float threshold;
    unsigned long long* counts;      // (NULL: er_pick_kernel counts nothing)
    uint32_t n[ER_FH_COUNTERS] = {0u, 0u, 0u, 0u, 0u};
    ERD Cutouts(float t, unsigned long long* c) : threshold(t), counts(c) {}
    ERD explicit Cutouts(float t) : threshold(t), counts(nullptr) {}
    ERD int visible(const FirstHit& fh, const Ray& ray, HitFull& hit) {
        uint32_t layers;
        bool capped;
        const int slot = fh.visible(ray, threshold, hit, layers, capped);
        tally(slot, layers, capped);
        return slot;
    }
    ERD void tally(int slot, uint32_t layers, bool capped) {
        n[ER_FH_RAYS]++;
        n[ER_FH_THROUGH] += layers ? 1u : 0u;
        n[ER_FH_LAYERS] += layers;
        n[ER_FH_CAPPED] += capped ? 1u : 0u;
        n[ER_FH_TO_MISS] += (slot < 0 && layers && !capped) ? 1u : 0u;
    }
    ERD void flush() const {
#pragma unroll
        for (int c = 0; c < ER_FH_COUNTERS; c++) {
            unsigned long long v = n[c];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
            if (threadIdx.x == 0 && v) atomicAdd(counts + (size_t)c * ER_FH_COUNT_STRIDE, v);
        }
    }
};

// the calling lane's handle; spill_base: gridDim.x * ER_FIRST_HIT_SPILL_PER_BLOCK uint2 (er_first_hit_blocks)
ERD FirstHit first_hit_lane(const DevScene& S, uint2* spill_base) {
    __shared__ uint2 s_stack[WF_LDS_STACK * 64];
    __shared__ int s_stack2[ER_STACK * 64];
    const uint32_t lane = threadIdx.x;
    FirstHit fh{S, s_stack + lane, spill_base + (size_t)blockIdx.x * ER_FIRST_HIT_SPILL_PER_BLOCK + lane, s_stack2 + lane, {}};
    scene_cam_trig(S, fh.trig);
    return fh;
}

// One wave per 8x8 tile, one lane per pixel; a fixed number of workgroups walks the owned tiles with a grid stride (no workgroup waits
// for or talks to another).  pixel(px, py, handle) runs for every owned pixel inside the frame; with idx = py * x_res + px its seed is
// jenkins_u32(idx + 1), the value er_setup_kernel gives DevScene::rng -- which is not touched.
template <class F>
ERD void first_hit_walk(const DevScene& S, uint2* spill_base, F&& pixel) {
    const FirstHit fh = first_hit_lane(S, spill_base);
    const uint32_t lane = threadIdx.x;
    for (uint32_t t = blockIdx.x; t < S.owned_tile_count; t += gridDim.x) {
        const uint32_t tile = S.owned_tiles[t];
        const uint32_t px = (tile % S.tiles_x) * ER_TILE + (lane & 7u), py = (tile / S.tiles_x) * ER_TILE + (lane >> 3);
        if (px >= S.x_res || py >= S.y_res) continue;
        pixel(px, py, fh);
    }
}

}  // namespace erd

namespace erh {

// the spill area grown to hold `blocks` slices (er_pick: 1).  The scene's mutex is held and its stream idle.
inline int er_first_hit_spill(ErScene* s, uint32_t blocks) {
    const size_t need = blocks * ER_FIRST_HIT_SPILL_PER_BLOCK;
    return s->d_first_hit_spill.n < need ? upload(s->d_first_hit_spill, nullptr, need, s->stream) : ER_OK;
}
// the whole-frame pass's workgroup count on the scene's device, with the spill area grown to as many slices
inline int er_first_hit_blocks(ErScene* s, uint32_t* blocks) {
    *blocks = std::max(1u, s->kept.cus) * ER_FIRST_HIT_BLOCKS_PER_CU;
    return er_first_hit_spill(s, *blocks);
}

// the threshold the mode-on kernels take, and the mode's counters around a whole-frame pass: zeroed on the stream before the launch,
// read back after it (the stream is idle on return).  Mode off: nothing is allocated, launched or copied.
inline bool er_first_hit_cutouts(const ErScene* s) { return s->first_hit.cutouts != 0; }
inline int er_first_hit_counts_begin(ErScene* s) {
    int rc;
    const size_t words = (size_t)ER_FH_COUNTERS * ER_FH_COUNT_STRIDE;
    if (s->d_first_hit_counts.n < words && (rc = upload(s->d_first_hit_counts, nullptr, words, s->stream)) != ER_OK) return rc;
    HIP_TRY(hipMemsetAsync(s->d_first_hit_counts.p, 0, words * sizeof(unsigned long long), s->stream));
    return ER_OK;
}
inline int er_first_hit_counts_end(ErScene* s) {
    unsigned long long got[ER_FH_COUNTERS * ER_FH_COUNT_STRIDE];
    HIP_TRY(hipMemcpyAsync(got, s->d_first_hit_counts.p, sizeof(got), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (int c = 0; c < ER_FH_COUNTERS; c++) s->first_hit.counts[c] = got[(size_t)c * ER_FH_COUNT_STRIDE];
    return ER_OK;
}

}  // namespace erh
