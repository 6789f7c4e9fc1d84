// er_first_hit.h -- the stateless first-hit camera pass, stated once for its four consumers: er_features_kernel (er_features.hip),
// er_ids_kernel and er_pick_kernel (er_ids.hip), er_history_key_kernel (er_history.hip).  Camera rays of the owned pixels through the
// production wide traversal; nothing of the render is read or written.  Each consumer keeps a kernel and a per-pixel body of its own;
// what their bit-exact contracts with one another rest on is here: the LDS stacks, the spill slice, the camera's trig, the walk over
// the owned tiles, the sample ray and the closest-hit query.  ONE EXCEPTION: er_ids_kernel restates all but the trig (see there).
#pragma once
#include "er_scene.h"
#include "er_trav.h"

// Workgroups (one wave each) of the pass per CU: the grid is bounded -- the tiles are walked with a grid stride -- so that the
// traversal's spill area (ER_FIRST_HIT_SPILL_PER_BLOCK uint2 per workgroup, 16 KB) stays at 4 MB per 64 CUs whatever the frame.
#define ER_FIRST_HIT_BLOCKS_PER_CU 4u
#define ER_FIRST_HIT_SPILL_PER_BLOCK ((size_t)ER_STACK8 * 64)

namespace erd {

// the three ids of the record in `slot`, and the object of a triangle (tri_object: the map of er_id_map, or NULL without a table)
ERD uint32_t slot_triangle(const DevScene& S, uint32_t slot) { return __builtin_bit_cast(uint32_t, S.tri_isect[(size_t)slot * 3].w); }
ERD uint32_t slot_material(const DevScene& S, uint32_t slot) { return __builtin_bit_cast(uint32_t, S.tri_attr[(size_t)slot * ER_ATTR_PIECES + 6].x); }
ERD uint32_t triangle_object(const DevScene& S, const uint32_t* __restrict__ tri_object, uint32_t tri) {
    return (tri_object && tri < S.tri_count) ? tri_object[tri] : ER_ID_NONE;
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

}  // namespace erh
