// er_debug_api.cpp -- the inspection hooks of include/eleven_hip_debug.h (host side).  Not part of the drop-in boundary:
// they exist so that the test-suite can compare single functions of the production path with the oracle -- the traversal
// (level 1) and the per-bounce trace of one pixel-sample (level 2; reference src/kernel.cpp:508-592) --
// and exercise the boundary's failure paths.
#include "er_scene.h"
#include "er_debug.h"
#include "er_hdri_trig.h"

using namespace erh;

// ---- host-only debug hook (include/eleven_hip_debug.h) ----
#include "../../include/eleven_hip_debug.h"

static int er_debug_closest_hit_impl(ErScene* s, const float* origins, const float* dirs, uint32_t n, int32_t* tri_ids, float* positions, float* distances) {
    if (!s || !origins || !dirs || !tri_ids || !positions || !distances) return fail(ER_ERR_INVALID_ARG, "er_debug_closest_hit: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_debug_closest_hit: er_render_begin has not succeeded");
    HIP_TRY(hipSetDevice(s->device));
    ScopedDevBuf<float> d_o, d_d, d_pos, d_dist;
    ScopedDevBuf<int32_t> d_tri;
    int rc;
    if ((rc = upload(d_o, origins, (size_t)n * 3, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_d, dirs, (size_t)n * 3, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_pos, (const float*)nullptr, (size_t)n * 3, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_dist, (const float*)nullptr, (size_t)n, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_tri, (const int32_t*)nullptr, (size_t)n, s->stream)) != ER_OK) return rc;
    er_launch_debug_hit(s->dev, d_o.p, d_d.p, n, d_tri.p, d_pos.p, d_dist.p, s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(tri_ids, d_tri.p, (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(positions, d_pos.p, (size_t)n * 12, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(distances, d_dist.p, (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ER_OK;
}

static int er_debug_cdf_search_impl(const float* cdf, int length, const float* values, int32_t* out, int count) {
    if (!cdf || !values || !out || length <= 0) return fail(ER_ERR_INVALID_ARG, "er_debug_cdf_search: bad argument");
    std::vector<uint32_t> guide;
    int buckets = er_build_cdf_guide(cdf, length, guide);
    for (int i = 0; i < count; i++) out[i] = er_cdf_search(cdf, length, guide.data(), buckets, values[i]);
    return ER_OK;
}

static int er_debug_stream_deal_impl(const uint32_t* owned, uint32_t count, uint32_t tiles_x, uint32_t blocks, int xcd_aware, uint32_t edge, uint32_t* out, uint32_t out_cap,
                                     uint32_t* most) {
    if ((count && !owned) || !tiles_x || !blocks || !most) return fail(ER_ERR_INVALID_ARG, "er_debug_stream_deal: bad argument");
    std::vector<uint32_t> deal;
    *most = er_stream_deal_tiles(owned, count, tiles_x, blocks, xcd_aware != 0, deal, edge);
    if (deal.size() > out_cap || (deal.size() && !out)) return fail(ER_ERR_INVALID_ARG, "er_debug_stream_deal: out holds fewer than blocks * most entries");
    for (size_t i = 0; i < deal.size(); i++) out[i] = deal[i];
    return ER_OK;
}

static int er_debug_stream_level_impl(const uint32_t* deal, uint32_t deal_n, uint32_t tiles_x, uint32_t blocks, const uint32_t* cost, uint32_t cost_n, uint32_t cap, uint32_t* out,
                                      uint32_t out_cap, uint32_t* most) {
    if ((deal_n && !deal) || (cost_n && !cost) || !tiles_x || !blocks || deal_n % blocks != 0u || !cap || !most) return fail(ER_ERR_INVALID_ARG, "er_debug_stream_level: bad argument");
    std::vector<uint32_t> lvl;
    *most = er_stream_level_by_cost(std::vector<uint32_t>(deal, deal + deal_n), tiles_x, blocks, cost, cost_n, cap, lvl);
    if (lvl.size() > out_cap || (lvl.size() && !out)) return fail(ER_ERR_INVALID_ARG, "er_debug_stream_level: out holds fewer than blocks * most entries");
    for (size_t i = 0; i < lvl.size(); i++) out[i] = lvl[i];
    return ER_OK;
}

static int er_debug_stream_balance_impl(ErScene* s, ErStreamBalance* info, uint64_t* wg_ticks, uint32_t* wg_tiles, uint64_t* wg_cost, uint32_t wg_cap, uint32_t* deal, uint32_t deal_cap,
                                        uint32_t* tile_cost, uint32_t cost_cap) {
    if (!s || !info) return fail(ER_ERR_INVALID_ARG, "er_debug_stream_balance: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    memset(info, 0, sizeof(*info));
    if (!s->begun || !(s->params.flags & ER_FLAG_STREAM)) return ER_OK;
    const StreamHost& st = s->st;
    info->blocks = st.blocks;
    info->most = st.blocks ? (uint32_t)(st.deal_host.size() / st.blocks) : 0u;
    info->levelled = st.deal_levelled ? 1u : 0u;
    info->counting = st.counting ? 1u : 0u;
    info->cost_tiles = (uint32_t)st.cost_host.size();
    info->cap = st.ring_cap / 64u;
    info->launch_ticks = st.launch_end > st.launch_start ? st.launch_end - st.launch_start : 0u;
    if (wg_cap >= st.blocks) {
        std::vector<uint32_t> tiles; std::vector<uint64_t> cost, ticks;
        stream_balance(s, tiles, cost, ticks);
        for (uint32_t b = 0; b < st.blocks; b++) {
            if (wg_ticks) wg_ticks[b] = ticks[b];
            if (wg_tiles) wg_tiles[b] = tiles[b];
            if (wg_cost) wg_cost[b] = cost[b];
        }
    }
    if (deal && deal_cap >= st.deal_host.size()) for (size_t i = 0; i < st.deal_host.size(); i++) deal[i] = st.deal_host[i];
    if (tile_cost && cost_cap >= st.cost_host.size()) for (size_t i = 0; i < st.cost_host.size(); i++) tile_cost[i] = st.cost_host[i];
    return ER_OK;
}

static int er_debug_stream_form_impl(uint32_t tiles, uint32_t blocks, int light_query, uint32_t tri_count, uint32_t flags, ErStreamForm* out) {
    if (!out || !blocks) return fail(ER_ERR_INVALID_ARG, "er_debug_stream_form: bad argument");
    const StreamForm f = stream_choose_form(tiles, blocks, light_query != 0, tri_count, flags);
    *out = ErStreamForm{f.waves, f.tracers, f.adapt ? 1u : 0u, f.keep ? 1u : 0u, f.spec ? 1u : 0u, 0u};
    return ER_OK;
}

static int er_debug_bvh_check_impl(const float* vertices, const float* normals, uint32_t tri_count, int threads, ErBvhCheck* out) {
    if (!out || (tri_count && (!vertices || !normals))) return fail(ER_ERR_INVALID_ARG, "er_debug_bvh_check: NULL argument");
    ErBvhBuild b;
    er_build_bvh(vertices, normals, tri_count, threads, &b);
    memset(out, 0, sizeof(*out));
    out->node_count = (uint32_t)b.nodes.size();
    out->leaf_count = b.leaf_count;
    out->max_depth = b.max_depth;
    out->lift_bound = b.lift_bound;
    out->build_ms = (float)b.build_ms;
    std::vector<uint8_t> seen(tri_count, 0), visited(b.nodes.size(), 0);
    struct Item { int32_t ref; float lo[3], hi[3]; bool has_box; };
    std::vector<Item> stack;
    if (!b.nodes.empty()) stack.push_back(Item{0, {0, 0, 0}, {0, 0, 0}, false});
    auto area = [](const float* lo, const float* hi) {
        float x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
        return 2.0 * ((double)x * y + (double)x * z + (double)y * z);
    };
    double root_area = 0;
    if (!b.nodes.empty()) {
        const ErNode& r = b.nodes[0];
        float lo[3], hi[3];
        for (int a = 0; a < 3; a++) {
            lo[a] = r.c1 == ER_BVH_NO_CHILD ? r.lo0[a] : std::min(r.lo0[a], r.lo1[a]);
            hi[a] = r.c1 == ER_BVH_NO_CHILD ? r.hi0[a] : std::max(r.hi0[a], r.hi1[a]);
        }
        root_area = area(lo, hi);
    }
    while (!stack.empty()) {
        Item it = stack.back();
        stack.pop_back();
        if (it.ref == ER_BVH_NO_CHILD) continue;
        if (it.ref >= 0) {
            if ((size_t)it.ref >= b.nodes.size()) { out->uncontained++; continue; }
            if (visited[it.ref]++) { out->duplicate_tris++; continue; }
            const ErNode& n = b.nodes[it.ref];
            const float* los[2] = {n.lo0, n.lo1};
            const float* his[2] = {n.hi0, n.hi1};
            const int32_t cs[2] = {n.c0, n.c1};
            for (int k = 0; k < 2; k++) {
                if (cs[k] == ER_BVH_NO_CHILD) continue;
                if (it.has_box)
                    for (int a = 0; a < 3; a++)
                        if (los[k][a] < it.lo[a] || his[k][a] > it.hi[a]) out->uncontained++;
                Item c;
                c.ref = cs[k];
                c.has_box = true;
                memcpy(c.lo, los[k], 12);
                memcpy(c.hi, his[k], 12);
                uint32_t cnt = 0;
                if (cs[k] < 0) cnt = ((uint32_t)~cs[k] & 7u) + 1;
                if (root_area > 0) out->sah_cost += area(los[k], his[k]) / root_area * (cs[k] < 0 ? cnt : 1.0);
                stack.push_back(c);
            }
        } else {
            uint32_t v = (uint32_t)~it.ref, first = v >> 3, cnt = (v & 7u) + 1;
            out->max_leaf_size = std::max(out->max_leaf_size, cnt);
            for (uint32_t i = 0; i < cnt; i++) {
                uint32_t slot = first + i;
                if (slot >= tri_count) { out->uncontained++; continue; }
                uint32_t id = b.slot_to_tri[slot];
                if (seen[id]++) out->duplicate_tris++;
                out->tris_in_leaves++;
                for (int k = 0; k < 3; k++)
                    for (int a = 0; a < 3; a++) {
                        float p = vertices[(size_t)id * 9 + k * 3 + a];
                        if (p < it.lo[a] || p > it.hi[a]) out->uncontained++;
                    }
            }
        }
    }
    for (uint8_t v : visited) if (!v) out->unreachable_nodes++;
    return ER_OK;
}

// ---- the structure itself, copied out for tests/accel_check.py: no judgement here ----
static int dump_put(const char* who, void* dst, uint64_t cap, const void* src, uint64_t bytes, bool from_device, hipStream_t st) {
    if (!dst) return ER_OK;
    if (cap < bytes) return fail(ER_ERR_INVALID_ARG, std::string(who) + ": a buffer is smaller than its array (all buffers NULL queries the sizes)");
    if (!bytes) return ER_OK;
    if (from_device) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    else memcpy(dst, src, bytes);
    return ER_OK;
}

static int er_debug_read_accel_impl(ErScene* s, ErAccelDump* info, void* nodes, uint64_t nodes_cap, void* nodes8, uint64_t nodes8_cap, void* isect, uint64_t isect_cap,
                                    void* attr, uint64_t attr_cap) {
    if (!s || !info) return fail(ER_ERR_INVALID_ARG, "er_debug_read_accel: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_debug_read_accel: er_render_begin has not succeeded");
    const DevScene& D = s->dev;
    memset(info, 0, sizeof(*info));
    info->tri_count = s->tri_count;
    info->node_count = D.node_count;
    info->node8_count = D.node8_count;
    info->node8_pieces = ER_NODE8_PIECES;
    info->attr_pieces = ER_ATTR_PIECES;
    info->max_depth = s->accel_depth2;
    info->max_depth8 = s->accel.max_depth;
    info->builder = s->accel.builder;
    for (int a = 0; a < 3; a++) { info->lo[a] = s->accel_lo[a]; info->hi[a] = s->accel_hi[a]; }
    info->lift_bound = s->accel.lift_bound;
    info->max_lift = D.max_lift;
    if (!nodes && !nodes8 && !isect && !attr) return ER_OK;
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    const char* who = "er_debug_read_accel";
    if ((rc = dump_put(who, nodes, nodes_cap, D.nodes, (uint64_t)D.node_count * sizeof(ErNode), true, s->stream)) != ER_OK) return rc;
    if ((rc = dump_put(who, nodes8, nodes8_cap, D.nodes8, (uint64_t)D.node8_count * ER_NODE8_PIECES * 16, true, s->stream)) != ER_OK) return rc;
    if ((rc = dump_put(who, isect, isect_cap, D.tri_isect, ((uint64_t)s->tri_count + 1) * sizeof(ErTriIsect), true, s->stream)) != ER_OK) return rc;
    if ((rc = dump_put(who, attr, attr_cap, D.tri_attr, (uint64_t)s->tri_count * sizeof(ErTriAttr), true, s->stream)) != ER_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ER_OK;
}

// ---- the terms of the structure's measured cost (er_cost.h) ----
static_assert(sizeof(ErCostSumsDebug) == 40, "four doubles, a float and a reserved word");
static void cost_sums_out(const ErCostSums& c, ErCostSumsDebug* out) { *out = ErCostSumsDebug{c.node_area, c.leaf_area, c.tri_area, c.cost, c.ms, 0u}; }

static int er_debug_accel_cost_terms_impl(ErScene* s, ErCostSumsDebug* sums, double* node_terms, uint64_t node_cap, float* tri_terms, uint64_t tri_cap) {
    if (!s || !sums) return fail(ER_ERR_INVALID_ARG, "er_debug_accel_cost_terms: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_debug_accel_cost_terms: er_render_begin has not succeeded");
    const ErGpuBvhDevice& g = s->kept.accel;
    if ((node_terms && node_cap < (uint64_t)g.nodes8_count * 16) || (tri_terms && tri_cap < (uint64_t)s->tri_count * 4))
        return fail(ER_ERR_INVALID_ARG, "er_debug_accel_cost_terms: a buffer is smaller than its array");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    ErCostSums c;
    std::string why;
    const int crc = er_cost_device(s->d_nodes8.p, g.nodes8_count, (const ErTriIsect*)(s->d_nodes8.p + g.n8_pieces), s->tri_count, s->stream, &c, node_terms, tri_terms, why);
    if (crc != 0) return fail(crc == -2 ? ER_ERR_OOM : ER_ERR_HIP, "er_debug_accel_cost_terms: " + why);
    cost_sums_out(c, sums);
    return ER_OK;
}

static int er_debug_accel_cost_host_impl(const void* nodes8, uint32_t node8_count, uint32_t node8_pieces, const void* isect, uint32_t tri_count, ErCostSumsDebug* sums,
                                         double* node_terms, uint64_t node_cap, float* tri_terms, uint64_t tri_cap) {
    if (!sums || (node8_count && !nodes8) || (tri_count && !isect)) return fail(ER_ERR_INVALID_ARG, "er_debug_accel_cost_host: NULL argument");
    if (node8_pieces * 16u < sizeof(ErNode8)) return fail(ER_ERR_INVALID_ARG, "er_debug_accel_cost_host: node8_pieces is below a wide node's 5 pieces");
    if ((node_terms && node_cap < (uint64_t)node8_count * 16) || (tri_terms && tri_cap < (uint64_t)tri_count * 4))
        return fail(ER_ERR_INVALID_ARG, "er_debug_accel_cost_host: a buffer is smaller than its array");
    ErCostSums c;
    er_cost_host(nodes8, node8_count, node8_pieces, (const ErTriIsect*)isect, tri_count, &c, node_terms, tri_terms);
    cost_sums_out(c, sums);
    return ER_OK;
}

// ---- the texture pool: the plan, and what lies on the device (copies only) ----
static_assert(sizeof(ErTexEntry) == sizeof(DevTex) && sizeof(ErFusedEntry) == sizeof(DevFused), "the debug header's entries are the device records");

static int er_debug_texture_plan_impl(const ErSceneDesc* d, ErTexturePlan* out, uint8_t* modes, uint64_t modes_cap, ErTexEntry* table, uint64_t table_cap, ErFusedEntry* fused,
                                      uint64_t fused_cap) {
    if (!d || !out) return fail(ER_ERR_INVALID_ARG, "er_debug_texture_plan: NULL argument");
    if ((d->texture_count && !d->textures) || (d->material_count && !d->materials)) return fail(ER_ERR_INVALID_ARG, "er_debug_texture_plan: a list is missing");
    std::vector<TexDecl> decl(d->texture_count);
    for (uint32_t i = 0; i < d->texture_count; i++) decl[i] = TexDecl{d->textures[i].width, d->textures[i].height, d->textures[i].channels, d->textures[i].filter};
    const TexDecl h{d->hdri.texture.width, d->hdri.texture.height, d->hdri.texture.channels, d->hdri.texture.filter};
    TexPlan P;
    er_texture_plan(decl.data(), decl.size(), d->materials, d->material_count, h, P);
    memset(out, 0, sizeof(*out));
    out->texture_count = d->texture_count;
    out->fused_count = (uint32_t)P.fused.size();
    out->fused_any = P.fused_any ? 1u : 0u;
    memcpy(&out->hdri, &P.hdri, sizeof(DevTex));
    out->pool_floats = P.pool_floats;
    int rc;
    const char* who = "er_debug_texture_plan";
    if ((rc = dump_put(who, modes, modes_cap, P.mode.data(), P.mode.size(), false, nullptr)) != ER_OK) return rc;
    if ((rc = dump_put(who, table, table_cap, P.table.data(), P.table.size() * sizeof(DevTex), false, nullptr)) != ER_OK) return rc;
    return dump_put(who, fused, fused_cap, P.fused.data(), P.fused.size() * sizeof(DevFused), false, nullptr);
}

static int er_debug_read_textures_impl(ErScene* s, ErTextureDump* info, void* table, uint64_t table_cap, void* pool, uint64_t pool_cap, void* fused, uint64_t fused_cap,
                                       void* mat_pre, uint64_t mat_pre_cap, void* materials, uint64_t materials_cap, void* cdf, uint64_t cdf_cap, void* guide, uint64_t guide_cap) {
    if (!s || !info) return fail(ER_ERR_INVALID_ARG, "er_debug_read_textures: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_debug_read_textures: er_render_begin has not succeeded");
    const DevScene& D = s->dev;
    memset(info, 0, sizeof(*info));
    info->texture_count = (uint32_t)s->d_textures.n;
    info->material_count = (uint32_t)s->d_materials.n;
    info->fused_count = (uint32_t)s->d_mat_fused.n;
    info->cdf_count = (uint32_t)s->d_cdf.n;
    info->guide_count = (uint32_t)s->d_guide.n;
    info->tex_pow2 = D.tex_pow2;
    info->fused_any = D.fused_any;
    info->hdri_buckets = D.hdri_buckets;
    info->hdri_radiance_sum = D.hdri_radiance_sum;
    memcpy(&info->hdri_tex, &D.hdri_tex, sizeof(DevTex));
    info->pool_floats = s->d_tex_pool.n;
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    const char* who = "er_debug_read_textures";
    if ((rc = dump_put(who, table, table_cap, s->d_textures.p, s->d_textures.n * sizeof(DevTex), true, s->stream)) != ER_OK) return rc;
    if ((rc = dump_put(who, pool, pool_cap, s->d_tex_pool.p, s->d_tex_pool.n * sizeof(float), true, s->stream)) != ER_OK) return rc;
    if ((rc = dump_put(who, fused, fused_cap, s->d_mat_fused.p, s->d_mat_fused.n * sizeof(DevFused), true, s->stream)) != ER_OK) return rc;
    if ((rc = dump_put(who, mat_pre, mat_pre_cap, s->d_mat_pre.p, s->d_mat_pre.n * sizeof(float4), true, s->stream)) != ER_OK) return rc;
    if ((rc = dump_put(who, materials, materials_cap, s->d_materials.p, s->d_materials.n * sizeof(ErMaterial), true, s->stream)) != ER_OK) return rc;
    if ((rc = dump_put(who, cdf, cdf_cap, s->d_cdf.p, s->d_cdf.n * sizeof(float), true, s->stream)) != ER_OK) return rc;
    if ((rc = dump_put(who, guide, guide_cap, s->d_guide.p, s->d_guide.n * sizeof(uint32_t), true, s->stream)) != ER_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ER_OK;
}

static int er_debug_bvh_dump_impl(const float* vertices, const float* normals, uint32_t tri_count, int threads, ErAccelDump* info, void* nodes, uint64_t nodes_cap,
                                  void* nodes8, uint64_t nodes8_cap, uint32_t* slot_to_tri, uint64_t slot_cap, float* tri_lift, uint64_t lift_cap) {
    if (!info || (tri_count && (!vertices || !normals))) return fail(ER_ERR_INVALID_ARG, "er_debug_bvh_dump: NULL argument");
    ErBvhBuild b;
    er_build_bvh(vertices, normals, tri_count, threads, &b);
    memset(info, 0, sizeof(*info));
    info->tri_count = tri_count;
    info->node_count = (uint32_t)b.nodes.size();
    info->node8_count = (uint32_t)b.nodes8.size();
    info->node8_pieces = sizeof(ErNode8) / 16;
    info->max_depth = b.max_depth;
    info->max_depth8 = b.max_depth8;
    for (int a = 0; a < 3; a++) { info->lo[a] = b.lo[a]; info->hi[a] = b.hi[a]; }
    info->lift_bound = info->max_lift = b.lift_bound;
    if (!nodes && !nodes8 && !slot_to_tri && !tri_lift) return ER_OK;
    int rc;
    const char* who = "er_debug_bvh_dump";
    if ((rc = dump_put(who, nodes, nodes_cap, b.nodes.data(), (uint64_t)b.nodes.size() * sizeof(ErNode), false, nullptr)) != ER_OK) return rc;
    if ((rc = dump_put(who, nodes8, nodes8_cap, b.nodes8.data(), (uint64_t)b.nodes8.size() * sizeof(ErNode8), false, nullptr)) != ER_OK) return rc;
    if ((rc = dump_put(who, slot_to_tri, slot_cap, b.slot_to_tri.data(), (uint64_t)tri_count * 4, false, nullptr)) != ER_OK) return rc;
    return dump_put(who, tri_lift, lift_cap, b.tri_lift.data(), (uint64_t)tri_count * 4, false, nullptr);
}

// What a spill buffer of er_launch_debug_trace, filled with 0xFF bytes before the launch, says after it: levels[i] = the leading levels of
// ray i's own column that hold an entry.  Returns what is wrong ("" = nothing): an entry above an unwritten level of its column, at or
// above level `usable`, or in the column of a lane that had no ray.
static std::string spill_levels_of(const uint2* spilled, uint32_t n, uint32_t usable, uint32_t* levels) {
    const uint32_t blocks = (n + 63) / 64;
    auto written = [](const uint2& e) { return e.x != 0xFFFFFFFFu || e.y != 0xFFFFFFFFu; };
    auto where = [](uint32_t b, uint32_t l, uint32_t k) { return "block " + std::to_string(b) + " lane " + std::to_string(l) + " level " + std::to_string(k); };
    for (uint32_t b = 0; b < blocks; b++)
        for (uint32_t l = 0; l < 64; l++) {
            const uint2* col = spilled + (size_t)b * ER_STACK8 * 64 + l;
            const uint32_t ray = b * 64 + l;
            uint32_t lead = 0;
            while (lead < (uint32_t)ER_STACK8 && written(col[(size_t)lead * 64])) lead++;
            for (uint32_t k = lead; k < (uint32_t)ER_STACK8; k++)
                if (written(col[(size_t)k * 64])) return where(b, l, k) + " holds an entry above the unwritten level " + std::to_string(lead);
            if (ray >= n) {
                if (lead) return where(b, l, 0) + " holds an entry, and the lane had no ray";
                continue;
            }
            if (lead > usable) return where(b, l, lead - 1) + " holds an entry, and the wide tree has only " + std::to_string(usable) + " levels beyond the LDS ones";
            levels[ray] = lead;
        }
    return "";
}

// spill_levels != nullptr: er_debug_trace_rays_levels.  The spill buffer is filled with 0xFF bytes before the launch -- a pushed entry's
// second word is nmask | imask << 8 (trav_choose), at most 0xFFFF, so the fill can never be an entry -- and read back after it: block b's
// region is ER_STACK8 levels of 64 columns, lane l's column the entries l, 64 + l, ...  (er_debug.hip: spill_base + b * ER_STACK8 * 64 + l).
static int er_debug_trace_rays_impl(ErScene* s, const float* origins, const float* dirs, uint32_t n, const int32_t* self_slots, const float* limits,
                                    int32_t* tri_ids, int32_t* slots, float* positions, float* distances, int32_t* info,
                                    uint32_t* spill_levels = nullptr) {
    if (!s || !origins || !dirs || !tri_ids || !slots || !positions || !distances || !info || (self_slots && !limits))
        return fail(ER_ERR_INVALID_ARG, "er_debug_trace_rays: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_debug_trace_rays: er_render_begin has not succeeded");
    HIP_TRY(hipSetDevice(s->device));
    ScopedDevBuf<float> d_o, d_d, d_pos, d_dist, d_lim;
    ScopedDevBuf<int32_t> d_tri, d_slot, d_info, d_self;
    ScopedDevBuf<uint2> d_spill;
    int rc;
    if ((rc = upload(d_o, origins, (size_t)n * 3, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_d, dirs, (size_t)n * 3, s->stream)) != ER_OK) return rc;
    if (self_slots) {
        // a slot handle must be a triangle slot of this scene (or -1): the kernel indexes the records with it
        for (uint32_t i = 0; i < n; i++)
            if (self_slots[i] < -1 || self_slots[i] >= (int32_t)s->tri_count) return fail(ER_ERR_INVALID_ARG, "er_debug_trace_rays: self slot out of range");
        if ((rc = upload(d_self, self_slots, (size_t)n, s->stream)) != ER_OK) return rc;
        if ((rc = upload(d_lim, limits, (size_t)n, s->stream)) != ER_OK) return rc;
    }
    if ((rc = upload(d_pos, (const float*)nullptr, (size_t)n * 3, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_dist, (const float*)nullptr, (size_t)n, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_tri, (const int32_t*)nullptr, (size_t)n, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_slot, (const int32_t*)nullptr, (size_t)n, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_info, (const int32_t*)nullptr, (size_t)n, s->stream)) != ER_OK) return rc;
    const size_t spill_entries = (size_t)((n + 63) / 64) * ER_STACK8 * 64;
    if ((rc = upload(d_spill, (const uint2*)nullptr, spill_entries, s->stream)) != ER_OK) return rc;
    if (spill_levels && spill_entries) HIP_TRY(hipMemsetAsync(d_spill.p, 0xFF, spill_entries * sizeof(uint2), s->stream));
    er_launch_debug_trace(s->dev, d_o.p, d_d.p, n, self_slots ? d_self.p : nullptr, self_slots ? d_lim.p : nullptr, d_tri.p, d_slot.p, d_pos.p,
                          d_dist.p, d_info.p, d_spill.p, s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(tri_ids, d_tri.p, (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(slots, d_slot.p, (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(info, d_info.p, (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(positions, d_pos.p, (size_t)n * 12, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(distances, d_dist.p, (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
    std::vector<uint2> spilled(spill_levels ? spill_entries : 0);
    if (!spilled.empty()) HIP_TRY(hipMemcpyAsync(spilled.data(), d_spill.p, spill_entries * sizeof(uint2), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (spill_levels) {
        // a level of the area can hold an entry only if the tree has a level for it: sp stays below the wide depth (er_trav.h)
        const uint32_t depth8 = s->accel.max_depth, lds = er_debug_lds_stack_levels();
        const uint32_t usable = depth8 > lds ? std::min<uint32_t>(depth8 - lds, ER_STACK8) : 0u;
        const std::string bad = spill_levels_of(spilled.data(), n, usable, spill_levels);
        if (!bad.empty()) return fail(ER_ERR_STATE, "er_debug_trace_rays_levels: " + bad);
    }
    return ER_OK;
}

static int er_debug_trace_pixel_impl(ErScene* s, uint32_t idx, ErTraceRec* recs, int max_recs, int* count) {
    if (!s || !recs || !count || max_recs <= 0) return fail(ER_ERR_INVALID_ARG, "er_debug_trace_pixel: bad argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_debug_trace_pixel: er_render_begin has not succeeded");
    if (idx >= s->x_res * s->y_res) return fail(ER_ERR_INVALID_ARG, "er_debug_trace_pixel: pixel index out of range");
    HIP_TRY(hipSetDevice(s->device));
    ScopedDevBuf<ErTraceRec> d_recs;
    ScopedDevBuf<int> d_count;
    ScopedDevBuf<uint2> d_spill;
    int rc;
    if ((rc = upload(d_recs, (const ErTraceRec*)nullptr, (size_t)max_recs, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_count, (const int*)nullptr, 1, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_spill, (const uint2*)nullptr, (size_t)ER_DEBUG_PIXEL_SCRATCH, s->stream)) != ER_OK) return rc;
    er_launch_debug_pixel(s->dev, idx, d_recs.p, max_recs, d_count.p, d_spill.p, s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(count, d_count.p, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (*count > 0) HIP_TRY(hipMemcpy(recs, d_recs.p, sizeof(ErTraceRec) * (size_t)*count, hipMemcpyDeviceToHost));
    return ER_OK;
}

static int er_debug_read_light_table_impl(ErScene* s, int32_t* tri_index, float* cdf, float* prob, uint32_t cap) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_debug_read_light_table: NULL scene");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_debug_read_light_table: er_render_begin has not succeeded");
    const uint32_t m = std::min(cap, s->light_emitters);
    if (m == 0) return ER_OK;
    HIP_TRY(hipSetDevice(s->device));
    ScopedDevBuf<int32_t> d_tri;
    ScopedDevBuf<float> d_cdf;
    int rc;
    if ((rc = upload(d_tri, (const int32_t*)nullptr, m, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_cdf, (const float*)nullptr, m, s->stream)) != ER_OK) return rc;
    ScopedDevBuf<float> d_prob;
    if (prob && (rc = upload(d_prob, (const float*)nullptr, m, s->stream)) != ER_OK) return rc;
    er_launch_light_table_read(s->dev.tri_isect, s->d_light_tab.p, s->tri_count, s->light_emitters, m, d_tri.p, d_cdf.p, prob ? d_prob.p : nullptr, s->stream);
    HIP_TRY(hipGetLastError());
    if (prob) HIP_TRY(hipMemcpyAsync(prob, d_prob.p, sizeof(float) * m, hipMemcpyDeviceToHost, s->stream));
    if (tri_index) HIP_TRY(hipMemcpyAsync(tri_index, d_tri.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, s->stream));
    if (cdf) HIP_TRY(hipMemcpyAsync(cdf, d_cdf.p, sizeof(float) * m, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ER_OK;
}

static int er_debug_read_hdri_trig_impl(ErScene* s, uint32_t* cols, uint32_t col_cap, uint32_t* rows, uint32_t row_cap) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_debug_read_hdri_trig: NULL scene");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_debug_read_hdri_trig: er_render_begin has not succeeded");
    const DevTex& t = s->kept.hdri;
    const size_t nc = std::min<size_t>(col_cap, (size_t)std::max(t.width, 0)), nr = std::min<size_t>(row_cap, (size_t)std::max(t.height, 0));
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t* tab = s->d_guide.p + s->kept.trig_at;
    if (cols && nc) HIP_TRY(hipMemcpyAsync(cols, tab, nc * sizeof(erd::HdriCol), hipMemcpyDeviceToHost, s->stream));
    if (rows && nr) HIP_TRY(hipMemcpyAsync(rows, tab + erd::hdri_trig_row_offset(t.width), nr * sizeof(erd::HdriRow), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ER_OK;
}

static int er_debug_hdri_trig_host_impl(int32_t width, int32_t height, uint32_t* cols, uint32_t* rows) {
    if (width < 0 || height < 0 || (width && !cols) || (height && !rows)) return fail(ER_ERR_INVALID_ARG, "er_debug_hdri_trig_host: bad argument");
    std::vector<uint32_t> tab(erd::hdri_trig_words(width, height));
    er_hdri_trig_host(DevTex{width, height, 3, 0, 0u}, tab.data());
    if (width) memcpy(cols, tab.data(), (size_t)width * sizeof(erd::HdriCol));
    if (height) memcpy(rows, tab.data() + erd::hdri_trig_row_offset(width), (size_t)height * sizeof(erd::HdriRow));
    return ER_OK;
}

static int er_debug_eval_impl(ErScene* s, int kind, const float* in, uint32_t n, uint32_t in_stride, float* out, uint32_t out_stride) {
    static const uint32_t need_in[ER_FN_COUNT] = {1, 7, 7, 29, 29, 29, 3, 2, 4, 1, 2, 3, 1};
    static const uint32_t need_out[ER_FN_COUNT] = {32, 6, 18, 3, 1, 3, 2, 3, 3, 1, 1, 1, 2};
    if (!s || !in || !out) return fail(ER_ERR_INVALID_ARG, "er_debug_eval: NULL argument");
    if (kind < 0 || kind >= ER_FN_COUNT) return fail(ER_ERR_INVALID_ARG, "er_debug_eval: unknown kind");
    if (in_stride < need_in[kind] || out_stride < need_out[kind]) return fail(ER_ERR_INVALID_ARG, "er_debug_eval: stride smaller than the kind's item");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_debug_eval: er_render_begin has not succeeded");
    if (kind == ER_FN_MESH_PICK && ((s->dev.ext_flags & ER_FLAG_MESH_LIGHTS) == 0 || s->light_emitters == 0))
        return fail(ER_ERR_STATE, "er_debug_eval: ER_FN_MESH_PICK needs a render begun with ER_FLAG_MESH_LIGHTS and a non-empty emitter table");
    if (kind == ER_FN_TEXTURE)
        for (uint32_t i = 0; i < n; i++) {
            int32_t id;
            memcpy(&id, &in[(size_t)i * in_stride], 4);
            if (id < -1 || id >= (int32_t)s->textures.size()) return fail(ER_ERR_INVALID_ARG, "er_debug_eval: texture id out of range");
            // The device table may hold a scalar-only texture with its first channel alone, possibly already to the power 2.2
            // (er_render_begin): a fetch from that entry is not a fetch from the scene's texture, so it is refused, not answered.
            if (id >= 0 && (size_t)id < s->tex_mode.size() && s->tex_mode[(size_t)id] != 0)
                return fail(ER_ERR_STATE, "er_debug_eval: texture " + std::to_string(id) + " is kept compacted on the device (first channel" +
                                              (s->tex_mode[(size_t)id] == 2 ? ", to the power 2.2" : "") + "); begin the render with ER_TEX_COMPACT=0 to evaluate ER_FN_TEXTURE on it");
        }
    HIP_TRY(hipSetDevice(s->device));
    ScopedDevBuf<float> d_in, d_out;
    int rc;
    if ((rc = upload(d_in, in, (size_t)n * in_stride, s->stream)) != ER_OK) return rc;
    if ((rc = upload(d_out, (const float*)nullptr, (size_t)n * out_stride, s->stream)) != ER_OK) return rc;
    HIP_TRY(hipMemsetAsync(d_out.p, 0, std::max<size_t>((size_t)n * out_stride, 1) * sizeof(float), s->stream));
    er_launch_debug_eval(s->dev, kind, d_in.p, n, in_stride, d_out.p, out_stride, s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out.p, (size_t)n * out_stride * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ER_OK;
}

static int er_measure_hbm_peak_impl(int device, uint64_t bytes, uint32_t iters, float* copy_GBps, float* read_GBps) {
    if (!copy_GBps || !read_GBps) return fail(ER_ERR_INVALID_ARG, "er_measure_hbm_peak: NULL argument");
    int ndev = er_device_count();
    if (device < 0 || device >= ndev) return fail(ER_ERR_NO_DEVICE, "er_measure_hbm_peak: no such HIP device");
    if (bytes == 0) bytes = 2ull << 30;
    if (iters == 0) iters = 5;
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)(bytes / 16);
    ScopedDevBuf<float4> a, b;
    ScopedDevBuf<float> sink;
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } sg{st};
    int rc;
    if ((rc = upload(a, (const float4*)nullptr, n, st)) != ER_OK) return rc;
    if ((rc = upload(b, (const float4*)nullptr, n, st)) != ER_OK) return rc;
    if ((rc = upload(sink, (const float*)nullptr, 1, st)) != ER_OK) return rc;
    HIP_TRY(hipMemsetAsync(a.p, 0, n * 16, st));
    HIP_TRY(hipMemsetAsync(b.p, 0, n * 16, st));
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    float best_copy = 0, best_read = 0;
    for (uint32_t it = 0; it < iters + 1; it++) {      // the first round warms up
        float ms = 0;
        HIP_TRY(hipEventRecord(ev.a, st));
        er_launch_hbm_copy(a.p, b.p, n, st);
        HIP_TRY(hipEventRecord(ev.b, st));
        HIP_TRY(hipEventSynchronize(ev.b));
        HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
        if (it > 0 && ms > 0) best_copy = std::max(best_copy, (float)(2.0 * n * 16 / (ms * 1e-3) / 1e9));
        HIP_TRY(hipEventRecord(ev.a, st));
        er_launch_hbm_read(a.p, sink.p, n, st);
        HIP_TRY(hipEventRecord(ev.b, st));
        HIP_TRY(hipEventSynchronize(ev.b));
        HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
        if (it > 0 && ms > 0) best_read = std::max(best_read, (float)(1.0 * n * 16 / (ms * 1e-3) / 1e9));
    }
    HIP_TRY(hipGetLastError());
    *copy_GBps = best_copy;
    *read_GBps = best_read;
    return ER_OK;
}

extern "C" void er_debug_set_host_alloc_limit(uint64_t bytes) { g_host_alloc_limit.store(bytes); }


static int er_debug_stream_info_impl(ErScene* s, ErStreamInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_debug_stream_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    memset(out, 0, sizeof(*out));
    out->cost_spread = -1.0;
    if (!s->begun || !(s->params.flags & ER_FLAG_STREAM)) return ER_OK;
    stream_fill_info(s, out);
    return ER_OK;
}

extern "C" {
void er_debug_set_gpu_build_failure(int kind) { er_debug_gpu_build_failure.store(kind < 0 || kind > 3 ? 0 : kind); }
int er_debug_stream_info(ErScene* s, ErStreamInfo* out) { return guarded("er_debug_stream_info", [&]() -> int { return er_debug_stream_info_impl(s, out); }); }
int er_debug_closest_hit(ErScene* s, const float* origins, const float* dirs, uint32_t n, int32_t* tri_ids, float* positions, float* distances) { return guarded("er_debug_closest_hit", [&]() -> int { return er_debug_closest_hit_impl(s, origins, dirs, n, tri_ids, positions, distances); }); }
int er_debug_cdf_search(const float* cdf, int length, const float* values, int32_t* out, int count) { return guarded("er_debug_cdf_search", [&]() -> int { return er_debug_cdf_search_impl(cdf, length, values, out, count); }); }
int er_debug_stream_deal(const uint32_t* owned, uint32_t count, uint32_t tiles_x, uint32_t blocks, int xcd_aware, uint32_t edge, uint32_t* out, uint32_t out_cap, uint32_t* most) {
    return guarded("er_debug_stream_deal", [&]() -> int { return er_debug_stream_deal_impl(owned, count, tiles_x, blocks, xcd_aware, edge, out, out_cap, most); });
}
int er_debug_stream_level(const uint32_t* deal, uint32_t deal_n, uint32_t tiles_x, uint32_t blocks, const uint32_t* cost, uint32_t cost_n, uint32_t cap, uint32_t* out, uint32_t out_cap, uint32_t* most) {
    return guarded("er_debug_stream_level", [&]() -> int { return er_debug_stream_level_impl(deal, deal_n, tiles_x, blocks, cost, cost_n, cap, out, out_cap, most); });
}
int er_debug_stream_balance(ErScene* s, ErStreamBalance* info, uint64_t* wg_ticks, uint32_t* wg_tiles, uint64_t* wg_cost, uint32_t wg_cap, uint32_t* deal, uint32_t deal_cap, uint32_t* tile_cost, uint32_t cost_cap) {
    return guarded("er_debug_stream_balance", [&]() -> int { return er_debug_stream_balance_impl(s, info, wg_ticks, wg_tiles, wg_cost, wg_cap, deal, deal_cap, tile_cost, cost_cap); });
}
int er_debug_stream_form(uint32_t tiles, uint32_t blocks, int light_query, uint32_t tri_count, uint32_t flags, ErStreamForm* out) {
    return guarded("er_debug_stream_form", [&]() -> int { return er_debug_stream_form_impl(tiles, blocks, light_query, tri_count, flags, out); });
}
int er_debug_read_accel(ErScene* s, ErAccelDump* info, void* nodes, uint64_t nodes_cap, void* nodes8, uint64_t nodes8_cap, void* isect, uint64_t isect_cap, void* attr, uint64_t attr_cap) {
    return guarded("er_debug_read_accel", [&]() -> int { return er_debug_read_accel_impl(s, info, nodes, nodes_cap, nodes8, nodes8_cap, isect, isect_cap, attr, attr_cap); });
}
int er_debug_bvh_dump(const float* vertices, const float* normals, uint32_t tri_count, int threads, ErAccelDump* info, void* nodes, uint64_t nodes_cap, void* nodes8, uint64_t nodes8_cap,
                      uint32_t* slot_to_tri, uint64_t slot_cap, float* tri_lift, uint64_t lift_cap) {
    return guarded("er_debug_bvh_dump", [&]() -> int { return er_debug_bvh_dump_impl(vertices, normals, tri_count, threads, info, nodes, nodes_cap, nodes8, nodes8_cap, slot_to_tri, slot_cap, tri_lift, lift_cap); });
}
int er_debug_texture_plan(const ErSceneDesc* d, ErTexturePlan* plan, uint8_t* modes, uint64_t modes_cap, ErTexEntry* table, uint64_t table_cap, ErFusedEntry* fused, uint64_t fused_cap) {
    return guarded("er_debug_texture_plan", [&]() -> int { return er_debug_texture_plan_impl(d, plan, modes, modes_cap, table, table_cap, fused, fused_cap); });
}
int er_debug_read_textures(ErScene* s, ErTextureDump* info, void* table, uint64_t table_cap, void* pool, uint64_t pool_cap, void* fused, uint64_t fused_cap, void* mat_pre,
                           uint64_t mat_pre_cap, void* materials, uint64_t materials_cap, void* cdf, uint64_t cdf_cap, void* guide, uint64_t guide_cap) {
    return guarded("er_debug_read_textures", [&]() -> int {
        return er_debug_read_textures_impl(s, info, table, table_cap, pool, pool_cap, fused, fused_cap, mat_pre, mat_pre_cap, materials, materials_cap, cdf, cdf_cap, guide, guide_cap);
    });
}
int er_debug_accel_cost_terms(ErScene* s, ErCostSumsDebug* sums, double* node_terms, uint64_t node_cap, float* tri_terms, uint64_t tri_cap) {
    return guarded("er_debug_accel_cost_terms", [&]() -> int { return er_debug_accel_cost_terms_impl(s, sums, node_terms, node_cap, tri_terms, tri_cap); });
}
int er_debug_accel_cost_host(const void* nodes8, uint32_t node8_count, uint32_t node8_pieces, const void* isect, uint32_t tri_count, ErCostSumsDebug* sums, double* node_terms,
                             uint64_t node_cap, float* tri_terms, uint64_t tri_cap) {
    return guarded("er_debug_accel_cost_host", [&]() -> int {
        return er_debug_accel_cost_host_impl(nodes8, node8_count, node8_pieces, isect, tri_count, sums, node_terms, node_cap, tri_terms, tri_cap);
    });
}
int er_debug_bvh_check(const float* vertices, const float* normals, uint32_t tri_count, int threads, ErBvhCheck* out) { return guarded("er_debug_bvh_check", [&]() -> int { return er_debug_bvh_check_impl(vertices, normals, tri_count, threads, out); }); }
int er_debug_trace_rays(ErScene* s, const float* origins, const float* dirs, uint32_t n, const int32_t* self_slots, const float* limits, int32_t* tri_ids,
                        int32_t* slots, float* positions, float* distances, int32_t* info) {
    return guarded("er_debug_trace_rays", [&]() -> int { return er_debug_trace_rays_impl(s, origins, dirs, n, self_slots, limits, tri_ids, slots, positions, distances, info); });
}
int er_debug_trace_rays_levels(ErScene* s, const float* origins, const float* dirs, uint32_t n, const int32_t* self_slots, const float* limits, int32_t* tri_ids,
                               int32_t* slots, float* positions, float* distances, int32_t* info, uint32_t* spill_levels, uint32_t* lds_levels, uint32_t* stack_levels) {
    return guarded("er_debug_trace_rays_levels", [&]() -> int {
        if (!spill_levels || !lds_levels || !stack_levels) return fail(ER_ERR_INVALID_ARG, "er_debug_trace_rays_levels: NULL argument");
        *lds_levels = er_debug_lds_stack_levels();
        *stack_levels = ER_STACK8;
        return er_debug_trace_rays_impl(s, origins, dirs, n, self_slots, limits, tri_ids, slots, positions, distances, info, spill_levels);
    });
}
int er_debug_spill_levels(const void* spilled, uint64_t spilled_bytes, uint32_t n, uint32_t usable, uint32_t* levels) {
    return guarded("er_debug_spill_levels", [&]() -> int {
        if (!spilled || !levels) return fail(ER_ERR_INVALID_ARG, "er_debug_spill_levels: NULL argument");
        if (spilled_bytes != (uint64_t)((n + 63) / 64) * ER_STACK8 * 64 * sizeof(uint2)) return fail(ER_ERR_INVALID_ARG, "er_debug_spill_levels: the buffer is not ceil(n / 64) regions of ER_STACK8 x 64 entries");
        const std::string bad = spill_levels_of((const uint2*)spilled, n, usable, levels);
        if (!bad.empty()) return fail(ER_ERR_STATE, "er_debug_spill_levels: " + bad);
        return ER_OK;
    });
}
int er_debug_trace_pixel(ErScene* s, uint32_t idx, ErTraceRec* recs, int max_recs, int* count) {
    return guarded("er_debug_trace_pixel", [&]() -> int { return er_debug_trace_pixel_impl(s, idx, recs, max_recs, count); });
}
int er_debug_read_light_table(ErScene* s, int32_t* tri_index, float* cdf, uint32_t cap) {
    return guarded("er_debug_read_light_table", [&]() -> int { return er_debug_read_light_table_impl(s, tri_index, cdf, nullptr, cap); });
}
int er_debug_read_light_table_prob(ErScene* s, int32_t* tri_index, float* cdf, float* prob, uint32_t cap) {
    return guarded("er_debug_read_light_table_prob", [&]() -> int { return er_debug_read_light_table_impl(s, tri_index, cdf, prob, cap); });
}
int er_debug_read_hdri_trig(ErScene* s, uint32_t* cols, uint32_t col_cap, uint32_t* rows, uint32_t row_cap) {
    return guarded("er_debug_read_hdri_trig", [&]() -> int { return er_debug_read_hdri_trig_impl(s, cols, col_cap, rows, row_cap); });
}
int er_debug_hdri_trig_host(int32_t width, int32_t height, uint32_t* cols, uint32_t* rows) {
    return guarded("er_debug_hdri_trig_host", [&]() -> int { return er_debug_hdri_trig_host_impl(width, height, cols, rows); });
}
int er_debug_eval(ErScene* s, int kind, const float* in, uint32_t n, uint32_t in_stride, float* out, uint32_t out_stride) {
    return guarded("er_debug_eval", [&]() -> int { return er_debug_eval_impl(s, kind, in, n, in_stride, out, out_stride); });
}
int er_measure_hbm_peak(int device, uint64_t bytes, uint32_t iters, float* copy_GBps, float* read_GBps) {
    return guarded("er_measure_hbm_peak", [&]() -> int { return er_measure_hbm_peak_impl(device, bytes, iters, copy_GBps, read_GBps); });
}
int er_debug_transform_apply(const float* m, uint32_t count, const float* v, const float* n, const float* t, float* ov, float* on, float* ot) {
    return guarded("er_debug_transform_apply", [&]() -> int {
        if (!m || (count && (!v || !n || !t || !ov || !on || !ot))) return fail(ER_ERR_INVALID_ARG, "er_debug_transform_apply: NULL argument");
        if (!er_xform_apply(m, count, v, n, t, ov, on, ot)) return fail(ER_ERR_INVALID_ARG, "er_debug_transform_apply: a matrix entry is not finite, or det(L) is not > 0");
        return ER_OK;
    });
}
int er_debug_skin_apply(const float* palette, uint32_t bone_count, uint32_t count, const uint16_t* bones, const float* weights, const float* v, const float* n, const float* t,
                        float* ov, float* on, float* ot) {
    return guarded("er_debug_skin_apply", [&]() -> int {
        if (!palette || (count && (!bones || !weights || !v || !n || !t || !ov || !on || !ot))) return fail(ER_ERR_INVALID_ARG, "er_debug_skin_apply: NULL argument");
        std::string why;
        if (!er_skin_apply(palette, bone_count, count, bones, weights, v, n, t, ov, on, ot, why)) return fail(ER_ERR_INVALID_ARG, "er_debug_skin_apply: " + why);
        return ER_OK;
    });
}
int er_debug_id_rank(const uint32_t* ids, uint32_t count, uint32_t* out_ids, uint32_t* out_counts, uint32_t* distinct) {
    return guarded("er_debug_id_rank", [&]() -> int {
        if ((count && !ids) || !out_ids || !out_counts || !distinct) return fail(ER_ERR_INVALID_ARG, "er_debug_id_rank: NULL argument");
        if (count > 64) return fail(ER_ERR_INVALID_ARG, "er_debug_id_rank: at most 64 ids");
        *distinct = er_id_rank(ids, 1, count, out_ids, out_counts);
        return ER_OK;
    });
}
}  // extern "C"
