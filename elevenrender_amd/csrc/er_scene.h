// er_scene.h -- host-side state behind the opaque ErScene handle of include/eleven_hip.h, and the small helpers the
// translation units of the boundary share (er_api.cpp: the drop-in entry points; er_api_edit.cpp: the in-place edits; er_stream_host.cpp: the streaming schedule's host
// side; er_debug_api.cpp: inspection hooks of include/eleven_hip_debug.h; er_collective.cpp: the RCCL framebuffer combine).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/eleven_hip.h"
#include "er_bvh.h"
#include "er_devbuf.h"
#include "er_device.h"
#include "er_gpu_build.h"
#include "er_kernels.h"
#include "er_wavefront.h"
#include "er_stream.h"
#include "er_stream_host.h"
#include "er_adaptive.h"
#include "er_lights.h"
#include "er_refit.h"
#include "er_cost.h"
#include "er_texplan.h"
#include "er_texstage.h"
#include "er_features.h"
#include "er_ids.h"
#include "er_history.h"
#include "er_variance_state.h"
#include "er_topology.h"

namespace erh {


inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg) noexcept {
    try { g_err = msg; } catch (...) { /* keeping the previous text beats unwinding through the C ABI */ }
    return code;
}

// Every extern "C" entry point runs its body through this: the header promises "never throws", and the bodies
// allocate (std::vector, std::string, std::map) -- a std::bad_alloc must come back as ER_ERR_OOM, not unwind
// through the C ABI into a host that may not even be C++ (reference: errors are logged and never propagated,
// src/Managers.cpp:244-246).
template <class F>
int guarded(const char* who, F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(ER_ERR_OOM, std::string(who) + ": out of host memory");
    } catch (const std::exception& e) {
        return fail(ER_ERR_STATE, std::string(who) + ": " + e.what());
    } catch (...) {
        return fail(ER_ERR_STATE, std::string(who) + ": unknown exception");
    }
}

// Test hook (include/eleven_hip_debug.h, er_debug_set_host_alloc_limit): the library's large host allocations
// announce their size here first, so the out-of-memory path can be exercised without exhausting the machine.
inline std::atomic<uint64_t> g_host_alloc_limit{0};
inline void host_reserve(uint64_t bytes) {
    const uint64_t lim = g_host_alloc_limit.load();
    if (lim && bytes > lim) throw std::bad_alloc();
}

struct EventPair {      // two timing events that do not outlive the function that made them
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess)                                                                          \
            return fail(e__ == hipErrorOutOfMemory ? ER_ERR_OOM : ER_ERR_HIP,                           \
                        std::string(#expr) + ": " + hipGetErrorString(e__));                            \
    } while (0)

struct HostTex {
    int32_t width, height, channels, filter;
    std::vector<float> data;
};

// Texture::getValueFromCoordinates, reference src/Texture.cpp:172-200 (host copy, used by the CDF)
inline void host_tex_coords(const HostTex& t, int x, int y, float out[3]) {
    x %= t.width;
    y %= t.height;
    if (x < 0) x *= -1;
    if (y < 0) y *= -1;
    out[0] = out[1] = out[2] = 0.0f;
    const float* d = t.data.data();
    if (t.channels == 1) {
        out[0] = out[1] = out[2] = d[y * t.width + x];
    } else if (t.channels == 2) {
        out[0] = d[t.channels * (y * t.width + x) + 0];
        out[1] = d[t.channels * (y * t.width + x) + 1];
    } else if (t.channels >= 3) {
        out[0] = d[t.channels * (y * t.width + x) + 0];
        out[1] = d[t.channels * (y * t.width + x) + 1];
        out[2] = d[t.channels * (y * t.width + x) + 2];
    }
}

// HDRI::generateCDF, reference src/HDRI.cpp:62-83 (host preparation, same float sequence)
inline void host_generate_cdf(const HostTex& t, std::vector<float>& cdf, float& radianceSum) {
    int c = 0;
    radianceSum = 0;
    cdf.assign((size_t)t.width * t.height + 1, 0.0f);
    float p[3];
    for (int j = 0; j < t.height; j++)
        for (int i = 0; i < t.width; i++) {
            host_tex_coords(t, i, j, p);
            radianceSum += p[0] + p[1] + p[2];
        }
    for (int j = 0; j < t.height; j++)
        for (int i = 0; i < t.width; i++) {
            host_tex_coords(t, i, j, p);
            cdf[c + 1] = cdf[c] + (p[0] + p[1] + p[2]) / radianceSum;
            c++;
        }
}

}  // namespace erh

using erh::DevBuf;
using erh::HostTex;

struct ErScene {
    // host copy of the description
    uint32_t tri_count = 0;
    std::vector<float> vertices, normals, tangents, uvs, tangent_sign;
    std::vector<int32_t> material_id;
    std::vector<ErMaterial> materials;
    std::vector<HostTex> textures;
    HostTex hdri_tex;
    std::vector<float> hdri_cdf;
    float hdri_radiance_sum = 0;
    ErCamera camera;
    std::vector<ErPointLight> point_lights;
    uint32_t x_res = 0, y_res = 0;

    // render state
    bool begun = false;
    int device = 0;
    ErRenderParams params{};
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    bool timing_open = false;
    DevScene dev{};
    ErAccelInfo accel{};
    float accel_lo[3] = {0, 0, 0}, accel_hi[3] = {0, 0, 0};   // scene bounds as the builder reported them (er_debug_read_accel)
    uint32_t accel_depth2 = 0;                                 // levels of the binary tree (the same hook)
    // What a restart in place (er_render_update, er_render_edit: er_api_edit.cpp) needs of the stages it does not run again.  Each value
    // is written once, by the stage that produces it, and read by begin_render_state and begin_descriptor (er_api.cpp), whoever calls
    // them: the structure's counts, depths, bounds and lift bound (begin_accel; a refit replaces bounds and lift bound), the HDRI's
    // table entry and the buckets of its search guide (begin_textures; the pool stage of an edit), the device's CUs and the flags as
    // the caller gave them (er_render_begin; params.flags holds the schedule that was chosen).
    struct Kept {
        ErGpuBvhDevice accel;      // (its three pointers are null: the scene owns the buffers)
        DevTex hdri{};
        int buckets = 0;
        size_t trig_at = 0;        // where the HDRI's row and column tables begin in d_guide (words; er_hdri_trig.h)
        uint32_t cus = 0, flags = 0;
    } kept;
    ErRefitTopo refit_topo;      // the trees' nodes by level, from the first refit after an er_render_begin until the next one
    ErUpdateInfo upd{};          // er_update_info (counts since er_scene_create)
    ErEditInfo edit{};           // er_edit_info (the same)
    ErSparseInfo sparse{};       // er_sparse_info (the same)
    // er_objects_set / er_render_transform (er_xform.h): the object table with the rest copy and the lazy half of the host copy -- call
    // er_objects_flush(objects, ...) before reading or partly overwriting vertices, normals or tangents --, its device form (built by the
    // first transform after er_objects_set or er_render_begin), and what er_transform_info reports: the last transform's figures in an
    // ErSparseInfo (calls, moved and the rest mean the same) and its listed objects.
    ErObjectTable objects;
    ErXformDev xform_dev;
    ErSparseInfo xform{};
    uint32_t xform_objects = 0;
    // er_skin_set / er_render_skin (er_skin.h): the skins beside the object table (empty until the first er_skin_set), the influences'
    // device form (built by the first er_render_skin after er_skin_set or er_render_begin), and what er_skin_info reports, as above.
    ErSkinTable skins;
    ErSkinDev skin_dev;
    ErSparseInfo skin{};
    uint32_t skin_objects = 0, skin_bones = 0;
    uint64_t skin_influence_bytes = 0;
    // er_render_topology (er_api_edit.cpp): the geometry store -- the six arrays on the device in id order, valid from a
    // topology edit whose build ran on the device until anything else writes geometry or material ids (store.release() there) -- and
    // what er_topology_info reports.
    ErGeomStore store;
    ErTopologyInfo topo{};
    void flush_poses() noexcept { er_skin_flush(objects, skins, vertices.data(), normals.data(), tangents.data()); }      // (both kinds of pending pose)
    // er_accel_cost / er_update_policy_set (er_api_edit.cpp): every build and every refit bumps accel_version; the cost last measured is kept
    // with the version it was measured at.  The baseline of ER_REBUILD_AUTO is the cost of the last BUILT tree: known once such a tree
    // has been measured, forgotten with the next build.
    uint64_t accel_version = 0, cost_version = ~0ull;
    ErAccelCost cost_kept{};
    bool baseline_known = false;
    double baseline_cost = 0;
    ErUpdatePolicy policy{ER_REBUILD_NEVER, 0.0f};      // lasts until er_scene_destroy
    ErRebuildInfo rebuild{};                           // er_rebuild_info (counts since er_scene_create; mode and ratio are filled from `policy`)
    size_t tex_pool_cap = 0;     // floats the allocation of d_tex_pool holds (d_tex_pool.n: the floats of the pool in it; an HDRI edit may shrink that)
    DevBuf<float4> d_nodes, d_nodes8, d_attr, d_passes;
    DevBuf<float4> d_plane;      // staging: one pass gathered as a plane for er_read_pass
    DevBuf<ErMaterial> d_materials;
    DevBuf<float4> d_mat_pre;    // DevScene::mat_pre
    DevBuf<ErPointLight> d_lights;
    DevBuf<float> d_light_tab;       // ER_FLAG_MESH_LIGHTS: the emitter table (er_lights.h), empty without emitters
    uint32_t light_emitters = 0;     //   its entries
    float light_total = 0.0f;        //   W, the sum of their weights
    DevBuf<DevTex> d_textures;
    DevBuf<float> d_tex_pool, d_cdf;
    DevBuf<uint32_t> d_samples, d_rng, d_owned;
    DevBuf<DevCounters> d_counters;
    std::vector<uint8_t> tex_mode;   // per texture, how the device table holds it: 0 as it came, 1 first channel alone, 2 first channel alone to the power 2.2 (er_render_begin)
    bool fused_any = false;          // some material's textures are fused
    DevBuf<DevFused> d_mat_fused;   // per material: its fused albedo / roughness / metallic texels in d_tex_pool, or width 0
    DevBuf<DevScene> d_dev;      // device copy of `dev`: the streaming kernel reads the scene descriptor through a pointer
    DevBuf<float4> d_wf4;        // 11 float4 arrays of the wavefront state, back to back
    DevBuf<uint32_t> d_wf1;      // hit, left, occluded, 4 queues, counts
    DevBuf<uint2> d_spill;
    DevBuf<uint32_t> d_guide;
    StreamHost st;               // the streaming schedule's host state (er_stream_host.h); its records, control words and spill live in d_wf4, d_wf1, d_spill
    // adaptive sampling (er_adaptive_set, er_api.cpp): the active tiles as a device list in the layout of er_adaptive.h, two buffers
    // that the test's compaction writes in turn; ad_dev = `dev` with owned_tiles pointing at the active list (wavefront, megakernel)
    uint32_t rendered = 0;                // samples given to every active tile since er_render_begin (adaptive or not)
    bool ad_on = false;
    float ad_threshold = 0;
    uint32_t ad_interval = 0, ad_next = 0, ad_tests = 0, ad_cur = 0;   // ad_cur: which of d_ad_list holds the active list
    bool ad_snapped = false;              // the snapshot for the next test has been taken
    float ad_max_error = -1.0f;
    uint64_t ad_pixel_samples = 0, ad_active_px = 0;    // samples given to owned pixels; in-frame pixels of the active tiles
    std::vector<uint32_t> ad_active, ad_tile_samples;   // host copy of the active list; samples per tile of the frame
    DevBuf<uint32_t> d_ad_list[2], d_ad_keep;
    DevBuf<float4> d_ad_snap;
    DevBuf<float> d_ad_err;
    DevScene ad_dev{};
    std::vector<WfState> wf;              // slot pools (see er_render_begin)
    std::vector<hipStream_t> pool_streams;   // pool 0 runs on `stream`, pool p > 0 on pool_streams[p - 1]
    std::vector<hipEvent_t> pool_events;     // [0] fork; [p] pool p has finished

    uint32_t trace_blocks = 0, shade_blocks = 0;
    std::vector<hipEvent_t> prof_events;   // ER_FLAG_PROFILE: e[3i], e[3i+1], e[3i+2] = before trace, between, after shade
    DevBuf<uint32_t> d_ray_log;            // ER_FLAG_PROFILE, wavefront: rays found by the i-th trace launch (same order)
    size_t prof_used = 0;
    ErProfile profile{};
    std::map<uint32_t, DevBuf<uint32_t>> d_rank_tiles;   // tile lists of other ranks (for unpack)
    // er_gather_pass: the packed owned pixels of this rank (non-root) and one receive buffer per peer (root), allocated at the first
    // gather and kept for the scene's life -- a read-back of five planes from seven peers was 35 hipMalloc / hipFree pairs inside the
    // time the gather is measured by; now it is pack + wire + unpack
    DevBuf<float4> d_gather_mine;
    std::map<uint32_t, DevBuf<float4>> d_gather_in;
    // which ranks' pixels of each plane were unpacked into this scene since the last sample was enqueued: er_denoise on a
    // sharded frame needs the whole BEAUTY and NORMAL planes (the rank the frame was gathered to)
    std::set<uint32_t> unpacked[ER_PASS_COUNT];
    // the first-hit camera pass (er_first_hit.h) of er_render_features, er_render_ids, er_pick and the history's key: the traversal's
    // spill area of its bounded grid (the consumers run one at a time on the scene's stream), and what a whole-frame pass reports
    DevBuf<uint2> d_first_hit_spill;
    // its mode (er_first_hit_set, er_first_hit.hip): set after er_render_begin and kept through every edit and a later er_render_begin;
    // threshold as resolved (0 -> 0.5).  counts: ErFirstHitInfo's five, of the last whole-frame pass run with the mode on, through
    // d_first_hit_counts (five words 64 bytes apart, allocated by the first such pass).
    struct FirstHitMode { uint32_t cutouts = 0; float threshold = 0.5f; uint64_t counts[5] = {0, 0, 0, 0, 0}; } first_hit;
    DevBuf<unsigned long long> d_first_hit_counts;
    struct PassInfo { bool valid = false; uint32_t samples = 0; uint64_t rays = 0; float ms = 0; };
    // the feature pass (er_features.hip): the ALBEDO and DEPTH planes back to back (row-major, allocated by the first er_render_features);
    // valid from a pass until the next er_render_begin or er_render_update.  Recomputable, so not part of the progressive state.
    // unpacked_feat: as `unpacked`, since the last pass.
    DevBuf<float4> d_feat;
    PassInfo feat;
    std::set<uint32_t> unpacked_feat[ER_FEATURE_COUNT];
    // the id pass (er_ids.hip): per kind an id plane and a count plane, 16 bytes per pixel each, back to back -- plane 2 * kind + 0 /
    // + 1, row-major, allocated by the first er_render_ids; ids.valid from a pass until the next er_render_begin, edit of any kind or
    // er_objects_set (ids_invalidate).  d_id_map: tri -> object of the current table (tri_count words), made again when the table
    // changed.  d_id_work: the words the consumers work in, grown on demand and kept (er_pick_rect: marks, block counts, offsets, the
    // selection; er_id_matte: the plane and the list; er_pick: one ErPick).  d_id_over: the pass's three overflow counters.
    DevBuf<float4> d_id_planes;
    DevBuf<uint32_t> d_id_map, d_id_work, d_id_over;
    PassInfo ids;
    bool id_map_valid = false;
    uint32_t ids_objects = 0, ids_overflow[ER_ID_KIND_COUNT] = {0, 0, 0};
    void ids_invalidate() noexcept { ids.valid = false; }
    // the temporal reprojection (er_history.hip): key planes, the captured colours and the resolved history; dropped by whatever changes
    // the look or moves a triangle other than by a pose (history_invalidate)
    ErHistoryState hist;
    void history_invalidate() noexcept { hist.invalidate(); }
    // the variance plane (er_variance.hip): the batch-mean moments of every pixel since the render last started over (variance_reset:
    // er_render_begin and every edit; er_state_import snapshots what it brought)
    ErVarianceState var;
    void variance_reset() noexcept { var.reset(); }
    std::mutex mtx;

    uint32_t tiles_x() const { return (x_res + ER_TILE - 1) / ER_TILE; }      // the frame in tiles of ER_TILE x ER_TILE pixels
    uint32_t tiles_y() const { return (y_res + ER_TILE - 1) / ER_TILE; }
    // point-light queries are on (they double the shadow records and the shadow queues of the wavefront schedule, er_wavefront.h) ...
    bool lights_on() const { return (kept.flags & ER_FLAG_POINT_LIGHTS) != 0 && !point_lights.empty(); }
    // ... and so is the second shadow record per slot: the point-light or the emitter query (after the emitter stage: an edit can create
    // the first emitter or remove the last)
    bool query_on() const { return lights_on() || light_emitters > 0; }
    std::vector<uint32_t> tiles_of(uint32_t rank, uint32_t world) const {
        std::vector<uint32_t> t;
        const uint32_t nx = tiles_x(), ny = tiles_y();
        for (uint32_t ty = 0; ty < ny; ty++)
            for (uint32_t tx = 0; tx < nx; tx++)
                if ((tx + ty) % world == rank) t.push_back(ty * nx + tx);
        return t;
    }
    uint32_t tile_pixels(uint32_t tile) const {      // pixels of a tile inside the frame
        const uint32_t nx = tiles_x(), tx = tile % nx, ty = tile / nx;
        return std::min<uint32_t>(ER_TILE, x_res - tx * ER_TILE) * std::min<uint32_t>(ER_TILE, y_res - ty * ER_TILE);
    }
    uint64_t owned_pixels() const {      // ... and of this rank's share of the frame
        uint64_t px = 0;
        for (uint32_t t : tiles_of(params.rank, params.world)) px += tile_pixels(t);
        return px;
    }
    void release_device() {
        d_nodes.release(); d_nodes8.release(); d_attr.release(); d_passes.release(); d_plane.release(); d_materials.release();
        d_textures.release(); d_tex_pool.release(); tex_pool_cap = 0; d_lights.release(); d_cdf.release(); d_samples.release(); d_rng.release();
        d_owned.release(); d_counters.release(); d_wf4.release(); d_wf1.release(); d_spill.release(); d_guide.release(); d_ray_log.release(); d_mat_fused.release(); d_mat_pre.release(); d_dev.release();
        st.release();
        d_ad_list[0].release(); d_ad_list[1].release(); d_ad_keep.release(); d_ad_snap.release(); d_ad_err.release();
        d_light_tab.release(); light_emitters = 0; light_total = 0.0f;
        refit_topo.release();
        xform_dev.release();
        skin_dev.release();
        store.release();
        d_first_hit_spill.release(); d_first_hit_counts.release();
        for (auto& c : first_hit.counts) c = 0;      // (the mode itself stays: er_first_hit_set)
        d_feat.release(); feat.valid = false;
        for (auto& u : unpacked_feat) u.clear();
        d_id_planes.release(); d_id_map.release(); d_id_work.release(); d_id_over.release(); ids.valid = id_map_valid = false;
        hist.release();
        var.release();
        ad_on = false; rendered = 0;
        for (auto& kv : d_rank_tiles) kv.second.release();
        d_rank_tiles.clear();
        d_gather_mine.release();
        for (auto& kv : d_gather_in) kv.second.release();
        d_gather_in.clear();
        for (hipEvent_t e : prof_events) (void)hipEventDestroy(e);
        prof_events.clear();
        prof_used = 0;
        for (hipEvent_t e : pool_events) (void)hipEventDestroy(e);
        pool_events.clear();
        for (hipStream_t st : pool_streams) (void)hipStreamDestroy(st);
        pool_streams.clear();
        wf.clear();
        if (ev_start) (void)hipEventDestroy(ev_start);
        if (ev_stop) (void)hipEventDestroy(ev_stop);
        if (stream) (void)hipStreamDestroy(stream);
        ev_start = ev_stop = nullptr;
        stream = nullptr;
        begun = false;
        timing_open = false;
    }
};

// ER_OK unless the streaming schedule's watchdog ended a call early (er_stream_host.cpp); call with the scene's stream idle and its
// mutex held.  Every entry point that hands planes out (read-backs, snapshot, gather, pack, denoise) ends with it.
extern "C" __attribute__((visibility("hidden"))) int er_scene_stream_status(ErScene* s, const char* who);   // (library-internal)

namespace erh {

// guide table of er_cdf.h: guide[j] = first i in [0,length] with cdf[i] >= j/buckets
inline int er_build_cdf_guide(const float* cdf, int length, std::vector<uint32_t>& guide) {
    // entries per bucket on average (buckets = a power of two >= length / per): every halving takes one dependent load off the
    // CDF search of every shading step and doubles the table (4 bytes per bucket).  C2 (2048x1024 HDRI): 8 -> 1362 / 1367,
    // 2 -> 1374 / 1375, 1 -> 1373 / 1372 Msamples/s on one box (profiles/r03_ab_cdf_buckets.log): 2 (a 4 MB table there).
    static const int per = [] { const char* e = getenv("ER_CDF_ENTRIES_PER_BUCKET"); int v = e ? atoi(e) : 2; return v < 1 ? 1 : v; }();
    int buckets = 1;
    while (buckets < length / per && buckets < (1 << 22)) buckets <<= 1;
    guide.assign((size_t)buckets + 1, (uint32_t)length);
    int i = 0;
    for (int j = 0; j <= buckets; j++) {
        float thr = (float)j / (float)buckets;
        while (i < length && cdf[i] < thr) i++;
        guide[j] = (uint32_t)i;
    }
    return buckets;
}

template <class T>
int upload(DevBuf<T>& b, const void* src, size_t count, hipStream_t s) {
    b.release();
    size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    HIP_TRY(hipMalloc((void**)&b.p, bytes));
    b.n = count;
    if (count && src) HIP_TRY(hipMemcpyAsync(b.p, src, count * sizeof(T), hipMemcpyHostToDevice, s));
    return ER_OK;
}

// The two range rules of a scene's lists, for er_scene_create and for the lists an edit would leave (er_api_edit.cpp).
inline void texture_ids(const ErMaterial& m, int32_t out[7]) {
    const int32_t ids[7] = {m.albedo_tex, m.emission_tex, m.roughness_tex, m.metallic_tex, m.normal_tex, m.opacity_tex, m.transmission_tex};
    memcpy(out, ids, sizeof(ids));
}
// every texture id of every material is below `ntex` (a negative id means "no texture")
inline int check_texture_ids(const ErMaterial* mats, size_t nmat, size_t ntex, const char* who) {
    for (size_t m = 0; m < nmat; m++) {
        int32_t ids[7];
        texture_ids(mats[m], ids);
        for (int32_t id : ids)
            if (id >= (int32_t)ntex) return fail(ER_ERR_INVALID_ARG, std::string(who) + ": texture id out of range");
    }
    return ER_OK;
}
// every triangle's material id names one of `nmat` materials
inline int check_material_ids(const int32_t* ids, size_t n, size_t nmat, const char* who) {
    for (size_t i = 0; i < n; i++)
        if (ids[i] < 0 || (uint32_t)ids[i] >= nmat) return fail(ER_ERR_INVALID_ARG, std::string(who) + ": material_id out of range");
    return ER_OK;
}

inline int check_tex(const ErTexture& in, const char* what) {      // what er_scene_create (and er_render_edit) refuse of a texture
    if (in.width <= 0 || in.height <= 0 || in.channels < 0 || (in.channels > 0 && !in.data))
        return fail(ER_ERR_INVALID_ARG, std::string("bad texture: ") + what);
    return ER_OK;
}

inline int copy_tex(const ErTexture& in, HostTex& out, const char* what) {
    if (check_tex(in, what) != ER_OK) return ER_ERR_INVALID_ARG;
    out.width = in.width; out.height = in.height; out.channels = in.channels; out.filter = in.filter;
    size_t n = (size_t)in.width * in.height * in.channels;
    out.data.assign(in.data, in.data + n);
    return ER_OK;
}


}  // namespace erh
