// er_api_edit.cpp -- er_render_update and er_render_edit (include/eleven_hip.h): a begun scene edited in place.  Both entry points are
// ONE function, edit_locked: every check with nothing touched, the host copy replaced, then the device stages the edit reaches --
// geometry, materials, pool, emitters -- and always edit_restart: the render's own state exactly as er_render_begin sets it up
// (begin_render_state, er_api_stages.h).  Also here: what the geometry stage decides by (er_accel_cost, er_update_policy_set) and the
// info getters.  er_render_update_sparse is the same function once more: its list of moved triangles (er_sparse_host.h) takes the place
// of the complete arrays in the checks, in the replacement of the host copy and in the refit, and nothing else knows of it.
// er_render_transform is the same function a third time: its list of posed OBJECTS (er_xform.h) takes the place of the sparse list in the
// same three places -- checked in O(objects), the host copy only marked (ErScene::flush_poses applies the marks where the arrays are
// read), the listed triangles posed on the device by the refit itself.  Also here: er_objects_set.
// er_render_skin is er_render_transform with palettes in place of matrices (er_skin.h): the same list type with its `skin` half filled, a
// branch in each of the same three places.  Also here: er_skin_set.
// er_render_topology (at the end) changes WHICH triangles there are: its own checks and renumbering (er_topology_host.h), the checks and
// the replacement of edit_locked for its `rest`, the geometry store (er_topology.h) in front of begin_accel, then the same stages.
#include <algorithm>
#include <chrono>

#include "er_api_stages.h"
#include "er_topology_host.h"

using namespace erh;

static_assert(ER_TOPO_REMOVE == ER_TOPO_HOST_REMOVE && ER_TOPO_APPEND == ER_TOPO_HOST_APPEND, "er_topology_host.h restates the two bits");

static_assert(ER_EDIT_CAMERA == ER_UPDATE_CAMERA && ER_EDIT_GEOMETRY == ER_UPDATE_GEOMETRY, "an ErSceneUpdate's bits are the first two of an ErSceneEdit");

namespace {

const uint32_t LOOK_BITS = ER_EDIT_MATERIALS | ER_EDIT_TEXTURES | ER_EDIT_HDRI;      // what er_render_edit adds to er_render_update

// er_render_transform's list: the caller's transforms, and what the checks derive from them (the upload entries, the triangles moved)
struct XformList {
    uint32_t count = 0;
    const ErObjectTransform* x = nullptr;
    std::vector<ErXformEntry> entries;
    uint32_t moved = 0;
    // er_render_skin: the caller's poses in place of `x`, and the entries and the palettes that go up in place of `entries`
    const ErSkinPose* poses = nullptr;
    bool skin = false;
    std::vector<ErSkinEntry> skin_entries;
    std::vector<float> palette;
};

static_assert(ER_SKIN_INFLUENCES == ER_SKIN_K && ER_SKIN_MAX_BONES == ER_SKIN_BONES_MAX, "er_skin.h restates the two constants");

// The pieces below run with the mutex held, the device set, the stream idle and the host copy already edited.

// moved triangles: the refit of the built structure from the host copy's arrays, or -- sp -- from the listed triangles alone, or -- xf --
// from the device-resident rest copy of the listed objects
int edit_refit(ErScene* s, bool new_normals, bool new_tangents, const ErSparseList* sp, const XformList* xf, const char* who) {
    ErGpuBvhDevice& g = s->kept.accel;
    ErRefitBuffers b;
    b.nodes = (ErNode*)s->d_nodes.p; b.node_count = (uint32_t)(g.nodes_f4 / 4); b.depth2 = g.max_depth2;
    b.nodes8 = s->d_nodes8.p; b.node8_count = g.nodes8_count; b.depth8 = g.max_depth8;
    b.isect = (ErTriIsect*)(s->d_nodes8.p + g.n8_pieces); b.attr = (ErTriAttr*)s->d_attr.p; b.tri_count = s->tri_count;
    if (!sp && !xf) s->flush_poses();      // (the full form reads the host arrays; edit_replace has left nothing pending)
    ErRefitArrays a;
    a.vertices = s->vertices.data(); a.normals = s->normals.data(); a.write_normals = new_normals;
    a.tangents = new_tangents ? s->tangents.data() : nullptr;
    ErRefitResult r;
    std::string why;
    int frc;
    if (sp || xf) {
        ErSparseResult sr;
        if (sp) {
            frc = er_refit_sparse(s->refit_topo, b, *sp, s->stream, &sr, why);
        } else {
            frc = s->xform_dev.valid ? 0 : er_xform_table_build(s->xform_dev, s->objects, s->stream, why);      // once per er_objects_set / er_render_begin
            if (!xf->skin) {
                ErXformCall c;
                c.table = &s->xform_dev; c.entries = (uint32_t)xf->entries.size(); c.list = xf->entries.data(); c.moved = xf->moved;
                if (frc == 0) frc = er_refit_xform(s->refit_topo, b, c, s->stream, &sr, why);
            } else {
                if (frc == 0 && !s->skin_dev.valid) frc = er_skin_table_build(s->skin_dev, s->objects, s->skins, s->stream, &s->skin_influence_bytes, why);      // once per er_skin_set / er_render_begin
                ErSkinCall c;
                c.table = &s->xform_dev; c.skin = &s->skin_dev; c.entries = (uint32_t)xf->skin_entries.size(); c.list = xf->skin_entries.data();
                c.bones = (uint32_t)(xf->palette.size() / 12); c.palette = xf->palette.data(); c.moved = xf->moved;
                if (frc == 0) frc = er_refit_skin(s->refit_topo, b, c, s->stream, &sr, why);
            }
        }
        r = sr.refit;
        ErSparseInfo& I = sp ? s->sparse : xf->skin ? s->skin : s->xform;
        I.path = sr.path; I.why_full = sr.why_full;
        I.dirty_nodes2 = sr.dirty_nodes2; I.dirty_nodes8 = sr.dirty_nodes8;
        I.bytes_uploaded = sr.bytes_uploaded; I.refit_ms = r.refit_ms;
    } else {
        frc = er_refit_device(s->refit_topo, b, a, s->stream, &r, why);
    }
    if (frc != 0) return fail(frc == -2 ? ER_ERR_OOM : ER_ERR_HIP, std::string(who) + ": refit: " + why);
    if (s->tri_count) {
        for (int k = 0; k < 3; k++) { g.lo[k] = s->accel_lo[k] = r.lo[k]; g.hi[k] = s->accel_hi[k] = r.hi[k]; }
        g.lift_bound = s->accel.lift_bound = r.lift_bound;
    }
    s->accel.builder = 2u;
    s->accel.build_ms = s->upd.refit_ms = r.refit_ms;
    s->accel_version++;
    return ER_OK;
}

// er_accel_cost of the structure as it lies, measured unless this version of it has been
int accel_cost_locked(ErScene* s, const char* who, ErAccelCost* out) {
    if (s->cost_version != s->accel_version) {
        const ErGpuBvhDevice& g = s->kept.accel;
        ErCostSums c;
        std::string why;
        const int crc = er_cost_device(s->d_nodes8.p, g.nodes8_count, (const ErTriIsect*)(s->d_nodes8.p + g.n8_pieces), s->tri_count, s->stream, &c, nullptr, nullptr, why);
        if (crc != 0) return fail(crc == -2 ? ER_ERR_OOM : ER_ERR_HIP, std::string(who) + ": structure cost: " + why);
        s->cost_kept = ErAccelCost{c.node_area, c.leaf_area, c.tri_area, c.cost, c.ms, s->accel.builder};
        s->cost_version = s->accel_version;
        if (s->accel.builder != 2u) { s->baseline_known = true; s->baseline_cost = c.cost; }      // a BUILT tree: what a later refit is judged against
    }
    *out = s->cost_kept;
    return ER_OK;
}

// ER_REBUILD_ALWAYS / AUTO: the structure stage of er_render_begin again, on the host copy as it is now.  The scene's structure
// buffers and the refit's level lists go first; the builder is chosen as er_render_begin chooses it, and its depth checks apply.
int edit_rebuild(ErScene* s, BeginStaging& B, const char* who) {
    const auto t0 = std::chrono::steady_clock::now();
    s->refit_topo.release();
    s->d_nodes.release(); s->d_nodes8.release(); s->d_attr.release();
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    int rc;
    try {
        rc = begin_accel(s, B, ev.a, who);
    } catch (...) {
        s->begun = false;      // (the old structure is gone: an exception on its way to guarded() must not leave a scene that renders)
        throw;
    }
    if (rc != ER_OK) return rc;
    HIP_TRY(hipEventRecord(ev.b, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    float up_ms = 0;
    (void)hipEventElapsedTime(&up_ms, ev.a, ev.b);
    accel_publish(s, up_ms);
    s->rebuild.rebuilds++;
    s->rebuild.rebuild_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ER_OK;
}

// The geometry bit: the refit, or a fresh build, by the scene's policy (include/eleven_hip.h ER_REBUILD_*).  ER_REBUILD_NEVER is the
// refit and nothing else.
int edit_geometry(ErScene* s, BeginStaging& B, bool new_normals, bool new_tangents, const ErSparseList* sp, const XformList* xf, const char* who) {
    const uint32_t mode = s->policy.mode;
    if (mode == ER_REBUILD_NEVER) return edit_refit(s, new_normals, new_tangents, sp, xf, who);
    int rc;
    ErRebuildInfo& R = s->rebuild;
    R.cost_built = R.cost_refit = R.cost_after = 0.0;
    R.cost_ms = R.rebuild_ms = 0.0f;
    if (mode == ER_REBUILD_ALWAYS) {
        if ((rc = edit_rebuild(s, B, who)) != ER_OK) return rc;
        R.last_decision = 3u;
        return ER_OK;
    }
    ErAccelCost c;
    uint32_t decision = 4u;      // rebuilt: no baseline
    if (!s->baseline_known && s->accel.builder != 2u) {      // the built tree, still in place: measured before it is refitted
        if ((rc = accel_cost_locked(s, who, &c)) != ER_OK) return rc;
        R.cost_ms += c.ms;
    }
    if (s->baseline_known) {
        R.cost_built = s->baseline_cost;
        if ((rc = edit_refit(s, new_normals, new_tangents, sp, xf, who)) != ER_OK) return rc;
        if ((rc = accel_cost_locked(s, who, &c)) != ER_OK) return rc;
        R.cost_ms += c.ms;
        R.cost_refit = c.cost;
        decision = (R.cost_built != 0.0 && R.cost_refit > (double)s->policy.max_cost_ratio * R.cost_built) ? 2u : 1u;
    }
    if (decision != 1u) {
        if ((rc = edit_rebuild(s, B, who)) != ER_OK) return rc;
        if ((rc = accel_cost_locked(s, who, &c)) != ER_OK) return rc;      // (a built tree: this is the next baseline)
        R.cost_ms += c.ms;
        R.cost_after = c.cost;
    }
    R.last_decision = decision;
    return ER_OK;
}

// The materials bit: the list and its constants, and the triangles' material ids if they came with it
int edit_materials(ErScene* s, BeginStaging& B, bool new_ids) {
    int rc;
    if ((rc = upload_materials(s, B)) != ER_OK) return rc;
    if (!new_ids || !s->tri_count) return ER_OK;
    ScopedDevBuf<int32_t> d_ids;
    if ((rc = upload(d_ids, s->material_id.data(), s->material_id.size(), s->stream)) != ER_OK) return rc;
    er_launch_material_ids(s->d_nodes8.p + s->kept.accel.n8_pieces, s->d_attr.p, s->tri_count, d_ids.p, s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));      // (d_ids goes with this frame)
    return ER_OK;
}

// What the checks prepare of the lists that change size, so that nothing of the scene is replaced before the last check has passed
// and nothing can fail between the first replacement and the last (moves and swaps only).  The arrays whose size the scene fixes
// need no copy beside the scene's: edit_replace.
// er_render_topology's side of edit_check: `rest` is checked against the RESULT of the topology edit
struct TopoCtx {
    const ErTopoList* l = nullptr;
    const std::vector<uint32_t>* sorted = nullptr;      // the removed ids, ascending
    uint32_t new_count = 0;
};

// the material ids the edited scene will hold against a list of nmat: those given for the whole result, or the appended ones and --
// `kept_too`: the list may have shrunk -- the survivors'
int topo_check_material_ids(const ErScene* s, const int32_t* given, bool kept_too, const TopoCtx& tc, size_t nmat, const char* who) {
    int rc;
    if (given) return check_material_ids(given, tc.new_count, nmat, who);
    if (kept_too) {
        const std::vector<uint32_t>& gone = *tc.sorted;
        uint32_t from = 0;
        for (size_t k = 0; k <= gone.size(); k++) {      // the runs between removed ids
            const uint32_t to = k < gone.size() ? gone[k] : s->tri_count;
            if (to > from && (rc = check_material_ids(s->material_id.data() + from, to - from, nmat, who)) != ER_OK) return rc;
            from = to + 1;
        }
    }
    return check_material_ids(tc.l->material_id, tc.l->appends(), nmat, who);
}

struct EditWork {
    bool rebuild_pool = false;            // the pool is laid out again and filled on the device
    std::vector<ErMaterial> materials;
    std::vector<HostTex> textures;        // the new list; kept[i]: entry i is the scene's own texture i (moved in when the copy is replaced)
    std::vector<uint8_t> kept;
    HostTex hdri;
    std::vector<float> cdf;
    float radiance_sum = 0;
};

// The pool work of the texture and HDRI bits (and of a materials bit that changed a texture id); stage, stage_ms: ErEditInfo's
int edit_pool(ErScene* s, uint32_t what, bool rebuild_pool, BeginStaging& B, const char* who, uint32_t& stage, float& stage_ms) {
    int rc;
    stage = 0;
    stage_ms = 0;
    if (rebuild_pool) {
        TexPlan P;
        plan_of_scene(s, P);
        if ((rc = check_pool_floats(P.pool_floats, who)) != ER_OK) return rc;
        std::vector<ErTexSource> src(s->textures.size());
        for (size_t i = 0; i < src.size(); i++) src[i] = ErTexSource{s->textures[i].data.data(), s->textures[i].width, s->textures[i].height, s->textures[i].channels};
        const ErTexSource hsrc{s->hdri_tex.data.data(), s->hdri_tex.width, s->hdri_tex.height, s->hdri_tex.channels};
        float* pool = nullptr;
        std::string why;
        const int trc = er_texstage_build(P, src.data(), src.size(), s->materials.data(), s->materials.size(), hsrc, s->stream, &pool, &stage_ms, why);
        if (trc != 0) return fail(trc == -2 ? ER_ERR_OOM : ER_ERR_HIP, std::string(who) + ": texture stage: " + why);
        s->d_tex_pool.release();      // the new pool is swapped in
        s->d_tex_pool.p = pool;
        s->d_tex_pool.n = (size_t)P.pool_floats;
        s->tex_pool_cap = std::max<size_t>((size_t)P.pool_floats, 1);
        B.table = P.table;
        B.fused = P.fused;
        if ((rc = upload(s->d_textures, B.table.data(), B.table.size(), s->stream)) != ER_OK) return rc;
        if ((rc = upload(s->d_mat_fused, B.fused.data(), B.fused.size(), s->stream)) != ER_OK) return rc;
        s->tex_mode = P.mode;
        s->fused_any = P.fused_any;
        s->kept.hdri = P.hdri;
        stage = 2;
    } else if (what & ER_EDIT_HDRI) {
        // the HDRI's texels lie last: the tail is rewritten in place if the allocation holds the new one, else the pool grows and
        // its head moves over by a device-to-device copy
        const size_t head = s->kept.hdri.offset, need = head + s->hdri_tex.data.size();
        EventPair ev;
        HIP_TRY(hipEventCreate(&ev.a));
        HIP_TRY(hipEventCreate(&ev.b));
        HIP_TRY(hipEventRecord(ev.a, s->stream));
        if (need > s->tex_pool_cap) {
            DevBuf<float> bigger;
            if ((rc = upload(bigger, nullptr, need, s->stream)) != ER_OK) return rc;
            hipError_t ce = head ? hipMemcpyAsync(bigger.p, s->d_tex_pool.p, head * sizeof(float), hipMemcpyDeviceToDevice, s->stream) : hipSuccess;
            if (ce == hipSuccess) ce = hipStreamSynchronize(s->stream);
            if (ce != hipSuccess) {
                bigger.release();
                HIP_TRY(ce);
            }
            s->d_tex_pool.release();
            s->d_tex_pool = bigger;
            s->tex_pool_cap = std::max<size_t>(need, 1);
        }
        if (!s->hdri_tex.data.empty())
            HIP_TRY(hipMemcpyAsync(s->d_tex_pool.p + head, s->hdri_tex.data.data(), s->hdri_tex.data.size() * sizeof(float), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipEventRecord(ev.b, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        (void)hipEventElapsedTime(&stage_ms, ev.a, ev.b);
        s->d_tex_pool.n = need;
        s->kept.hdri = DevTex{s->hdri_tex.width, s->hdri_tex.height, s->hdri_tex.channels, s->hdri_tex.filter, (uint32_t)head};
        stage = 1;
    }
    if (what & ER_EDIT_HDRI) {
        if ((rc = upload(s->d_cdf, s->hdri_cdf.data(), s->hdri_cdf.size(), s->stream)) != ER_OK) return rc;
        if ((rc = upload_hdri_guide(s, B)) != ER_OK) return rc;      // (with the new HDRI's row and column tables behind it)
    }
    return ER_OK;
}

// ER_FLAG_MESH_LIGHTS: the emitter table again -- it holds areas of placed triangles and the emission of their materials and textures
int edit_emitters(ErScene* s, BeginStaging& B, const char* who) {
    s->d_light_tab.release(); s->light_emitters = 0; s->light_total = 0.0f;
    return begin_emitters(s, B, who);
}

// what a fresh scene's er_render_begin would find: no adaptive state, no samples, no open timing or profile window, the streaming
// schedule's host state and the wavefront schedule's pools as new -- then stages 6-8
int edit_restart(ErScene* s, BeginStaging& B) {
    s->ad_on = false;
    s->rendered = 0;
    s->timing_open = false;
    s->prof_used = 0;
    s->profile = ErProfile{};
    for (auto& set : s->unpacked) set.clear();
    s->st.release();
    s->st = StreamHost{};
    for (hipEvent_t e : s->pool_events) (void)hipEventDestroy(e);
    s->pool_events.clear();
    for (hipStream_t st : s->pool_streams) (void)hipStreamDestroy(st);
    s->pool_streams.clear();
    s->wf.clear();
    s->params.flags = s->kept.flags;      // (the schedule is chosen again, from the same flags on the same share)
    return begin_render_state(s, B, nullptr);
}

// The device work of an edit, the host copy replaced (section "The stages of an edit"): an absent bit skips its piece
int edit_device(ErScene* s, const ErSceneEdit* e, const ErSparseList* sp, const XformList* xf, bool rebuild_pool, const char* who, uint32_t& stage, float& stage_ms) {
    int rc;
    const uint32_t what = e->what;
    BeginStaging B;                     // outlives begin_render_state's hipStreamSynchronize
    const bool new_normals = sp ? sp->normals != nullptr : e->normals != nullptr, new_tangents = sp ? sp->tangents != nullptr : e->tangents != nullptr;
    if ((what & ER_EDIT_GEOMETRY) && (rc = edit_geometry(s, B, new_normals, new_tangents, sp, xf, who)) != ER_OK) return rc;
    if ((what & ER_EDIT_MATERIALS) && (rc = edit_materials(s, B, e->material_id != nullptr)) != ER_OK) return rc;
    if ((rc = edit_pool(s, what, rebuild_pool, B, who, stage, stage_ms)) != ER_OK) return rc;
    if ((what & (ER_EDIT_GEOMETRY | ER_EDIT_MATERIALS | ER_EDIT_TEXTURES)) && (rc = edit_emitters(s, B, who)) != ER_OK) return rc;
    return edit_restart(s, B);
}

// Every check of an edit, with nothing of the scene touched; W gets the new lists that the replacement will move in.  sp: the
// geometry bit's arrays are that list's (er_render_update_sparse), checked in O(count); xf: they are the listed objects' poses
// (er_render_transform), checked in O(objects listed), and xf gets the upload entries.
int edit_check(const ErScene* s, const ErSceneEdit* e, const ErSparseList* sp, XformList* xf, uint32_t known, const char* who, EditWork& W, const TopoCtx* tc = nullptr) {
    const std::string pre = std::string(who) + ": ";
    const uint32_t what = e->what;
    int rc;
    if ((what == 0 && !tc) || (what & ~known)) return fail(ER_ERR_INVALID_ARG, pre + "`what` names nothing, or something unknown");      // (a topology edit may come alone)
    const size_t n = s->tri_count, n9 = n * 9;
    if ((what & ER_EDIT_GEOMETRY) && sp) {
        std::string why;
        if (!er_sparse_check(s->tri_count, *sp, why)) return fail(ER_ERR_INVALID_ARG, pre + why);
    } else if ((what & ER_EDIT_GEOMETRY) && xf && xf->skin) {
        std::string why;
        const int src = er_skin_pose_check(s->objects, s->skins, xf->count, xf->poses, xf->skin_entries, xf->palette, xf->moved, why);
        if (src != 0) return fail(src == 2 ? ER_ERR_STATE : ER_ERR_INVALID_ARG, pre + why);
    } else if ((what & ER_EDIT_GEOMETRY) && xf) {
        std::string why;
        if (!er_xform_check(s->objects, xf->count, xf->x, xf->entries, xf->moved, why)) return fail(ER_ERR_INVALID_ARG, pre + why);
    } else if (what & ER_EDIT_GEOMETRY) {
        if (!e->vertices) return fail(ER_ERR_INVALID_ARG, pre + "the geometry bit without vertices");
        for (size_t i = 0; i < n9; i++)
            if (!std::isfinite(e->vertices[i])) return fail(ER_ERR_INVALID_ARG, pre + "vertex " + std::to_string(i / 3) + " is not finite");
    }
    const size_t old_ntex = s->textures.size();
    size_t ntex = old_ntex;
    if (what & ER_EDIT_TEXTURES) {
        ntex = e->texture_count;
        if (ntex < old_ntex) return fail(ER_ERR_INVALID_ARG, pre + "texture_count is below the scene's (textures are replaced or appended, never removed)");
        if (ntex && !e->textures) return fail(ER_ERR_INVALID_ARG, pre + "ER_EDIT_TEXTURES without the texture list");
        for (size_t i = 0; i < ntex; i++) {
            const ErTexture& t = e->textures[i];
            if (!t.data) {
                if (i >= old_ntex) return fail(ER_ERR_INVALID_ARG, pre + "texture " + std::to_string(i) + " has no data and the scene has no such texture to keep");
                continue;
            }
            if ((rc = check_tex(t, "scene texture")) != ER_OK) return rc;
        }
    }
    const ErMaterial* mats = s->materials.data();
    size_t nmat = s->materials.size();
    bool ids_differ = false;
    if (what & ER_EDIT_MATERIALS) {
        if (e->material_count == 0 || !e->materials) return fail(ER_ERR_INVALID_ARG, pre + "ER_EDIT_MATERIALS needs at least one material");
        mats = e->materials;
        nmat = e->material_count;
        if ((rc = check_texture_ids(mats, nmat, ntex, who)) != ER_OK) return rc;
        if (tc) rc = topo_check_material_ids(s, e->material_id, true, *tc, nmat, who);
        else rc = check_material_ids(e->material_id ? e->material_id : s->material_id.data(), n, nmat, who);
        if (rc != ER_OK) return rc;
        ids_differ = nmat != s->materials.size();
        for (size_t m = 0; m < nmat && !ids_differ; m++) {
            int32_t a[7], b[7];
            texture_ids(mats[m], a);
            texture_ids(s->materials[m], b);
            ids_differ = memcmp(a, b, sizeof(a)) != 0;
        }
    }
    if (tc && !(what & ER_EDIT_MATERIALS) && (rc = topo_check_material_ids(s, nullptr, false, *tc, nmat, who)) != ER_OK) return rc;
    if ((what & ER_EDIT_HDRI) && (rc = check_tex(e->hdri.texture, "hdri")) != ER_OK) return rc;
    W.rebuild_pool = (what & ER_EDIT_TEXTURES) != 0 || ids_differ;
    {   // the pool the edited scene needs, from the plan
        const TexDecl hd = (what & ER_EDIT_HDRI) ? TexDecl{e->hdri.texture.width, e->hdri.texture.height, e->hdri.texture.channels, e->hdri.texture.filter}
                                                 : TexDecl{s->hdri_tex.width, s->hdri_tex.height, s->hdri_tex.channels, s->hdri_tex.filter};
        uint64_t pool_floats = 0;
        if (W.rebuild_pool) {
            std::vector<TexDecl> decl(ntex);
            for (size_t i = 0; i < ntex; i++) {
                const bool keep = !(what & ER_EDIT_TEXTURES) || !e->textures[i].data;
                decl[i] = keep ? TexDecl{s->textures[i].width, s->textures[i].height, s->textures[i].channels, s->textures[i].filter}
                               : TexDecl{e->textures[i].width, e->textures[i].height, e->textures[i].channels, e->textures[i].filter};
            }
            TexPlan P;
            er_texture_plan(decl.data(), ntex, mats, nmat, hd, P);
            pool_floats = P.pool_floats;
        } else if (what & ER_EDIT_HDRI) {
            pool_floats = (uint64_t)s->kept.hdri.offset + (uint64_t)hd.width * (uint64_t)hd.height * (uint64_t)hd.channels;
        }
        if ((rc = check_pool_floats(pool_floats, who)) != ER_OK) return rc;
    }
    // the new lists, beside the scene's (an allocation that fails here leaves the scene as it was)
    if (what & ER_EDIT_MATERIALS) W.materials.assign(e->materials, e->materials + e->material_count);
    if (what & ER_EDIT_TEXTURES) {
        W.textures.resize(ntex);
        W.kept.assign(ntex, 0);
        for (size_t i = 0; i < ntex; i++) {
            if (!e->textures[i].data) { W.kept[i] = 1; continue; }
            if ((rc = copy_tex(e->textures[i], W.textures[i], "scene texture")) != ER_OK) return rc;
        }
    }
    if (what & ER_EDIT_HDRI) {
        if ((rc = copy_tex(e->hdri.texture, W.hdri, "hdri")) != ER_OK) return rc;
        if (e->hdri.cdf) {
            W.cdf.assign(e->hdri.cdf, e->hdri.cdf + (size_t)W.hdri.width * W.hdri.height + 1);
            W.radiance_sum = e->hdri.radiance_sum;
        } else {
            host_generate_cdf(W.hdri, W.cdf, W.radiance_sum);
        }
    }
    return ER_OK;
}

// The host copy replaced, after the last check.  Nothing here can throw or fail: vertices, normals and tangents hold 9 x tri_count
// floats and material_id tri_count entries (er_scene_create; er_render_topology resizes all of them together, before it comes
// here), so std::copy into them writes into storage that is there and never allocates; the lists that change size were made in W and are swapped in.
// The poses that er_render_transform left pending (er_xform.h: no allocation, no failure either) are applied before a list patches the
// arrays or a full update keeps some of them, and forgotten where all three arrays are replaced whole; a transform only marks.
void edit_replace(ErScene* s, const ErSceneEdit* e, const ErSparseList* sp, const XformList* xf, EditWork& W) noexcept {
    const uint32_t what = e->what;
    const size_t n = s->tri_count, n9 = n * 9;
    if (what & ER_EDIT_CAMERA) s->camera = e->camera;
    if ((what & ER_EDIT_GEOMETRY) && sp) {
        s->flush_poses();
        er_sparse_patch(*sp, s->vertices.data(), s->normals.data(), s->tangents.data());
    } else if ((what & ER_EDIT_GEOMETRY) && xf && xf->skin) {
        er_skin_mark(s->objects, s->skins, xf->skin_entries.data(), (uint32_t)xf->skin_entries.size(), xf->palette.data());
    } else if ((what & ER_EDIT_GEOMETRY) && xf) {
        er_objects_mark(s->objects, xf->entries.data(), (uint32_t)xf->entries.size());
    } else if (what & ER_EDIT_GEOMETRY) {
        if (e->normals && e->tangents) s->objects.forget_pending();
        else s->flush_poses();
        std::copy(e->vertices, e->vertices + n9, s->vertices.begin());
        if (e->normals) std::copy(e->normals, e->normals + n9, s->normals.begin());
        if (e->tangents) std::copy(e->tangents, e->tangents + n9, s->tangents.begin());
    }
    if (what & ER_EDIT_MATERIALS) {
        s->materials.swap(W.materials);
        if (e->material_id) std::copy(e->material_id, e->material_id + n, s->material_id.begin());
    }
    if (what & ER_EDIT_TEXTURES) {
        for (size_t i = 0; i < W.textures.size(); i++)
            if (W.kept[i]) std::swap(W.textures[i], s->textures[i]);
        s->textures.swap(W.textures);
    }
    if (what & ER_EDIT_HDRI) {
        std::swap(s->hdri_tex, W.hdri);
        s->hdri_cdf.swap(W.cdf);
        s->hdri_radiance_sum = W.radiance_sum;
    }
}

// er_render_update (known = its two bits), er_render_edit and er_render_update_sparse (sp: its list), with the mutex held and the
// scene begun
int edit_locked(ErScene* s, const ErSceneEdit* e, const ErSparseList* sp, XformList* xf, uint32_t known, const char* who, std::chrono::steady_clock::time_point t0) {
    int rc;
    EditWork W;
    if ((rc = edit_check(s, e, sp, xf, known, who, W)) != ER_OK) return rc;
    // pending asynchronous work first (the pool streams join the scene's stream at the end of every call)
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    // the host copy, before any device work: whatever happens below, a later er_render_begin builds the edited scene
    edit_replace(s, e, sp, xf, W);
    // a deformation has no back matrix: a palette pose drops the history, and so does the matrix pose that takes an object out of one
    const bool deformed = xf && (e->what & ER_EDIT_GEOMETRY) && (xf->skin || er_skin_mark_matrix(s->skins, xf->entries.data(), (uint32_t)xf->entries.size()));
    if ((e->what & ER_EDIT_GEOMETRY) || ((e->what & ER_EDIT_MATERIALS) && e->material_id)) s->store.release();      // er_render_topology's geometry store does not follow other edits
    s->feat.valid = false;      // the feature planes show the scene before the edit (er_render_features makes them again)
    for (auto& set : s->unpacked_feat) set.clear();
    s->ids_invalidate();        // (and so do the id planes: er_render_ids)
    if (((e->what & ER_EDIT_GEOMETRY) && (!xf || deformed)) || (e->what & LOOK_BITS)) s->history_invalidate();      // a camera or a pose keeps the history (er_history.hip)
    s->variance_reset();        // the render starts over: so do the variance moments (er_variance.hip)
    uint32_t stage = 0;
    float stage_ms = 0;
    const bool sparse_geometry = sp && (e->what & ER_EDIT_GEOMETRY);
    if (sparse_geometry) {      // (a call that ends in a rebuild without a refit leaves these)
        const uint32_t calls = s->sparse.calls;
        s->sparse = ErSparseInfo{};
        s->sparse.calls = calls;
    }
    const bool xform_geometry = xf && (e->what & ER_EDIT_GEOMETRY);
    if (xform_geometry) {
        ErSparseInfo& I = xf->skin ? s->skin : s->xform;
        const uint32_t calls = I.calls;
        I = ErSparseInfo{};
        I.calls = calls;
        if (xf->skin) s->skin_influence_bytes = 0;
    }
    if ((rc = edit_device(s, e, sp, xf, W.rebuild_pool, who, stage, stage_ms)) != ER_OK) {
        s->begun = false;      // (er_render_begin releases what is left and rebuilds from the edited host copy)
        return rc;
    }
    // The books (include/eleven_hip.h, at ER_EDIT_*): updates and refits count the calls of either entry point.  A call that named only
    // CAMERA / GEOMETRY, through either, is an update: it leaves its wall time in upd.update_ms and ErEditInfo alone.  A call that named
    // one of the other bits is an edit: it writes ErEditInfo and leaves upd.update_ms alone.
    s->upd.updates++;
    if (sparse_geometry) {
        s->sparse.calls++;
        s->sparse.moved = sp->count;
        if (s->accel.builder != 2u) s->sparse.path = 3u;      // the policy ended the call in a build: the refit's figures, if one ran, stay
    }
    if (xform_geometry && !xf->skin) {
        s->xform.calls++;
        s->xform.moved = xf->moved;
        s->xform_objects = xf->count;
        if (s->accel.builder != 2u) s->xform.path = 3u;
    }
    if (xform_geometry && xf->skin) {
        s->skin.calls++;
        s->skin.moved = xf->moved;
        s->skin_objects = xf->count;
        s->skin_bones = (uint32_t)(xf->palette.size() / 12);
        if (s->accel.builder != 2u) s->skin.path = 3u;
    }
    if ((e->what & ER_EDIT_GEOMETRY) && s->accel.builder == 2u) s->upd.refits++;      // (under a rebuild policy the call may have ended in a build)
    const float wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (e->what & LOOK_BITS) {
        s->edit.edits++;
        s->edit.texture_stage = stage;
        s->edit.texture_stage_ms = stage_ms;
        s->edit.pool_floats = s->d_tex_pool.n;
        s->edit.edit_ms = wall_ms;
    } else {
        s->upd.update_ms = wall_ms;
    }
    return ER_OK;
}

}  // namespace

static int er_render_update_impl(ErScene* s, const ErSceneUpdate* u) {
    if (!s || !u) return fail(ER_ERR_INVALID_ARG, "er_render_update: NULL argument");
    const auto t0 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_render_update: er_render_begin has not succeeded");
    ErSceneEdit e{};
    e.what = u->what; e.camera = u->camera; e.vertices = u->vertices; e.normals = u->normals; e.tangents = u->tangents;
    return edit_locked(s, &e, nullptr, nullptr, ER_UPDATE_CAMERA | ER_UPDATE_GEOMETRY, "er_render_update", t0);
}

static int er_render_update_sparse_impl(ErScene* s, const ErSparseUpdate* u) {
    if (!s || !u) return fail(ER_ERR_INVALID_ARG, "er_render_update_sparse: NULL argument");
    const auto t0 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_render_update_sparse: er_render_begin has not succeeded");
    ErSceneEdit e{};      // (its arrays stay NULL: the list stands for them)
    e.what = u->what; e.camera = u->camera;
    ErSparseList l;
    l.count = u->count; l.tri_ids = u->tri_ids; l.vertices = u->vertices; l.normals = u->normals; l.tangents = u->tangents;
    return edit_locked(s, &e, &l, nullptr, ER_UPDATE_CAMERA | ER_UPDATE_GEOMETRY, "er_render_update_sparse", t0);
}

static int er_sparse_info_impl(ErScene* s, ErSparseInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_sparse_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    *out = s->sparse;
    return ER_OK;
}

static int er_objects_set_impl(ErScene* s, uint32_t object_count, const uint32_t* first, const uint32_t* tri_ids) {
    if (!s || (object_count && !first)) return fail(ER_ERR_INVALID_ARG, "er_objects_set: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    std::string why;
    if (!er_objects_check(s->tri_count, object_count, first, tri_ids, why)) return fail(ER_ERR_INVALID_ARG, "er_objects_set: " + why);
    if (object_count) host_reserve((uint64_t)first[object_count] * (27 + 1) * 4 + (uint64_t)object_count * 20 * 4);
    s->flush_poses();      // the rest pose is the CURRENT pose
    er_objects_take(s->objects, object_count, first, tri_ids, s->vertices.data(), s->normals.data(), s->tangents.data());
    er_skin_drop(s->skins);      // (skins do not survive a new table)
    if (s->xform_dev.valid || s->xform_dev.d_rest || s->skin_dev.valid || s->skin_dev.d_w) {      // the device forms were the old table's: the next transform or skin builds the new ones
        (void)hipSetDevice(s->device);
        if (s->stream) (void)hipStreamSynchronize(s->stream);
        s->xform_dev.release();
        s->skin_dev.release();
    }
    s->ids_invalidate();      // the OBJECT plane and the tri -> object map were the old table's (er_ids.hip)
    s->history_invalidate();      // (and the captured poses)
    s->id_map_valid = false;
    return ER_OK;
}

static int er_render_transform_impl(ErScene* s, const ErTransformUpdate* u) {
    if (!s || !u) return fail(ER_ERR_INVALID_ARG, "er_render_transform: NULL argument");
    const auto t0 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_render_transform: er_render_begin has not succeeded");
    if ((u->what & ER_UPDATE_GEOMETRY) && s->objects.objects() == 0) return fail(ER_ERR_STATE, "er_render_transform: the geometry bit without an object table (er_objects_set)");
    ErSceneEdit e{};      // (its arrays stay NULL: the listed objects stand for them)
    e.what = u->what; e.camera = u->camera;
    XformList l;
    l.count = u->count; l.x = u->transforms;
    return edit_locked(s, &e, nullptr, &l, ER_UPDATE_CAMERA | ER_UPDATE_GEOMETRY, "er_render_transform", t0);
}

static int er_transform_info_impl(ErScene* s, ErTransformInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_transform_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    const ErSparseInfo& x = s->xform;
    *out = ErTransformInfo{x.calls, s->xform_objects, x.moved, x.path, x.why_full, x.dirty_nodes2, x.dirty_nodes8, 0u, x.bytes_uploaded, x.refit_ms};
    return ER_OK;
}

static int er_skin_set_impl(ErScene* s, const ErSkin* k) {
    if (!s || !k || (k->bone_count && (!k->bones || !k->weights))) return fail(ER_ERR_INVALID_ARG, "er_skin_set: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (s->objects.objects() == 0) return fail(ER_ERR_STATE, "er_skin_set: no object table (er_objects_set)");
    std::string why;
    if (!er_skin_check(s->objects, *k, why)) return fail(ER_ERR_INVALID_ARG, "er_skin_set: " + why);
    if (k->bone_count) host_reserve((uint64_t)s->objects.size_of(k->object) * 72 + (uint64_t)k->bone_count * 48 + (uint64_t)s->objects.objects() * 64);
    s->flush_poses();      // (a palette pose of this object that is still pending is applied with the skin it was given for)
    er_skin_take(s->skins, s->objects, *k);
    if (s->skin_dev.valid || s->skin_dev.d_w) {      // the device form was of the old skins: the next er_render_skin builds the new one
        (void)hipSetDevice(s->device);
        if (s->stream) (void)hipStreamSynchronize(s->stream);
        s->skin_dev.release();
    }
    return ER_OK;
}

static int er_render_skin_impl(ErScene* s, const ErSkinUpdate* u) {
    if (!s || !u) return fail(ER_ERR_INVALID_ARG, "er_render_skin: NULL argument");
    const auto t0 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_render_skin: er_render_begin has not succeeded");
    if ((u->what & ER_UPDATE_GEOMETRY) && s->objects.objects() == 0) return fail(ER_ERR_STATE, "er_render_skin: the geometry bit without an object table (er_objects_set, er_skin_set)");
    ErSceneEdit e{};      // (its arrays stay NULL: the listed objects stand for them)
    e.what = u->what; e.camera = u->camera;
    XformList l;
    l.count = u->count; l.poses = u->poses; l.skin = true;
    return edit_locked(s, &e, nullptr, &l, ER_UPDATE_CAMERA | ER_UPDATE_GEOMETRY, "er_render_skin", t0);
}

static int er_skin_info_impl(ErScene* s, ErSkinInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_skin_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    const ErSparseInfo& x = s->skin;
    *out = ErSkinInfo{x.calls, s->skins.skinned, s->skin_objects, s->skin_bones, x.moved, x.path, x.why_full, x.dirty_nodes2, x.dirty_nodes8, x.refit_ms, x.bytes_uploaded,
                      s->skin_influence_bytes};
    return ER_OK;
}

static int er_render_edit_impl(ErScene* s, const ErSceneEdit* e) {
    if (!s || !e) return fail(ER_ERR_INVALID_ARG, "er_render_edit: NULL argument");
    const auto t0 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_render_edit: er_render_begin has not succeeded");
    return edit_locked(s, e, nullptr, nullptr, ER_EDIT_CAMERA | ER_EDIT_GEOMETRY | LOOK_BITS, "er_render_edit", t0);
}

static int er_accel_cost_impl(ErScene* s, ErAccelCost* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_accel_cost: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_accel_cost: er_render_begin has not succeeded");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));      // pending asynchronous work first
    return accel_cost_locked(s, "er_accel_cost", out);
}

static int er_update_policy_set_impl(ErScene* s, const ErUpdatePolicy* p) {
    if (!s || !p) return fail(ER_ERR_INVALID_ARG, "er_update_policy_set: NULL argument");
    if (p->mode > ER_REBUILD_AUTO) return fail(ER_ERR_INVALID_ARG, "er_update_policy_set: unknown mode");
    if (p->mode == ER_REBUILD_AUTO && !(std::isfinite(p->max_cost_ratio) && p->max_cost_ratio >= 1.0f))
        return fail(ER_ERR_INVALID_ARG, "er_update_policy_set: ER_REBUILD_AUTO needs a finite max_cost_ratio >= 1");
    std::lock_guard<std::mutex> lk(s->mtx);
    s->policy = *p;
    return ER_OK;
}

static int er_update_info_impl(ErScene* s, ErUpdateInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_update_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    *out = s->upd;
    return ER_OK;
}

static int er_edit_info_impl(ErScene* s, ErEditInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_edit_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    *out = s->edit;
    return ER_OK;
}

static int er_rebuild_info_impl(ErScene* s, ErRebuildInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_rebuild_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    *out = s->rebuild;
    out->mode = s->policy.mode;
    out->max_cost_ratio = s->policy.max_cost_ratio;
    return ER_OK;
}


namespace {

// ---- er_render_topology ----

// The device work of a topology edit, the host copy replaced: the geometry store brought to the new numbering (compacted where it was
// resident, else filled), the structure stage of er_render_begin on it -- the builder chosen as er_render_begin chooses it --, then the
// stages of `rest` and the restart, as edit_device.  old_count: the triangle count before the edit (what a resident store holds).
int topo_device(ErScene* s, const ErSceneEdit* rest, const ErTopoList& l, const std::vector<uint32_t>& sorted, uint32_t old_count, bool rebuild_pool, const char* who) {
    int rc;
    ErTopologyInfo& I = s->topo;
    BeginStaging B;
    ErGpuSceneArrays dev_arrays{};
    const ErGpuSceneArrays* dev = nullptr;
    if (accel_device_first(s)) {
        std::string why;
        int src;
        if (s->store.valid && s->store.count == old_count) {
            const ErGpuSceneArrays tail{l.vertices, l.normals, l.tangents, l.uvs, l.tangent_sign, l.material_id};
            src = er_store_edit(s->store, l.removes(), sorted.data(), l.appends(), tail, s->stream, &I.bytes_uploaded, &I.store_ms, why);
            I.path = 1u;
        } else {
            const ErGpuSceneArrays host{s->vertices.data(), s->normals.data(), s->tangents.data(), s->uvs.data(), s->tangent_sign.data(), s->material_id.data()};
            src = er_store_fill(s->store, host, s->tri_count, s->stream, &I.bytes_uploaded, why);
            I.path = 2u;
        }
        if (src == -1) return fail(ER_ERR_HIP, std::string(who) + ": geometry store: " + why);
        if (src != 0) {      // out of device memory: no store, the structure stage runs as it is
            (void)hipGetLastError();
            I.path = 0u; I.bytes_uploaded = 0; I.store_ms = 0;
        } else {
            dev_arrays = s->store.arrays();
            dev = &dev_arrays;
        }
    } else {
        s->store.release();
    }
    s->refit_topo.release();      // (the sparse refit's kept boxes were the old tree's)
    s->d_nodes.release(); s->d_nodes8.release(); s->d_attr.release();
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    try {
        rc = begin_accel(s, B, ev.a, who, dev);
    } catch (...) {
        s->begun = false;      // (as edit_rebuild: the old structure is gone)
        throw;
    }
    if (rc != ER_OK) return rc;
    HIP_TRY(hipEventRecord(ev.b, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    float up_ms = 0;
    (void)hipEventElapsedTime(&up_ms, ev.a, ev.b);
    accel_publish(s, up_ms);
    if (s->accel.builder != 1u) {      // the device builder declined or failed and the host built: no store was used
        s->store.release();
        I.path = 0u; I.bytes_uploaded = 0; I.store_ms = 0;
    }
    I.build_ms = s->accel.build_ms;
    const uint32_t what = rest->what;
    if ((what & ER_EDIT_MATERIALS) && (rc = edit_materials(s, B, false)) != ER_OK) return rc;      // (the records have their material ids from the build)
    if ((rc = edit_pool(s, what, rebuild_pool, B, who, I.texture_stage, I.texture_stage_ms)) != ER_OK) return rc;
    if ((rc = edit_emitters(s, B, who)) != ER_OK) return rc;
    return edit_restart(s, B);
}

}  // namespace

static int er_render_topology_impl(ErScene* s, const ErTopologyEdit* t) {
    const char* who = "er_render_topology";
    if (!s || !t) return fail(ER_ERR_INVALID_ARG, "er_render_topology: NULL argument");
    const auto t0 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_render_topology: er_render_begin has not succeeded");
    int rc;
    ErTopoList l;
    l.what = t->what; l.remove_count = t->remove_count; l.remove_ids = t->remove_ids; l.append_count = t->append_count;
    l.vertices = t->vertices; l.normals = t->normals; l.tangents = t->tangents; l.uvs = t->uvs; l.tangent_sign = t->tangent_sign;
    l.material_id = t->material_id; l.append_as_object = t->append_as_object;
    // every check, with nothing of the scene touched
    std::vector<uint32_t> sorted;
    uint32_t new_count = 0;
    std::string why;
    if (!er_topo_check(s->tri_count, l, sorted, new_count, why)) return fail(ER_ERR_INVALID_ARG, std::string(who) + ": " + why);
    if (new_count >= (1u << 28)) return fail(ER_ERR_INVALID_ARG, std::string(who) + ": too many triangles (er_scene_create refuses the result)");
    if (t->rest.what & ER_EDIT_GEOMETRY) return fail(ER_ERR_INVALID_ARG, std::string(who) + ": ER_EDIT_GEOMETRY in rest.what (moved vertices are er_render_update's)");
    TopoCtx tc;
    tc.l = &l; tc.sorted = &sorted; tc.new_count = new_count;
    EditWork W;
    if ((rc = edit_check(s, &t->rest, nullptr, nullptr, ER_EDIT_CAMERA | LOOK_BITS, who, W, &tc)) != ER_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));      // pending asynchronous work first
    {   // the store's kernels are probed here, not by er_render_begin (er_kernels.h says why a probe at all): a render that never edits
        // its topology loads nothing for it
        const char* which = nullptr;
        const hipError_t pe = er_probe_topology(&which);
        if (pe != hipSuccess) return fail(ER_ERR_HIP, std::string(who) + ": libeleven_hip.so has no usable gfx950 code object for " + (which ? which : "?") + " (" + hipGetErrorString(pe) + ")");
    }
    // what can still fail for want of host memory, beside the scene: room for the appended rows, and the renumbered object table
    const uint32_t old_count = s->tri_count;
    if (new_count > old_count) host_reserve((uint64_t)(new_count - old_count) * (9 * 3 + 6 + 1 + 1) * 4);
    const ErTopoArrays A{&s->vertices, &s->normals, &s->tangents, &s->uvs, &s->tangent_sign, &s->material_id};
    er_topo_reserve(A, new_count);
    s->flush_poses();      // (the edited description is the current one with pending poses flushed; the arrays' meaning does not change)
    ErObjectTable table;
    er_topo_remap_objects(s->objects, old_count, sorted, l, table);
    // the host copy, before any device work; nothing below can fail until the device is touched
    er_topo_apply(A, old_count, sorted, l);
    s->tri_count = new_count;
    std::swap(s->objects, table);
    edit_replace(s, &t->rest, nullptr, nullptr, W);      // (rest.material_id has new_count entries: tri_count is the new one)
    s->feat.valid = false;
    for (auto& set : s->unpacked_feat) set.clear();
    s->ids_invalidate();
    s->history_invalidate();
    s->variance_reset();
    s->d_id_map.release();      // the tri -> object map and the table's device form were of the old numbering: the lazy paths make them again
    s->id_map_valid = false;
    s->xform_dev.release();
    er_skin_drop(s->skins);      // (skins do not survive a renumbering; their pending poses were flushed above)
    s->skin_dev.release();
    if ((t->rest.what & ER_EDIT_MATERIALS) && t->rest.material_id) s->store.release();      // (the store's material ids would be stale: filled again below)
    const uint32_t calls = s->topo.calls;
    s->topo = ErTopologyInfo{};
    s->topo.calls = calls;
    if ((rc = topo_device(s, &t->rest, l, sorted, old_count, W.rebuild_pool, who)) != ER_OK) {
        s->begun = false;      // (er_render_begin releases what is left and builds from the edited host copy)
        s->store.release();
        return rc;
    }
    s->topo.calls++;
    s->topo.removed = l.removes();
    s->topo.appended = l.appends();
    s->topo.tri_count = new_count;
    s->topo.edit_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ER_OK;
}

static int er_topology_info_impl(ErScene* s, ErTopologyInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_topology_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    *out = s->topo;
    return ER_OK;
}

// ---- the exported entry points: every body above runs inside guarded() (no exception crosses the C ABI) ----
extern "C" {
int er_render_update(ErScene* s, const ErSceneUpdate* u) { return guarded("er_render_update", [&]() -> int { return er_render_update_impl(s, u); }); }
int er_update_info(ErScene* s, ErUpdateInfo* out) { return guarded("er_update_info", [&]() -> int { return er_update_info_impl(s, out); }); }
int er_render_update_sparse(ErScene* s, const ErSparseUpdate* u) { return guarded("er_render_update_sparse", [&]() -> int { return er_render_update_sparse_impl(s, u); }); }
int er_sparse_info(ErScene* s, ErSparseInfo* out) { return guarded("er_sparse_info", [&]() -> int { return er_sparse_info_impl(s, out); }); }
int er_objects_set(ErScene* s, uint32_t object_count, const uint32_t* first, const uint32_t* tri_ids) { return guarded("er_objects_set", [&]() -> int { return er_objects_set_impl(s, object_count, first, tri_ids); }); }
int er_render_transform(ErScene* s, const ErTransformUpdate* u) { return guarded("er_render_transform", [&]() -> int { return er_render_transform_impl(s, u); }); }
int er_transform_info(ErScene* s, ErTransformInfo* out) { return guarded("er_transform_info", [&]() -> int { return er_transform_info_impl(s, out); }); }
int er_skin_set(ErScene* s, const ErSkin* k) { return guarded("er_skin_set", [&]() -> int { return er_skin_set_impl(s, k); }); }
int er_render_skin(ErScene* s, const ErSkinUpdate* u) { return guarded("er_render_skin", [&]() -> int { return er_render_skin_impl(s, u); }); }
int er_skin_info(ErScene* s, ErSkinInfo* out) { return guarded("er_skin_info", [&]() -> int { return er_skin_info_impl(s, out); }); }
int er_render_edit(ErScene* s, const ErSceneEdit* e) { return guarded("er_render_edit", [&]() -> int { return er_render_edit_impl(s, e); }); }
int er_edit_info(ErScene* s, ErEditInfo* out) { return guarded("er_edit_info", [&]() -> int { return er_edit_info_impl(s, out); }); }
int er_accel_cost(ErScene* s, ErAccelCost* out) { return guarded("er_accel_cost", [&]() -> int { return er_accel_cost_impl(s, out); }); }
int er_update_policy_set(ErScene* s, const ErUpdatePolicy* p) { return guarded("er_update_policy_set", [&]() -> int { return er_update_policy_set_impl(s, p); }); }
int er_rebuild_info(ErScene* s, ErRebuildInfo* out) { return guarded("er_rebuild_info", [&]() -> int { return er_rebuild_info_impl(s, out); }); }
int er_render_topology(ErScene* s, const ErTopologyEdit* t) { return guarded("er_render_topology", [&]() -> int { return er_render_topology_impl(s, t); }); }
int er_topology_info(ErScene* s, ErTopologyInfo* out) { return guarded("er_topology_info", [&]() -> int { return er_topology_info_impl(s, out); }); }
}  // extern "C"
