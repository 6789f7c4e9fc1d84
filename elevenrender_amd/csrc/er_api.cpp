// er_api.cpp -- implementation of the C ABI declared in include/eleven_hip.h.
// Host side of the device boundary: the MI355X replacement for dev_Scene's constructor,
// copy_scene, renderSetup, kernel_render_enqueue and RenderingManager::get_pass
// (reference src/kernel.cpp:244-266,651-706; src/SYCLCopy.cpp:3-104; src/Managers.cpp:287-302).
// There is NO CPU fallback: without a usable HIP device every compute entry point fails.
#include <algorithm>
#include <chrono>

#include "er_api_stages.h"
#include <thread>
#include <system_error>

using namespace erh;

int er_abi_version(void) { return ER_ABI_VERSION; }
const char* er_last_error(void) { return g_err.c_str(); }

int er_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int er_device_info_impl(int index, ErDeviceInfo* out) {
    if (!out) return fail(ER_ERR_INVALID_ARG, "er_device_info: out is NULL");
    int n = er_device_count();
    if (index < 0 || index >= n) return fail(ER_ERR_NO_DEVICE, "er_device_info: no such HIP device");
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, index));
    memset(out, 0, sizeof(*out));
    snprintf(out->name, sizeof(out->name), "%s", p.name);
    snprintf(out->platform, sizeof(out->platform), "AMD HIP");
    snprintf(out->arch, sizeof(out->arch), "%s", p.gcnArchName);
    out->memory_bytes = p.totalGlobalMem;
    out->compute_units = (uint32_t)p.multiProcessorCount;
    out->compatible = strncmp(p.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
    return ER_OK;
}

static int er_device_find_impl(const char* selector) {
    if (!selector) return fail(ER_ERR_INVALID_ARG, "er_device_find: selector is NULL");
    int n = er_device_count();
    for (int i = 0; i < n; i++) {
        ErDeviceInfo info;
        if (er_device_info(i, &info) != ER_OK) continue;
        std::string s = std::string(info.name) + "|" + info.platform;   // NameSelector, reference src/Managers.cpp:201
        if (s == selector) return i;
    }
    return fail(ER_ERR_NO_DEVICE, std::string("er_device_find: no device matches '") + selector + "'");
}

static int er_scene_create_impl(const ErSceneDesc* d, ErScene** out) {
    if (!d || !out) return fail(ER_ERR_INVALID_ARG, "er_scene_create: NULL argument");
    *out = nullptr;
    if (d->x_res == 0 || d->y_res == 0) return fail(ER_ERR_INVALID_ARG, "er_scene_create: zero resolution");
    if ((uint64_t)d->x_res * d->y_res > 0x7fffffffull) return fail(ER_ERR_INVALID_ARG, "er_scene_create: resolution too large");
    if (d->tri_count >= (1u << 28)) return fail(ER_ERR_INVALID_ARG, "er_scene_create: too many triangles");
    if (d->tri_count && (!d->vertices || !d->normals || !d->tangents || !d->uvs || !d->tangent_sign || !d->material_id))
        return fail(ER_ERR_INVALID_ARG, "er_scene_create: triangle arrays missing");
    if (d->material_count == 0 || !d->materials) return fail(ER_ERR_INVALID_ARG, "er_scene_create: at least one material is required");
    size_t n = d->tri_count;
    {   // what the host copy of the description will take (texel payloads + 31 floats per triangle + the HDRI CDF)
        uint64_t bytes = (uint64_t)n * (9 * 3 + 6 + 1 + 1) * 4 + (uint64_t)d->material_count * sizeof(ErMaterial);
        for (uint32_t i = 0; i < d->texture_count && d->textures; i++)
            bytes += (uint64_t)std::max(0, d->textures[i].width) * std::max(0, d->textures[i].height) * std::max(0, d->textures[i].channels) * 4;
        bytes += (uint64_t)std::max(0, d->hdri.texture.width) * std::max(0, d->hdri.texture.height) * (std::max(0, d->hdri.texture.channels) + 1) * 4;
        host_reserve(bytes);
    }
    if (d->texture_count && !d->textures) return fail(ER_ERR_INVALID_ARG, "er_scene_create: texture table missing");
    std::unique_ptr<ErScene> owner(new ErScene());   // released to the caller only on success
    ErScene* s = owner.get();
    s->tri_count = d->tri_count;
    if (n) {
        s->vertices.assign(d->vertices, d->vertices + n * 9);
        s->normals.assign(d->normals, d->normals + n * 9);
        s->tangents.assign(d->tangents, d->tangents + n * 9);
        s->uvs.assign(d->uvs, d->uvs + n * 6);
        s->tangent_sign.assign(d->tangent_sign, d->tangent_sign + n);
        s->material_id.assign(d->material_id, d->material_id + n);
    }
    int rc;
    if ((rc = check_material_ids(s->material_id.data(), n, d->material_count, "er_scene_create")) != ER_OK) return rc;
    s->materials.assign(d->materials, d->materials + d->material_count);
    if ((rc = check_texture_ids(s->materials.data(), s->materials.size(), d->texture_count, "er_scene_create")) != ER_OK) return rc;
    s->textures.resize(d->texture_count);
    for (uint32_t i = 0; i < d->texture_count; i++) {
        if ((rc = copy_tex(d->textures[i], s->textures[i], "scene texture")) != ER_OK) return rc;
    }
    if ((rc = copy_tex(d->hdri.texture, s->hdri_tex, "hdri")) != ER_OK) return rc;
    if (d->hdri.cdf) {
        s->hdri_cdf.assign(d->hdri.cdf, d->hdri.cdf + (size_t)s->hdri_tex.width * s->hdri_tex.height + 1);
        s->hdri_radiance_sum = d->hdri.radiance_sum;
    } else {
        host_generate_cdf(s->hdri_tex, s->hdri_cdf, s->hdri_radiance_sum);
    }
    s->camera = d->camera;
    if (d->point_light_count && d->point_lights) s->point_lights.assign(d->point_lights, d->point_lights + d->point_light_count);
    s->x_res = d->x_res;
    s->y_res = d->y_res;
    *out = owner.release();
    return ER_OK;
}

void er_scene_destroy(ErScene* s) {
    if (!s) return;
    if (s->begun || s->stream) {
        (void)hipSetDevice(s->device);
        if (s->stream) (void)hipStreamSynchronize(s->stream);
    }
    s->release_device();
    delete s;
}

// ---- er_render_begin: a sequence of stages, each with an explicit result ----
// (those an edit in place runs again are declared in er_api_stages.h; the others are this file's own)
namespace erh {

// stage 1: arguments and device; the device's description comes back (its CU count is used by the schedules)
static int begin_check(const ErRenderParams* p, ErDeviceInfo& info) {
    const uint32_t world = p->world ? p->world : 1;
    if (p->rank >= world) return fail(ER_ERR_INVALID_ARG, "er_render_begin: rank >= world");
    // (the schedules keep a path's bounce count in 16 bits of a packed word: one more would read back as a flag, and the path would never end)
    if (p->max_bounces > ER_MAX_BOUNCES)
        return fail(ER_ERR_INVALID_ARG, "er_render_begin: max_bounces " + std::to_string(p->max_bounces) + " is above ER_MAX_BOUNCES (" + std::to_string(ER_MAX_BOUNCES) + ")");
    int ndev = er_device_count();
    if (ndev <= 0) return fail(ER_ERR_NO_DEVICE, "er_render_begin: no HIP device available (there is no CPU fallback)");
    if (p->device < 0 || p->device >= ndev) return fail(ER_ERR_NO_DEVICE, "er_render_begin: device ordinal out of range");
    // the library carries gfx950 code objects only; launching on anything else faults inside the runtime
    int irc = er_device_info(p->device, &info);
    if (irc != ER_OK) return irc;
    if (!info.compatible) return fail(ER_ERR_NO_DEVICE, std::string("er_render_begin: device arch '") + info.arch + "' is not gfx950");
    return ER_OK;
}

// ... the previous render's device state goes, the new one's stream and events are made
static int begin_open(ErScene* s, const ErRenderParams* p) {
    if (s->begun || s->stream) {
        (void)hipSetDevice(s->device);
        if (s->stream) (void)hipStreamSynchronize(s->stream);
        s->release_device();
    }
    s->device = p->device;
    s->params = *p;
    s->ad_on = false;      // (adaptive sampling is set per render, after its er_render_begin)
    s->feat.valid = false; // (the feature planes are of the scene state that ends here)
    s->ids_invalidate();   // (and so are the id planes)
    s->history_invalidate();   // (and the reprojection history)
    s->variance_reset();       // (and the variance moments: the render starts over)
    s->rendered = 0;
    s->params.world = p->world ? p->world : 1;
    if (s->params.max_bounces == 0) s->params.max_bounces = 5;   // the literal of reference src/kernel.cpp:508
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&s->ev_start));
    HIP_TRY(hipEventCreate(&s->ev_stop));
    // Probe one kernel of every translation unit before the first launch: a library that carries no code object
    // this device can run (a stale or mis-targeted build) makes hipLaunchKernelGGL dereference a null function
    // inside the runtime (recorded in round 1: SIGSEGV under er_launch_setup after "No compatible code objects
    // found for gfx950:sramecc+:xnack-").  hipFuncGetAttributes reports the same condition as an error code.
    {
        const char* which = nullptr;
        hipError_t pe = er_probe_kernels(&which);
        if (pe == hipSuccess) pe = er_probe_ids(&which);
        if (pe == hipSuccess) pe = er_probe_first_hit(&which);
        if (pe == hipSuccess) pe = er_probe_history(&which);
        if (pe == hipSuccess) pe = er_probe_history_variance(&which);
        if (pe == hipSuccess) pe = er_probe_variance(&which);
        if (pe != hipSuccess)
            return fail(ER_ERR_HIP, std::string("er_render_begin: libeleven_hip.so has no usable gfx950 code object for ") + (which ? which : "?") +
                                        " on this device (" + hipGetErrorString(pe) + "); rebuild with `make -C elevenrender_amd/csrc`");
    }
    return ER_OK;
}

// stage 2, host builder: the triangle and attribute records in slot order, wide nodes and triangle records in ONE buffer, uploaded
static int accel_upload_host(ErScene* s, BeginStaging& B) {
    const ErGpuBvhDevice& g = s->kept.accel;
    const ErBvhBuild& bvh = B.bvh;
    std::vector<ErTriIsect>& isect = B.isect;
    std::vector<ErTriAttr>& attr = B.attr;
    const size_t n = s->tri_count, n8_pieces = g.n8_pieces;
    int rc;
    isect.resize(n + 1);      // +1: the wide traversal fetches triangles in pairs
    attr.resize(n);
    for (size_t slot = 0; slot < n; slot++) {
        uint32_t id = bvh.slot_to_tri[slot];
        const float* v = &s->vertices[(size_t)id * 9];
        ErTriIsect& r = isect[slot];
        memcpy(r.v0, v, 12); memcpy(r.v1, v + 3, 12); memcpy(r.v2, v + 6, 12);
        r.tri_id = (int32_t)id;
        r.lift = bvh.tri_lift[id];
        r.sign = s->tangent_sign[id];
        ErTriAttr& a = attr[slot];
        memcpy(a.n, &s->normals[(size_t)id * 9], 36);
        memcpy(a.t, &s->tangents[(size_t)id * 9], 36);
        memcpy(a.uv, &s->uvs[(size_t)id * 6], 24);
        a.material = s->material_id[id];
        a.pad[0] = a.pad[1] = a.pad[2] = 0;
    }
    if ((rc = upload(s->d_nodes, bvh.nodes.data(), g.nodes_f4, s->stream)) != ER_OK) return rc;
    memset(&isect[n], 0, sizeof(ErTriIsect));
    // wide nodes and triangle records share ONE buffer: the wide traversal addresses both with a 32-bit
    // offset in 16-byte units
    B.geom.assign(g.geom_f4, make_float4(0, 0, 0, 0));
    for (size_t k = 0; k < bvh.nodes8.size(); k++) memcpy(B.geom.data() + k * ER_NODE8_PIECES, &bvh.nodes8[k], sizeof(ErNode8));
    memcpy(B.geom.data() + n8_pieces, isect.data(), (n + 1) * sizeof(ErTriIsect));
    if ((rc = upload(s->d_nodes8, B.geom.data(), B.geom.size(), s->stream)) != ER_OK) return rc;
    return upload(s->d_attr, attr.data(), g.attr_f4, s->stream);
}

// whether stage 2 asks the device builder first
bool accel_device_first(const ErScene* s) {
    // Which builder: the device build (er_gpu_build.hip: the host builder's binned SAH, level by level on the GPU -- the same tree in a
    // fraction of the time) unless the scene is small enough for the host to be done before the device has started, or the caller says so.
    const uint32_t flags = s->params.flags;
    const bool force_dev = (flags & ER_FLAG_GPU_BUILD) || getenv("ER_GPU_BUILD");
    const bool force_host = !force_dev && ((flags & ER_FLAG_HOST_BUILD) || getenv("ER_HOST_BUILD"));
    uint32_t min_tris = ER_GPU_BUILD_MIN_TRIS;
    if (const char* e = getenv("ER_GPU_BUILD_MIN_TRIS")) min_tris = (uint32_t)std::max(0, atoi(e));
    return !force_host && (force_dev || s->tri_count >= min_tris) && s->tri_count > ER_BVH_LEAF_MAX;
}

// stage 2: the acceleration structure, by the device build or the host's binned-SAH build.  Either builder fills ONE description, `g`,
// ONE block of checks runs on it, it is kept in s->kept.accel (the scene owns the buffers either way: the record's three pointers are
// null), and s->accel.builder says who built.  `built_ev` is recorded when the tree is there and the uploads begin.
int begin_accel(ErScene* s, BeginStaging& B, hipEvent_t built_ev, const char* who, const ErGpuSceneArrays* device_arrays) {
    const std::string W = who;
    ErGpuBvhDevice g;
    s->flush_poses();      // (er_render_transform leaves the host arrays behind: the builders read them)
    const uint32_t flags = s->params.flags;
    const size_t n = s->tri_count;
    bool built = false;
    const bool force_dev = (flags & ER_FLAG_GPU_BUILD) || getenv("ER_GPU_BUILD");
    if (accel_device_first(s)) {
        // whole structure on the device: tree, wide-node collapse, slot order, triangle records
        std::string why;
        ErGpuSceneArrays arrays{s->vertices.data(), s->normals.data(), s->tangents.data(), s->uvs.data(), s->tangent_sign.data(), s->material_id.data()};
        int brc = device_arrays ? er_gpu_build_device_arrays(*device_arrays, s->tri_count, s->device, &g, why) : er_gpu_build_device(arrays, s->tri_count, s->device, &g, why);
        if (brc < 0 && force_dev) return fail(brc == -2 ? ER_ERR_OOM : ER_ERR_HIP, W + ": device BVH build: " + why);
        // What a default device build that did not deliver means: a DECLINE (> 0: too few triangles, a tree deeper than the
        // traversal stacks) and OUT OF DEVICE MEMORY (-2: the build's transient buffers beside other scenes or ranks) are ordinary -- the
        // host builder takes over silently (ER_GPU_BUILD_VERBOSE says so).  Anything else (-1: a HIP error, one of the builder's own
        // guards) is a fault of the builder: the host build still takes over -- the caller gets its image -- but never silently:
        // one line on stderr, unconditionally, with the reason.
        if (brc < 0) (void)hipGetLastError();
        if (brc == -1) fprintf(stderr, "[eleven_hip] %s: the device BVH build FAILED (%s); the host builder takes over (seconds instead of milliseconds at this size) -- please report\n", who, why.c_str());
        else if (brc != 0 && getenv("ER_GPU_BUILD_VERBOSE")) fprintf(stderr, "[er_gpu_build] %s: the host builds instead\n", why.c_str());
        if (brc == 0) {
            // the scene owns the three buffers from here on (release_device frees them on any later error)
            s->d_nodes.release(); s->d_nodes8.release(); s->d_attr.release();
            s->d_nodes.p = g.nodes; s->d_nodes.n = g.nodes_f4;
            s->d_nodes8.p = g.geom; s->d_nodes8.n = g.geom_f4;
            s->d_attr.p = g.attr; s->d_attr.n = g.attr_f4;
            built = true;
        } else g = ErGpuBvhDevice{};
        // brc > 0: the device builder declined (tree too deep for the traversal stacks); brc < 0 without the flag: it failed -- host build
    }
    if (!built) {
        host_reserve((uint64_t)n * (sizeof(ErTriIsect) * 2 + sizeof(ErTriAttr) + 2 * sizeof(ErNode)));
        const ErBvhBuild& bvh = B.bvh;
        er_build_bvh(s->vertices.data(), s->normals.data(), s->tri_count, 0, &B.bvh);
        g.n8_pieces = bvh.nodes8.size() * ER_NODE8_PIECES + 8;   // + padding: a step fetches 96 B from a node's start
        g.nodes_f4 = bvh.nodes.size() * 4; g.geom_f4 = g.n8_pieces + (n + 1) * 3; g.attr_f4 = n * ER_ATTR_PIECES;      // (n + 1: the wide traversal fetches triangles in pairs)
        g.nodes8_count = (uint32_t)bvh.nodes8.size(); g.max_depth8 = bvh.max_depth8; g.max_depth2 = bvh.max_depth; g.leaf_count = bvh.leaf_count;
        for (int a = 0; a < 3; a++) { g.lo[a] = bvh.lo[a]; g.hi[a] = bvh.hi[a]; }
        g.lift_bound = bvh.lift_bound;
        g.build_ms = bvh.build_ms;
    }
    HIP_TRY(hipEventRecord(built_ev, s->stream));
    // what the kernels are sized for, whoever built (the stream schedule's and the wavefront's spill regions hold ER_STACK8 levels of
    // the wide tree per wave, the exact re-trace stacks ER_BVH_MAX_DEPTH of the binary one)
    if (g.max_depth2 > ER_BVH_MAX_DEPTH) return fail(ER_ERR_STATE, W + ": BVH deeper than the traversal stack");
    if (g.max_depth8 > ER_STACK8) return fail(ER_ERR_STATE, W + ": wide BVH deeper than the traversal stack (ER_STACK8)");
    if (g.geom_f4 >= (1ull << 30)) return fail(ER_ERR_INVALID_ARG, W + ": geometry exceeds the 16 GB addressable by the wide traversal");
    s->accel.builder = built ? 1u : 0u;
    s->accel_version++;            // (er_accel_cost's kept result and ER_REBUILD_AUTO's baseline were another tree's)
    s->baseline_known = false;
    s->kept.accel = g;
    s->kept.accel.nodes = s->kept.accel.geom = s->kept.accel.attr = nullptr;      // (the scene owns the buffers)
    return built ? ER_OK : accel_upload_host(s, B);
}

// what er_accel_info and er_debug_read_accel report of a structure that begin_accel has just made
void accel_publish(ErScene* s, float up_ms) {
    const ErGpuBvhDevice& g = s->kept.accel;
    s->accel.node_count = g.nodes8_count;
    s->accel.node_bytes = sizeof(ErNode8);
    s->accel.max_depth = g.max_depth8;
    s->accel.leaf_count = g.leaf_count;
    s->accel.tri_record_bytes = sizeof(ErTriIsect);
    s->accel.build_ms = (float)g.build_ms;
    s->accel.upload_ms = up_ms;
    s->accel.lift_bound = g.lift_bound;
    for (int a = 0; a < 3; a++) { s->accel_lo[a] = g.lo[a]; s->accel_hi[a] = g.hi[a]; }
    s->accel_depth2 = g.max_depth2;
}

// the materials and their precomputed constants (stage 3 without the point lights: what a material edit runs again)
int upload_materials(ErScene* s, BeginStaging& B) {
    int rc;
    if ((rc = upload(s->d_materials, s->materials.data(), s->materials.size(), s->stream)) != ER_OK) return rc;
    std::vector<float4>& mat_pre = B.mat_pre;
    mat_pre.resize(s->materials.size());
    for (size_t i = 0; i < s->materials.size(); i++) {      // DevScene::mat_pre: the per-material constants of generate_hit_data and GTR1
        const ErMaterial& m = s->materials[i];
        const float a = 0.1f + m.clearcoat_gloss * (0.001f - 0.1f);      // lerpf(0.1f, 0.001f, clearcoatGloss), src/Math.hpp:38-41
        const float a2 = a * a;
        mat_pre[i] = make_float4(ermath::er_pow(m.roughness, 2.2f), ermath::er_pow(m.metallic, 2.2f), a < 1.0f ? ermath::er_log(a2) : 0.0f, a < 1.0f ? 1.0f : 0.0f);
    }
    if (getenv("ER_MAT_PRE_ON_DEVICE")) for (auto& v : mat_pre) v.w = 0.0f;      // (A/B and test knob: GTR1's logarithm on the device)
    return upload(s->d_mat_pre, mat_pre.data(), mat_pre.size(), s->stream);
}

// stage 3: materials, their precomputed constants, point lights
static int begin_materials(ErScene* s, BeginStaging& B) {
    int rc;
    if ((rc = upload_materials(s, B)) != ER_OK) return rc;
    return upload(s->d_lights, s->point_lights.data(), s->point_lights.size(), s->stream);
}

// the scene's host textures as the texture plan (er_texplan.h) takes them
void plan_of_scene(const ErScene* s, TexPlan& P) {
    std::vector<TexDecl> decl(s->textures.size());
    for (size_t i = 0; i < decl.size(); i++) decl[i] = TexDecl{s->textures[i].width, s->textures[i].height, s->textures[i].channels, s->textures[i].filter};
    const TexDecl h{s->hdri_tex.width, s->hdri_tex.height, s->hdri_tex.channels, s->hdri_tex.filter};
    er_texture_plan(decl.data(), decl.size(), s->materials.data(), s->materials.size(), h, P);
}

// stage 4: the texture pool.  Needs only the host scene; leaves the pool, the table, the fused records, the HDRI's CDF and its guide
// on the device and the per-texture modes in s->tex_mode.  Every layout decision -- modes, offsets, which materials are fused -- is the
// texture plan's (er_texplan.h, where the rules are written down); this stage fills that layout on the HOST (er_render_edit fills the
// same layout on the device, er_texstage.hip).  The HDRI's table entry and its guide's buckets go to s->kept.
static int begin_textures(ErScene* s, BeginStaging& B, const char* who) {
    int rc;
    std::vector<DevTex>& table = B.table;
    std::vector<float>& pool = B.pool;
    std::vector<DevFused>& fused = B.fused;
    TexPlan P;
    plan_of_scene(s, P);
    if ((rc = check_pool_floats(P.pool_floats, who)) != ER_OK) return rc;
    table = P.table;
    fused = P.fused;
    const std::vector<uint8_t>& mode = P.mode;
    s->tex_mode = mode;
    pool.resize((size_t)P.pool_floats);
    // the one-channel copies are made by a few threads (C5: 8.4 M er_pow, ~0.2 s on one core), each texture at its offset.
    // (The pool is sized HERE, on the calling thread: a std::bad_alloc then unwinds into guarded() -> ER_ERR_OOM; thrown inside a
    // worker it would be an uncaught exception of that thread, i.e. std::terminate.  The workers below only compute.)
    {
        std::atomic<size_t> next{0};
        auto work = [&]() noexcept {
            for (size_t i = next.fetch_add(1); i < s->textures.size(); i = next.fetch_add(1)) {
                if (!mode[i]) continue;
                const HostTex& t = s->textures[i];
                const size_t n = (size_t)t.width * (size_t)t.height;
                float* one = pool.data() + table[i].offset;
                for (size_t k = 0; k < n; k++) {
                    const float v = t.data[k * (size_t)t.channels];
                    one[k] = mode[i] == 2 ? ermath::er_pow(v, 2.2f) : v;
                }
            }
        };
        const unsigned nt = std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency()));
        // (joined by a scope guard: if a std::thread constructor throws while earlier workers run, they are joined before the
        // exception leaves this block -- a joinable thread destroyed is std::terminate -- and the work they did not get to is done here)
        struct JoinAll {
            std::vector<std::thread> th;
            ~JoinAll() { for (auto& x : th) if (x.joinable()) x.join(); }
        } pool_threads;
        pool_threads.th.reserve(nt);
        try {
            for (unsigned k = 1; k < nt; k++) pool_threads.th.emplace_back(work);
        } catch (const std::system_error&) {
            // fewer workers than asked for: the calling thread takes what is left
        }
        work();
    }
    for (size_t i = 0; i < s->textures.size(); i++) {
        const HostTex& t = s->textures[i];
        if (!mode[i] && !t.data.empty()) memcpy(pool.data() + table[i].offset, t.data.data(), t.data.size() * sizeof(float));
    }
    for (size_t m = 0; m < s->materials.size(); m++) {
        if (fused[m].width <= 0) continue;
        const ErMaterial& M = s->materials[m];
        const HostTex &A = s->textures[(size_t)M.albedo_tex], &R = s->textures[(size_t)M.roughness_tex], &K = s->textures[(size_t)M.metallic_tex];
        const bool powered = fused[m].filter == 2;
        const size_t n = (size_t)A.width * (size_t)A.height;
        // (a texture the pass above already raised to the power is copied from the pool, not raised again: C5's 8.4 M texels)
        const DevTex tr = table[(size_t)M.roughness_tex], tk = table[(size_t)M.metallic_tex];
        const bool r_done = powered && tr.filter == 2, k_done = powered && tk.filter == 2;
        float* o = pool.data() + fused[m].offset;
        for (size_t k = 0; k < n; k++, o += 5) {
            const float* a = A.data.data() + k * (size_t)A.channels;
            const float r = r_done ? pool[tr.offset + k] : R.data[k * (size_t)R.channels], mt = k_done ? pool[tk.offset + k] : K.data[k * (size_t)K.channels];
            // (one channel: the value three times; two: x, y, 0; three or more: the first three -- src/Texture.cpp:181-197)
            o[0] = a[0];
            o[1] = A.channels == 1 ? a[0] : a[1];
            o[2] = A.channels == 1 ? a[0] : (A.channels == 2 ? 0.0f : a[2]);
            o[3] = powered && !r_done ? ermath::er_pow(r, 2.2f) : r;
            o[4] = powered && !k_done ? ermath::er_pow(mt, 2.2f) : mt;
        }
    }
    s->fused_any = P.fused_any;
    if ((rc = upload(s->d_mat_fused, fused.data(), fused.size(), s->stream)) != ER_OK) return rc;
    s->kept.hdri = P.hdri;
    if (!s->hdri_tex.data.empty()) memcpy(pool.data() + P.hdri.offset, s->hdri_tex.data.data(), s->hdri_tex.data.size() * sizeof(float));
    if ((rc = upload(s->d_textures, table.data(), table.size(), s->stream)) != ER_OK) return rc;
    if ((rc = upload(s->d_tex_pool, pool.data(), pool.size(), s->stream)) != ER_OK) return rc;
    s->tex_pool_cap = pool.size();
    if ((rc = upload(s->d_cdf, s->hdri_cdf.data(), s->hdri_cdf.size(), s->stream)) != ER_OK) return rc;
    return upload_hdri_guide(s, B);
}

// the CDF's guide table and, behind it in the same buffer, the row and column tables of the HDRI's sample directions (er_hdri_trig.h),
// which one kernel fills on the device from the descriptor s->kept.hdri
int upload_hdri_guide(ErScene* s, BeginStaging& B) {
    int rc;
    s->kept.buckets = er_build_cdf_guide(s->hdri_cdf.data(), s->hdri_tex.width * s->hdri_tex.height, B.guide);
    const size_t at = (B.guide.size() + 3) & ~(size_t)3;      // (16-byte aligned)
    B.guide.resize(at + erd::hdri_trig_words(s->kept.hdri.width, s->kept.hdri.height), 0u);
    if ((rc = upload(s->d_guide, B.guide.data(), B.guide.size(), s->stream)) != ER_OK) return rc;
    s->kept.trig_at = at;
    er_launch_hdri_trig(s->kept.hdri, s->d_guide.p + at, s->stream);
    HIP_TRY(hipGetLastError());
    return ER_OK;
}

// stage 5, ER_FLAG_MESH_LIGHTS: the emitter table, built on the device from the placed triangle records (er_lights.hip).  An empty
// table leaves the render as it would be without the flag.
int begin_emitters(ErScene* s, BeginStaging& B, const char* who) {
    if (!(s->params.flags & ER_FLAG_MESH_LIGHTS)) return ER_OK;
    int rc;
    std::vector<int32_t>& etex = B.etex;
    for (const ErMaterial& m : s->materials)
        if (m.emission_tex >= 0 && (size_t)m.emission_tex < s->textures.size()) etex.push_back(m.emission_tex);
    std::sort(etex.begin(), etex.end());
    etex.erase(std::unique(etex.begin(), etex.end()), etex.end());
    ScopedDevBuf<int32_t> d_etex;
    if ((rc = upload(d_etex, etex.data(), etex.size(), s->stream)) != ER_OK) return rc;
    float* tab = nullptr;
    HIP_TRY(er_lights_build(s->d_nodes8.p + s->kept.accel.n8_pieces, s->d_attr.p, s->tri_count, s->d_materials.p, s->d_textures.p, s->d_tex_pool.p, d_etex.p,
                            (uint32_t)etex.size(), (uint32_t)s->textures.size(), &tab, &s->light_emitters, &s->light_total, s->stream));
    s->d_light_tab.p = tab;
    s->d_light_tab.n = tab ? (size_t)s->tri_count + 2 * (size_t)s->light_emitters : 0;
    if (s->lights_on() && s->light_emitters > 0)
        return fail(ER_ERR_INVALID_ARG, std::string(who) + ": ER_FLAG_POINT_LIGHTS and ER_FLAG_MESH_LIGHTS on a scene with both point lights and "
                                                           "emissive triangles: both need the one light-query record per slot");
    return ER_OK;
}

// stage 6: the planes, this rank's tiles, the counters ...
static int begin_planes(ErScene* s, BeginStaging& B) {
    int rc;
    const size_t npx = (size_t)s->x_res * s->y_res;
    if ((rc = upload(s->d_passes, nullptr, npx * ER_PASS_COUNT, s->stream)) != ER_OK) return rc;
    if ((rc = upload(s->d_samples, nullptr, npx, s->stream)) != ER_OK) return rc;
    if ((rc = upload(s->d_rng, nullptr, npx, s->stream)) != ER_OK) return rc;
    B.owned = s->tiles_of(s->params.rank, s->params.world);
    if ((rc = upload(s->d_owned, B.owned.data(), B.owned.size(), s->stream)) != ER_OK) return rc;
    if ((rc = upload(s->d_counters, nullptr, 1, s->stream)) != ER_OK) return rc;
    HIP_TRY(hipMemsetAsync(s->d_counters.p, 0, sizeof(DevCounters), s->stream));
    return ER_OK;
}

// ... and the schedule (into s->params.flags): forced by a flag, else the streaming schedule unless this rank's share is beyond its
// pixel rings (see eleven_hip.h).  B.deal is made here for the streaming schedule to start with.
static int begin_choose_schedule(ErScene* s, BeginStaging& B, uint32_t cus) {
    const uint32_t all = ER_FLAG_MEGAKERNEL | ER_FLAG_FUSED | ER_FLAG_WAVEFRONT | ER_FLAG_STREAM;
    uint32_t forced = s->params.flags & all;
    // (ER_FLAG_FUSED named round 1's lane-asynchronous single kernel, which the streaming schedule has overtaken at every frame size --
    // C1 at 256 x 256: 1 186 against 849 Msamples/s, profiles/r05_schedules_small_frames.log -- and which round 5 removed: the flag
    // is still accepted and means the streaming schedule)
    if (forced == ER_FLAG_FUSED) forced = ER_FLAG_STREAM;
    if (forced & (forced - 1)) return fail(ER_ERR_INVALID_ARG, "er_render_begin: more than one schedule flag");
    uint32_t sched = forced;
    if (forced == 0 || forced == ER_FLAG_STREAM) B.deal = stream_deal_owned(B.owned, s->tiles_x(), cus);
    if (forced == 0) {
        // beyond the streaming schedule's pixel rings -> wavefront.  Decided on the REAL deal of tiles to workgroups, not on an
        // estimate of its largest share: the XCD-aware deal hands out whole super-tiles and can be less balanced than
        // ceil(tiles / CUs) (near the limit the estimate chose ER_FLAG_STREAM and er_render_begin then failed
        // with INVALID_ARG instead of taking the other schedule)
        // (and the streaming schedule carries a pixel as px | py << 16)
        sched = ((size_t)B.deal.most * 64u > ER_STREAM_MAX_RING || s->x_res > 65535u || s->y_res > 65535u) ? ER_FLAG_WAVEFRONT : ER_FLAG_STREAM;
    }
    s->params.flags = (s->params.flags & ~all) | sched;
    return ER_OK;
}

// stage 7, ER_FLAG_WAVEFRONT (the streaming schedule's: stream_begin, er_stream_host.cpp)
static int begin_wavefront(ErScene* s, const std::vector<uint32_t>& owned, uint32_t cus, bool query_on) {
    int rc;
    // wavefront path state: one slot per owned pixel lane.
    // SLOT POOLS: the owned tiles are dealt round-robin to `pools` independent path pools, each with its own
    // queues and counters and its own HIP stream.  A ray is a sequential chain of dependent fetches, so every
    // trace launch ends in a tail in which the last long rays keep a few lanes busy while the chip idles
    // (measured: 29 % of all lane slots fall after the queue has run dry, at 19 % lane occupancy); the launches
    // of one pool fill the tails of the others.  Pools never exchange data (disjoint pixels), so the planes
    // do not depend on their number.  Measured on C2: 1 pool 901, 2 pools 959, 3 pools 969, 4 pools 947.
    uint32_t pools = 3;
    if (const char* e = getenv("ER_WF_POOLS")) pools = (uint32_t)std::min(8, std::max(1, atoi(e)));   // tuning knob
    pools = std::min<uint32_t>(pools, std::max<uint32_t>(1u, (uint32_t)owned.size()));
    const size_t pool_tiles = (owned.size() + pools - 1) / pools;
    const size_t qcap = pool_tiles * 64;          // queue capacity of one pool
    size_t slots = owned.size() * 64;
    const size_t sh = query_on ? 2 : 1;           // shadow records per slot: [slot] HDRI query, [slot + slots] point light / emitter
    const size_t qs_cap = qcap * sh;              // shadow-queue capacity of one pool
    const size_t q_words = 2 * qcap + 2 * qs_cap; // two closest + two shadow queues per pool
    if ((rc = upload(s->d_wf4, nullptr, slots * (7 + 4 * sh), s->stream)) != ER_OK) return rc;
    if ((rc = upload(s->d_wf1, nullptr, slots * (3 + 3 * sh) + q_words * pools + (size_t)WF_COUNTS * pools, s->stream)) != ER_OK) return rc;
    WfState W{};
    float4* f = s->d_wf4.p;
    W.ray_o = f; W.ray_d = f + slots; W.light = f + 2 * slots; W.reduc = f + 3 * slots;
    W.aov_n = f + 4 * slots; W.aov_t = f + 5 * slots; W.aov_b = f + 6 * slots;
    W.sh_o = f + 7 * slots; W.sh_d = W.sh_o + sh * slots; W.c_vis = W.sh_d + sh * slots; W.c_occ = W.c_vis + sh * slots;
    uint32_t* u = s->d_wf1.p;
    W.hit = (int*)u; W.left = u + slots; W.hit2 = (int*)(u + 2 * slots);
    W.occluded = (int*)(u + 3 * slots); W.occ_a = W.occluded + sh * slots; W.occ_b = W.occ_a + sh * slots;
    uint32_t* qbase = u + (3 + 3 * sh) * slots;
    uint32_t* cbase = qbase + q_words * pools;
    W.pools = pools;
    W.slots = (uint32_t)slots;
    // persistent waves per CU, tuned together with the pools (the launches of different pools share the CUs):
    // trace 8/10/12/14/16 -> 1016/1046/1043/1022/1042 Msamples/s at shade 5; shade 4/5/6/7 -> 1019/1051/1012/987
    s->trace_blocks = cus * 12;
    s->shade_blocks = cus * 5;
    if (const char* e = getenv("ER_TRACE_WAVES_PER_CU")) s->trace_blocks = cus * (uint32_t)std::max(1, atoi(e));   // tuning knob
    if (const char* e = getenv("ER_SHADE_WAVES_PER_CU")) s->shade_blocks = cus * (uint32_t)std::max(1, atoi(e));
    // (uint2 entries: the trace waves' stack levels beyond the LDS ones, then the shade waves' exact re-trace stacks, two ints per entry)
    const size_t trace_spill = (size_t)s->trace_blocks * ER_STACK8 * 64;
    const size_t spill_per_pool = trace_spill + (size_t)s->shade_blocks * ER_BVH_MAX_DEPTH * 32;
    if ((rc = upload(s->d_spill, nullptr, spill_per_pool * pools, s->stream)) != ER_OK) return rc;
    s->wf.clear();
    for (uint32_t p2 = 0; p2 < pools; p2++) {
        W.pool = p2;
        uint32_t* q = qbase + (size_t)p2 * q_words;
        W.q[0] = q; W.q[1] = q + qcap; W.qs[0] = q + 2 * qcap; W.qs[1] = q + 2 * qcap + qs_cap;
        W.counts = cbase + (size_t)p2 * WF_COUNTS;
        W.spill = s->d_spill.p + (size_t)p2 * spill_per_pool;
        W.shade_stack = (int*)(W.spill + trace_spill);
        s->wf.push_back(W);
    }
    for (uint32_t p2 = 1; p2 < pools; p2++) {
        hipStream_t st;
        HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        s->pool_streams.push_back(st);
    }
    for (uint32_t p2 = 0; p2 < pools; p2++) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        s->pool_events.push_back(e);
    }
    return ER_OK;
}

// stage 8: the scene descriptor, on the host and on the device
static int begin_descriptor(ErScene* s, uint32_t owned_tiles) {
    const ErGpuBvhDevice& g = s->kept.accel;
    const float lift_bound = g.lift_bound;
    float scene_scale = 0;
    for (int a = 0; a < 3; a++) scene_scale = std::max(scene_scale, std::max(std::fabs(g.lo[a]), std::fabs(g.hi[a])));
    scene_scale = std::max(scene_scale, std::max(std::fabs(s->camera.position.x), std::max(std::fabs(s->camera.position.y), std::fabs(s->camera.position.z))));

    DevScene& D = s->dev;
    memset(&D, 0, sizeof(D));
    D.nodes = s->d_nodes.p;
    D.nodes8 = s->d_nodes8.p;
    D.tri_isect = s->d_nodes8.p + g.n8_pieces;
    D.tri_base_pieces = (uint32_t)g.n8_pieces;
    D.tri_attr = s->d_attr.p;
    D.tri_count = s->tri_count;
    D.node_count = (uint32_t)(g.nodes_f4 / 4);
    D.node8_count = g.nodes8_count;
    D.prune_margin = lift_bound + 1e-5f * scene_scale;
    D.max_lift = lift_bound;
    D.scene_scale = scene_scale;
    D.materials = s->d_materials.p;
    D.mat_pre = s->d_mat_pre.p;
    D.textures = s->d_textures.p;
    D.tex_pool = s->d_tex_pool.p;
    D.mat_fused = s->d_mat_fused.p;
    D.fused_any = s->fused_any ? 1u : 0u;
    D.hdri_tex = s->kept.hdri;
    D.hdri_cdf = s->d_cdf.p;
    D.hdri_guide = s->d_guide.p;
    D.hdri_buckets = s->kept.buckets;
    D.hdri_radiance_sum = s->hdri_radiance_sum;
    // (A/B and test knob: ER_HDRI_TRIG_ON_DEVICE=1 = the kernels evaluate the sample's sines and cosines themselves)
    D.hdri_trig = getenv("ER_HDRI_TRIG_ON_DEVICE") ? nullptr : s->d_guide.p + s->kept.trig_at;
    D.cam = s->camera;
    D.x_res = s->x_res;
    D.y_res = s->y_res;
    D.tiles_x = s->tiles_x();
    D.tiles_y = s->tiles_y();
    D.max_bounces = s->params.max_bounces;
    {   // power-of-two sides everywhere: texture coordinates wrap with a mask instead of a signed division (er_device.h wrap_abs)
        auto pow2 = [](int32_t v) { return v > 0 && (v & (v - 1)) == 0; };
        bool all = pow2(s->kept.hdri.width) && pow2(s->kept.hdri.height);
        for (const HostTex& t : s->textures) all = all && pow2(t.width) && pow2(t.height);
        D.tex_pow2 = all ? 1u : 0u;
        if (const char* e = getenv("ER_TEX_POW2")) D.tex_pow2 = (atoi(e) != 0 && all) ? 1u : 0u;      // A/B knob: 0 = always the division
    }
    D.trace_every_query = 0u;      // (test and A/B knob: 1 = shadow queries whose two outcomes are the same addend are traced as well, er_bounce.inc)
    if (const char* e = getenv("ER_TRACE_EVERY_QUERY")) D.trace_every_query = atoi(e) != 0 ? 1u : 0u;
    D.ext_flags = s->params.flags & (ER_FLAG_POINT_LIGHTS | ER_FLAG_MIS);
    D.lights = s->d_lights.p;
    D.light_count = (uint32_t)s->point_lights.size();
    if (s->light_emitters > 0) {      // (the words of the point lights, which this render does not sample: er_device.h)
        D.ext_flags = (D.ext_flags & ~(uint32_t)ER_FLAG_POINT_LIGHTS) | ER_FLAG_MESH_LIGHTS;
        D.mesh_lights = s->d_light_tab.p;
        D.emitter_count = s->light_emitters;
    }
    D.passes = s->d_passes.p;
    D.samples = s->d_samples.p;
    D.rng = s->d_rng.p;
    D.owned_tiles = s->d_owned.p;
    D.owned_tile_count = owned_tiles;
    D.counters = s->d_counters.p;
    D.tile_cost = ((s->params.flags & ER_FLAG_STREAM) && s->st.counting) ? s->st.d_tile_cost.p : nullptr;
    D.px_draws = (s->params.flags & ER_FLAG_STREAM) ? s->st.d_px_draws.p : nullptr;
    {   // the camera's rotation sines / cosines, once, with the functions the device would call (er_math.h: one implementation for both sides)
        const erd::CamTrig t = erd::camera_trig(D.cam);
        D.cam_cx = t.cx; D.cam_sx = t.sx; D.cam_cy = t.cy; D.cam_sy = t.sy; D.cam_cz = t.cz; D.cam_sz = t.sz;
        D.cam_trig_valid = getenv("ER_CAM_TRIG_ON_DEVICE") ? 0u : 1u;      // (A/B and test knob: 1 = use the host's values)
    }
    return upload(s->d_dev, &D, 1, s->stream);
}

// stages 6-8 and the set-up launch: the render's own state -- planes, schedule, descriptor -- on a structure, materials and textures that
// are in place.  The tail of er_render_begin, and what every edit in place ends in.  `uploads_done` (may be null) is recorded
// before the descriptor goes up.  Leaves the stream idle.
int begin_render_state(ErScene* s, BeginStaging& B, hipEvent_t uploads_done) {
    int rc;
    const uint32_t cus = s->kept.cus;
    const bool query_on = s->query_on();
    if ((rc = begin_planes(s, B)) != ER_OK) return rc;
    if ((rc = begin_choose_schedule(s, B, cus)) != ER_OK) return rc;
    if (s->params.flags & ER_FLAG_STREAM) rc = stream_begin(s, B.owned, B.deal, cus, query_on);
    else if (s->params.flags & ER_FLAG_WAVEFRONT) rc = begin_wavefront(s, B.owned, cus, query_on);
    if (rc != ER_OK) return rc;
    if (uploads_done) HIP_TRY(hipEventRecord(uploads_done, s->stream));
    if ((rc = begin_descriptor(s, (uint32_t)B.owned.size())) != ER_OK) return rc;

    er_launch_setup(s->dev, s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ER_OK;
}

}  // namespace erh

static int er_render_begin_impl(ErScene* s, const ErRenderParams* p) {
    if (!s || !p) return fail(ER_ERR_INVALID_ARG, "er_render_begin: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    int rc;
    ErDeviceInfo info;
    if ((rc = begin_check(p, info)) != ER_OK) return rc;
    if ((rc = begin_open(s, p)) != ER_OK) return rc;
    const char* who = "er_render_begin";
    s->kept.cus = std::max(1u, info.compute_units);
    s->kept.flags = p->flags;
    EventPair ev;                       // (upload time: from the tree being there to the last upload enqueued) destroyed on every return path
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    BeginStaging B;                     // outlives the hipStreamSynchronize below
    if ((rc = begin_accel(s, B, ev.a, who)) != ER_OK) return rc;
    if ((rc = begin_materials(s, B)) != ER_OK) return rc;
    if ((rc = begin_textures(s, B, who)) != ER_OK) return rc;
    if ((rc = begin_emitters(s, B, who)) != ER_OK) return rc;
    if ((rc = begin_render_state(s, B, ev.b)) != ER_OK) return rc;
    float up_ms = 0;
    (void)hipEventElapsedTime(&up_ms, ev.a, ev.b);

    accel_publish(s, up_ms);
    s->begun = true;
    return ER_OK;
}

// n more samples of the wavefront schedule: trace and shade launches of every slot pool, on the pools' streams
static int wavefront_enqueue(ErScene* s, const DevScene& D, uint32_t n, bool count) {
    // a path takes at most max_bounces ray steps plus one finalize-only step
    const uint64_t iters64 = (uint64_t)n * ((uint64_t)s->params.max_bounces + 1u);
    if (iters64 > 0xFFFFFFFFull)      // (refused before anything is launched: a wrapped count would render fewer iterations than the samples need)
        return fail(ER_ERR_INVALID_ARG, "er_render_samples: " + std::to_string(n) + " samples of " + std::to_string(s->params.max_bounces) +
                                            " bounces are more than 4294967295 iterations of the wavefront schedule in one call");
    const uint32_t iters = (uint32_t)iters64;
    const uint32_t pools = (uint32_t)s->wf.size();
    const bool prof = (s->params.flags & ER_FLAG_PROFILE) != 0;
    if (prof) {
        const size_t need = s->prof_used / 3 + (size_t)iters * pools;      // launches profiled since the last er_wait
        while (s->prof_events.size() < 3 * need) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            s->prof_events.push_back(e);
        }
        if (s->d_ray_log.n < need) {
            // grow, keeping what earlier calls of this timing window logged (they are still in flight or done)
            DevBuf<uint32_t> bigger;
            int rc2 = upload(bigger, nullptr, need * 2, s->stream);
            if (rc2 != ER_OK) return rc2;
            if (s->d_ray_log.p && s->prof_used) {
                HIP_TRY(hipStreamSynchronize(s->stream));
                HIP_TRY(hipMemcpy(bigger.p, s->d_ray_log.p, (s->prof_used / 3) * sizeof(uint32_t), hipMemcpyDeviceToDevice));
            }
            s->d_ray_log.release();
            s->d_ray_log = bigger;
        }
    }
    // fork: the pool streams start after everything already enqueued on the scene's stream
    if (pools > 1) {
        HIP_TRY(hipEventRecord(s->pool_events[0], s->stream));
        for (uint32_t p = 1; p < pools; p++) HIP_TRY(hipStreamWaitEvent(s->pool_streams[p - 1], s->pool_events[0], 0));
    }
    auto pool_stream = [&](uint32_t p) { return p == 0 ? s->stream : s->pool_streams[p - 1]; };
    for (uint32_t p = 0; p < pools; p++) er_launch_wf_begin(D, s->wf[p], n, pool_stream(p));
    for (uint32_t it = 0; it < iters; it++) {
        for (uint32_t p = 0; p < pools; p++) {
            hipStream_t st = pool_stream(p);
            uint32_t* ray_log = prof ? s->d_ray_log.p + s->prof_used / 3 : nullptr;
            if (prof) HIP_TRY(hipEventRecord(s->prof_events[s->prof_used++], st));
            er_launch_wf_trace(D, s->wf[p], it & 1, count, s->trace_blocks, ray_log, st);
            if (prof) HIP_TRY(hipEventRecord(s->prof_events[s->prof_used++], st));
            er_launch_wf_shade(D, s->wf[p], it & 1, count, s->shade_blocks, st);
            if (prof) HIP_TRY(hipEventRecord(s->prof_events[s->prof_used++], st));
        }
    }
    // join: the scene's stream continues once every pool has drained
    for (uint32_t p = 1; p < pools; p++) {
        HIP_TRY(hipEventRecord(s->pool_events[p], s->pool_streams[p - 1]));
        HIP_TRY(hipStreamWaitEvent(s->stream, s->pool_events[p], 0));
    }
    return ER_OK;
}

// n more samples to every active tile (all owned tiles unless an adaptive render has stopped some), enqueued on the scene's stream;
// the caller holds s->mtx.  The streaming kernel is handed the active tiles through its deal (StreamHost::d_deal), the wavefront and
// megakernel schedules through the tile list of the scene descriptor they are launched with.
static int enqueue_samples(ErScene* s, uint32_t n) {
    const DevScene& D = s->ad_on ? s->ad_dev : s->dev;
    const bool count = (s->params.flags & ER_FLAG_COUNTERS) != 0;
    int rc = ER_OK;
    if (!(s->params.flags & (ER_FLAG_MEGAKERNEL | ER_FLAG_STREAM))) {
        if (n > 0) rc = wavefront_enqueue(s, D, n, count);
    } else {
        const bool prof = (s->params.flags & ER_FLAG_PROFILE) && n > 0;
        if (prof) {
            while (s->prof_events.size() < s->prof_used + 3) {
                hipEvent_t e;
                HIP_TRY(hipEventCreate(&e));
                s->prof_events.push_back(e);
            }
            HIP_TRY(hipEventRecord(s->prof_events[s->prof_used++], s->stream));
        }
        if (s->params.flags & ER_FLAG_STREAM) rc = stream_enqueue(s, n);
        else er_launch_render(D, n, count, s->stream);
        if (rc == ER_OK && prof) {
            HIP_TRY(hipEventRecord(s->prof_events[s->prof_used++], s->stream));
            HIP_TRY(hipEventRecord(s->prof_events[s->prof_used++], s->stream));   // (trace, shade) triple: shade = 0
        }
    }
    if (rc != ER_OK) return rc;
    HIP_TRY(hipGetLastError());
    return ER_OK;
}

static int adaptive_render(ErScene* s, uint32_t n);

static int er_render_samples_async_impl(ErScene* s, uint32_t n) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_render_samples: NULL scene");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_render_samples: er_render_begin has not succeeded");
    if ((s->params.flags & ER_FLAG_STREAM) && n >= (1u << 24))      // (its pixel-ring entries keep the samples left in 24 bits)
        return fail(ER_ERR_INVALID_ARG, "er_render_samples: at most 16777215 samples per call in the streaming schedule");
    HIP_TRY(hipSetDevice(s->device));
    if (!s->timing_open) {
        HIP_TRY(hipEventRecord(s->ev_start, s->stream));
        s->timing_open = true;
    }
    if (n > 0) for (auto& u : s->unpacked) u.clear();     // other ranks' pixels gathered earlier are stale from here on
    if (s->ad_on) return adaptive_render(s, n);
    const int rc = enqueue_samples(s, n);
    if (rc == ER_OK) s->rendered += n;      // (a refused call rendered nothing)
    return rc;
}

static int er_wait_impl(ErScene* s, float* elapsed_ms) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_wait: NULL scene");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_wait: er_render_begin has not succeeded");
    HIP_TRY(hipSetDevice(s->device));
    float ms = 0;
    if (s->timing_open) {
        HIP_TRY(hipEventRecord(s->ev_stop, s->stream));
        HIP_TRY(hipEventSynchronize(s->ev_stop));
        HIP_TRY(hipEventElapsedTime(&ms, s->ev_start, s->ev_stop));
        s->timing_open = false;
    } else {
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    if (elapsed_ms) *elapsed_ms = ms;
    { int rc = er_scene_stream_status(s, "er_wait"); if (rc != ER_OK) { s->prof_used = 0; return rc; } }   // (the profiling window ends with the call either way)
    stream_adapt(s);
    s->profile = ErProfile{};
    s->profile.schedule = s->params.flags & (ER_FLAG_MEGAKERNEL | ER_FLAG_WAVEFRONT | ER_FLAG_STREAM);
    s->profile.concurrency = (s->params.flags & ER_FLAG_WAVEFRONT) ? (uint32_t)std::max<size_t>(1, s->wf.size()) : 1u;
    // The wavefront host loop always enqueues n * (max_bounces + 1) iterations per pool; the last ones find empty
    // queues (a path rarely takes every bounce).  Those launches are reported apart, so that per-launch figures are
    // averages over launches that traced something.
    std::vector<uint32_t> ray_log;
    const bool wf = (s->params.flags & ER_FLAG_WAVEFRONT) != 0;
    if (wf && s->prof_used && s->d_ray_log.p) {
        ray_log.resize(s->prof_used / 3);
        HIP_TRY(hipMemcpy(ray_log.data(), s->d_ray_log.p, ray_log.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i + 2 < s->prof_used; i += 3) {
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, s->prof_events[i], s->prof_events[i + 1]));
        HIP_TRY(hipEventElapsedTime(&b, s->prof_events[i + 1], s->prof_events[i + 2]));
        if (wf && i / 3 < ray_log.size() && ray_log[i / 3] == 0) {
            s->profile.empty_launches++;
            s->profile.empty_ms += a + b;
            continue;
        }
        s->profile.trace_ms += a;
        s->profile.shade_ms += b;
        s->profile.trace_launches++;
        s->profile.shade_launches++;
        if (wf && i / 3 < ray_log.size()) s->profile.rays_logged += ray_log[i / 3];
    }
    s->prof_used = 0;
    return ER_OK;
}

static int er_render_samples_impl(ErScene* s, uint32_t n) {
    int rc = er_render_samples_async(s, n);
    if (rc != ER_OK) return rc;
    return er_wait(s, nullptr);
}

// the copy itself; the caller holds s->mtx
static int read_back_locked(ErScene* s, const void* src, void* dst, size_t bytes, const char* who) {
    if (!s->begun) return fail(ER_ERR_STATE, std::string(who) + ": er_render_begin has not succeeded");
    HIP_TRY(hipSetDevice(s->device));
    // ordered after everything enqueued so far: a sample-boundary snapshot, never a torn read
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return er_scene_stream_status(s, who);
}

static int read_back(ErScene* s, const void* src, void* dst, size_t bytes, const char* who) {
    if (!s || !dst) return fail(ER_ERR_INVALID_ARG, std::string(who) + ": NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    return read_back_locked(s, src, dst, bytes, who);
}

static int er_samples_done_impl(ErScene* s, uint32_t* out) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_samples_done: NULL scene");
    // dev_samples[0], reference src/Managers.cpp:217-221; with tile sharding pixel 0 may belong to another
    // rank, so report the first owned pixel instead.
    uint32_t first = 0;
    std::unique_lock<std::mutex> lk(s->mtx);
    if (s->begun && s->params.world > 1) {
        std::vector<uint32_t> t = s->tiles_of(s->params.rank, s->params.world);
        if (!t.empty()) {
            const uint32_t tiles_x = s->tiles_x();
            first = (t[0] / tiles_x) * ER_TILE * s->x_res + (t[0] % tiles_x) * ER_TILE;
        }
    }
    lk.unlock();
    return read_back(s, s->d_samples.p + first, out, sizeof(uint32_t), "er_samples_done");
}

static int er_read_pass_impl(ErScene* s, int pass, float* dst) {
    if (pass < 0 || pass >= ER_PASS_COUNT) return fail(ER_ERR_INVALID_ARG, "er_read_pass: pass out of range");
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_read_pass: NULL scene");
    if (!dst) return fail(ER_ERR_INVALID_ARG, "er_read_pass: NULL argument");
    // the device keeps the accumulated passes interleaved per pixel (er_pass_index, er_device.h): the plane the ABI hands out is
    // gathered into a staging plane first, on the library's stream (so it is the same sample-boundary snapshot as before).
    // ONE staging plane per scene: the lock is held from the gather kernel to the end of the copy, so that two threads reading
    // two passes of one scene cannot interleave as gather A, gather B, copy, copy.
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_read_pass: er_render_begin has not succeeded");
    size_t npx = (size_t)s->x_res * s->y_res;
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    if (s->d_plane.n < npx && (rc = upload(s->d_plane, nullptr, npx, s->stream)) != ER_OK) return rc;
    er_launch_plane(s->dev, pass, s->d_plane.p, s->stream);
    HIP_TRY(hipGetLastError());
    return read_back_locked(s, s->d_plane.p, dst, npx * sizeof(float4), "er_read_pass");
}
// ---- checkpoint / resume: passes + samples + rng are the whole progressive state (reference src/kernel.h:44-46) ----
namespace {
struct StateHeader {
    char magic[8];            // "ERSTATE2" (2: the accumulated passes interleaved per pixel, er_pass_index; a snapshot of layout 1 is refused)
    uint32_t x_res, y_res, passes, reserved;
    uint64_t bytes;
    uint8_t pad[32];
};
static_assert(sizeof(StateHeader) == 64, "snapshot header is 64 bytes");
uint64_t state_bytes(const ErScene* s) {
    const uint64_t npx = (uint64_t)s->x_res * s->y_res;
    return sizeof(StateHeader) + npx * (ER_PASS_COUNT * sizeof(float4) + 2 * sizeof(uint32_t));
}
}  // namespace

static int er_state_size_impl(ErScene* s, uint64_t* bytes) {
    if (!s || !bytes) return fail(ER_ERR_INVALID_ARG, "er_state_size: NULL argument");
    *bytes = state_bytes(s);
    return ER_OK;
}

static int er_state_export_impl(ErScene* s, void* dst, uint64_t bytes) {
    if (!s || !dst) return fail(ER_ERR_INVALID_ARG, "er_state_export: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_state_export: er_render_begin has not succeeded");
    if (bytes < state_bytes(s)) return fail(ER_ERR_INVALID_ARG, "er_state_export: buffer smaller than er_state_size");
    HIP_TRY(hipSetDevice(s->device));
    const size_t npx = (size_t)s->x_res * s->y_res;
    StateHeader h{};
    memcpy(h.magic, "ERSTATE2", 8);
    h.x_res = s->x_res; h.y_res = s->y_res; h.passes = ER_PASS_COUNT; h.bytes = state_bytes(s);
    uint8_t* p = (uint8_t*)dst;
    memcpy(p, &h, sizeof(h));
    p += sizeof(h);
    // ordered after everything enqueued so far (the pool streams join the scene's stream at the end of every call)
    HIP_TRY(hipMemcpyAsync(p, s->d_passes.p, npx * ER_PASS_COUNT * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
    p += npx * ER_PASS_COUNT * sizeof(float4);
    HIP_TRY(hipMemcpyAsync(p, s->d_samples.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    p += npx * sizeof(uint32_t);
    HIP_TRY(hipMemcpyAsync(p, s->d_rng.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return er_scene_stream_status(s, "er_state_export");     // never checkpoint planes the library itself calls incomplete
}

static int er_state_import_impl(ErScene* s, const void* src, uint64_t bytes) {
    if (!s || !src) return fail(ER_ERR_INVALID_ARG, "er_state_import: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_state_import: er_render_begin has not succeeded");
    if (s->ad_on) return fail(ER_ERR_STATE, "er_state_import: resuming an adaptive render is not supported (er_adaptive_set)");
    StateHeader h;
    if (bytes < sizeof(h)) return fail(ER_ERR_INVALID_ARG, "er_state_import: truncated snapshot");
    memcpy(&h, src, sizeof(h));
    if (memcmp(h.magic, "ERSTATE2", 8) != 0) return fail(ER_ERR_INVALID_ARG, "er_state_import: not a snapshot of this library version (bad magic)");
    if (h.x_res != s->x_res || h.y_res != s->y_res || h.passes != ER_PASS_COUNT)
        return fail(ER_ERR_INVALID_ARG, "er_state_import: the snapshot is of a " + std::to_string(h.x_res) + "x" + std::to_string(h.y_res) + " frame");
    if (h.bytes != state_bytes(s) || bytes < h.bytes) return fail(ER_ERR_INVALID_ARG, "er_state_import: truncated snapshot");
    HIP_TRY(hipSetDevice(s->device));
    const size_t npx = (size_t)s->x_res * s->y_res;
    const uint8_t* p = (const uint8_t*)src + sizeof(h);
    HIP_TRY(hipMemcpyAsync(s->d_passes.p, p, npx * ER_PASS_COUNT * sizeof(float4), hipMemcpyHostToDevice, s->stream));
    p += npx * ER_PASS_COUNT * sizeof(float4);
    HIP_TRY(hipMemcpyAsync(s->d_samples.p, p, npx * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    p += npx * sizeof(uint32_t);
    HIP_TRY(hipMemcpyAsync(s->d_rng.p, p, npx * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));      // the caller's buffer may go away
    s->history_invalidate();      // (the planes are another render's: er_history.hip)
    return er_variance_mark_imported(s);      // (and the variance starts over from them: er_variance.hip)
}

static int er_denoise_impl(ErScene* s, uint32_t levels, float colour_sigma) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_denoise: NULL scene");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_denoise: er_render_begin has not succeeded");
    // a sharded frame: only on the rank that BEAUTY and NORMAL were gathered to (er_gather_pass / er_unpack_owned of every
    // other rank) after the last sample; DenoiseManager of the reference likewise runs where the whole pass is (src/CommandManager.cpp:265-274)
    if (s->params.world > 1 && (s->unpacked[ER_PASS_BEAUTY].size() + 1 < s->params.world || s->unpacked[ER_PASS_NORMAL].size() + 1 < s->params.world))
        return fail(ER_ERR_STATE, "er_denoise: the frame is sharded over several ranks; gather BEAUTY and NORMAL to this rank first (er_gather_pass)");
    if (levels == 0) levels = 5;
    if (levels > 8) return fail(ER_ERR_INVALID_ARG, "er_denoise: at most 8 levels");
    if (!(colour_sigma >= 0)) return fail(ER_ERR_INVALID_ARG, "er_denoise: colour_sigma must be >= 0");
    if (colour_sigma == 0) colour_sigma = 1.0f;
    HIP_TRY(hipSetDevice(s->device));
    const size_t npx = (size_t)s->x_res * s->y_res;
    ScopedDevBuf<float4> tmp;
    int rc;
    if ((rc = upload(tmp, (const void*)nullptr, npx, s->stream)) != ER_OK) return rc;
    const float4* beauty = s->d_passes.p + er_pass_index(npx, ER_PASS_BEAUTY, 0);      // (interleaved passes: stride 4, er_device.h)
    const float4* normal = s->d_passes.p + er_pass_index(npx, ER_PASS_NORMAL, 0);
    float4* out = s->d_passes.p + er_pass_index(npx, ER_PASS_DENOISE, 0);
    // ping-pong so that the last level lands in the DENOISE plane
    const float4* src = beauty;
    for (uint32_t k = 0; k < levels; k++) {
        float4* dst = ((levels - 1 - k) & 1u) ? tmp.p : out;
        // the colour edge-stop tightens with the level, as the residual noise shrinks
        const float kc = 1.0f / (colour_sigma * colour_sigma) * (float)(1u << k);
        er_launch_atrous(src, src == beauty ? 4 : 1, normal, 4, dst, (int)s->x_res, (int)s->y_res, 1 << k, kc, s->stream);
        src = dst;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    return er_scene_stream_status(s, "er_denoise");
}

static int er_read_samples_impl(ErScene* s, uint32_t* dst) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_read_samples: NULL scene");
    return read_back(s, s->d_samples.p, dst, (size_t)s->x_res * s->y_res * 4, "er_read_samples");
}
static int er_read_rng_impl(ErScene* s, uint32_t* dst) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_read_rng: NULL scene");
    return read_back(s, s->d_rng.p, dst, (size_t)s->x_res * s->y_res * 4, "er_read_rng");
}

static int er_owned_count_impl(ErScene* s, uint32_t rank, uint64_t* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_owned_count: NULL argument");
    uint32_t world = s->begun ? s->params.world : 1;
    if (rank >= world) return fail(ER_ERR_INVALID_ARG, "er_owned_count: rank >= world");
    *out = (uint64_t)s->tiles_of(rank, world).size() * 64;
    return ER_OK;
}

static int er_pack_owned_impl(ErScene* s, int pass, void* dev_dst) {
    if (!s || !dev_dst) return fail(ER_ERR_INVALID_ARG, "er_pack_owned: NULL argument");
    if (pass < 0 || pass >= ER_PASS_COUNT) return fail(ER_ERR_INVALID_ARG, "er_pack_owned: pass out of range");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_pack_owned: er_render_begin has not succeeded");
    HIP_TRY(hipSetDevice(s->device));
    er_launch_pack(s->dev, s->d_owned.p, s->dev.owned_tile_count, pass, dev_dst, s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    return er_scene_stream_status(s, "er_pack_owned");
}

static int er_unpack_owned_impl(ErScene* s, int pass, uint32_t src_rank, const void* dev_src) {
    if (!s || !dev_src) return fail(ER_ERR_INVALID_ARG, "er_unpack_owned: NULL argument");
    if (pass < 0 || pass >= ER_PASS_COUNT) return fail(ER_ERR_INVALID_ARG, "er_unpack_owned: pass out of range");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_unpack_owned: er_render_begin has not succeeded");
    if (src_rank >= s->params.world) return fail(ER_ERR_INVALID_ARG, "er_unpack_owned: src_rank >= world");
    HIP_TRY(hipSetDevice(s->device));
    auto it = s->d_rank_tiles.find(src_rank);
    if (it == s->d_rank_tiles.end()) {
        std::vector<uint32_t> t = s->tiles_of(src_rank, s->params.world);
        ScopedDevBuf<uint32_t> b;
        int rc = upload(b, t.data(), t.size(), s->stream);
        if (rc != ER_OK) return rc;
        HIP_TRY(hipStreamSynchronize(s->stream));   // t goes out of scope
        it = s->d_rank_tiles.emplace(src_rank, DevBuf<uint32_t>(b)).first;
        b.p = nullptr;                               // now owned by the scene
    }
    er_launch_unpack(s->dev, it->second.p, (uint32_t)it->second.n, pass, dev_src, s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (src_rank != s->params.rank) s->unpacked[pass].insert(src_rank);
    return ER_OK;
}

static int er_get_counters_impl(ErScene* s, ErCounters* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_get_counters: NULL argument");
    DevCounters c;
    int rc = read_back(s, s->d_counters.p, &c, sizeof(c), "er_get_counters");
    if (rc != ER_OK) return rc;
    out->paths = c.paths; out->bounce_samples = c.bounce_samples; out->rays = c.rays; out->node_visits = c.node_visits;
    out->tri_tests = c.tri_tests; out->shaded_hits = c.shaded_hits; out->texel_fetches = c.texel_fetches;
    out->hdri_samples = c.hdri_samples;
    out->trace_wave_steps = c.trace_wave_steps; out->trace_busy_lanes = c.trace_busy_lanes;
    out->trace_node_lanes = c.trace_node_lanes; out->trace_tri_lanes = c.trace_tri_lanes;
    return ER_OK;
}

static int er_get_profile_impl(ErScene* s, ErProfile* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_get_profile: NULL argument");
    if (!s->begun) return fail(ER_ERR_STATE, "er_get_profile: er_render_begin has not succeeded");
    *out = s->profile;
    return ER_OK;
}

static int er_accel_info_impl(ErScene* s, ErAccelInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_accel_info: NULL argument");
    if (!s->begun) return fail(ER_ERR_STATE, "er_accel_info: er_render_begin has not succeeded");
    *out = s->accel;
    return ER_OK;
}


// ---- adaptive sampling (include/eleven_hip.h er_adaptive_set; the test and the compaction: er_adaptive.hip) ----
// The active tiles live on the device as a list in the layout of er_adaptive.h (two buffers: a test reads one and compacts the kept
// tiles into the other); the host keeps a copy, read back with the test's result in one copy, because the streaming schedule's deal
// is made on the host (stream_redeal, er_stream_host.cpp).  Pack, unpack, gather, denoise and er_samples_done keep working on the whole owned share (s->dev).

// After a change of the active list (the caller holds the mutex; the stream is idle): the descriptor the wavefront and megakernel
// schedules are launched with, and -- `redeal` -- the streaming schedule's deal and form for the new share, within the buffers
// er_render_begin allocated for the owned share (records, spill and pixel rings: a smaller share fits).
static int adaptive_apply_list(ErScene* s, bool redeal) {
    s->ad_dev = s->dev;
    s->ad_dev.owned_tiles = s->d_ad_list[s->ad_cur].p + ER_AD_LIST;
    s->ad_dev.owned_tile_count = (uint32_t)s->ad_active.size();
    s->ad_active_px = 0;
    for (uint32_t t : s->ad_active) s->ad_active_px += s->tile_pixels(t);
    if (!redeal || !(s->params.flags & ER_FLAG_STREAM) || s->ad_active.empty()) return ER_OK;
    return stream_redeal(s);
}

// The test at s->ad_next samples: error plane, compaction, one read-back of the new list (the host waits for it here).
static int adaptive_test(ErScene* s) {
    const uint32_t count = (uint32_t)s->ad_active.size(), next = s->ad_cur ^ 1u;
    er_launch_adaptive_test(s->dev, s->d_ad_list[s->ad_cur].p, count, s->d_ad_snap.p, s->ad_threshold, s->d_ad_err.p, s->d_ad_keep.p, s->d_ad_list[next].p, s->stream);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> out(ER_AD_LIST + (size_t)count);
    HIP_TRY(hipMemcpyAsync(out.data(), s->d_ad_list[next].p, out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    int rc = er_scene_stream_status(s, "er_render_samples");
    if (rc != ER_OK) return rc;
    const uint32_t kept = out[0];
    if (kept > count) return fail(ER_ERR_STATE, "er_render_samples: the adaptive test returned more tiles than it was given");
    s->ad_active.assign(out.begin() + ER_AD_LIST, out.begin() + ER_AD_LIST + kept);
    memcpy(&s->ad_max_error, &out[1], sizeof(float));
    s->ad_cur = next;
    s->ad_tests++;
    s->ad_next += s->ad_interval;
    s->ad_snapped = false;
    return adaptive_apply_list(s, kept != count);
}

// er_render_samples_async in adaptive mode: the n samples in chunks that end at every snapshot and test point, so that the test points
// depend on the parameters alone and never on how the caller splits its calls.  The caller holds the mutex.
static int adaptive_render(ErScene* s, uint32_t n) {
    while (n > 0 && !s->ad_active.empty()) {
        const uint32_t snap_at = s->ad_next - s->ad_interval;
        if (s->rendered == snap_at && !s->ad_snapped) {
            er_launch_adaptive_snapshot(s->dev, s->d_ad_list[s->ad_cur].p, (uint32_t)s->ad_active.size(), s->d_ad_snap.p, s->stream);
            HIP_TRY(hipGetLastError());
            s->ad_snapped = true;
        }
        const uint32_t stop = s->rendered < snap_at ? snap_at : s->ad_next;
        const uint32_t k = std::min(n, stop - s->rendered);
        int rc = enqueue_samples(s, k);
        if (rc != ER_OK) return rc;
        s->rendered += k;
        n -= k;
        s->ad_pixel_samples += (uint64_t)k * s->ad_active_px;
        for (uint32_t t : s->ad_active) s->ad_tile_samples[t] += k;
        if (s->rendered == s->ad_next && (rc = adaptive_test(s)) != ER_OK) return rc;
    }
    return ER_OK;
}

static int er_adaptive_set_impl(ErScene* s, const ErAdaptiveParams* p) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_adaptive_set: NULL scene");
    ErAdaptiveParams q{};
    if (p) {
        q = *p;
        if (!(q.threshold >= 0.0f)) return fail(ER_ERR_INVALID_ARG, "er_adaptive_set: threshold must be >= 0 (and not NaN)");
        if (q.min_samples == 0) q.min_samples = 16;
        if (q.interval == 0) q.interval = 8;
        if (q.interval >= q.min_samples) return fail(ER_ERR_INVALID_ARG, "er_adaptive_set: interval must be smaller than min_samples");
    }
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_adaptive_set: er_render_begin has not succeeded");
    if (s->rendered > 0) return fail(ER_ERR_STATE, "er_adaptive_set: only between er_render_begin and the first sample");
    if (!p) { s->ad_on = false; return ER_OK; }
    HIP_TRY(hipSetDevice(s->device));
    const std::vector<uint32_t> owned = s->tiles_of(s->params.rank, s->params.world);
    const size_t n_tiles = (size_t)s->dev.tiles_x * s->dev.tiles_y;
    std::vector<uint32_t> list(ER_AD_LIST + owned.size());
    const float none = -1.0f;
    list[0] = (uint32_t)owned.size();
    memcpy(&list[1], &none, sizeof(float));
    std::copy(owned.begin(), owned.end(), list.begin() + ER_AD_LIST);
    const std::vector<float> err(n_tiles, -1.0f);
    int rc;
    if ((rc = upload(s->d_ad_list[0], list.data(), list.size(), s->stream)) != ER_OK) return rc;
    if ((rc = upload(s->d_ad_list[1], nullptr, list.size(), s->stream)) != ER_OK) return rc;
    if ((rc = upload(s->d_ad_keep, nullptr, owned.size(), s->stream)) != ER_OK) return rc;
    if ((rc = upload(s->d_ad_snap, nullptr, owned.size() * 64, s->stream)) != ER_OK) return rc;
    if ((rc = upload(s->d_ad_err, err.data(), err.size(), s->stream)) != ER_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));      // (`list` and `err` go out of scope)
    s->ad_threshold = q.threshold;
    s->ad_interval = q.interval;
    s->ad_next = q.min_samples;
    s->ad_tests = 0;
    s->ad_cur = 0;
    s->ad_snapped = false;
    s->ad_max_error = -1.0f;
    s->ad_pixel_samples = 0;
    s->ad_active = owned;
    s->ad_tile_samples.assign(n_tiles, 0u);
    s->ad_on = true;
    return adaptive_apply_list(s, false);
}

static int er_light_info_impl(ErScene* s, ErLightInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_light_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_light_info: er_render_begin has not succeeded");
    *out = ErLightInfo{};
    out->emitters = s->light_emitters;
    out->total_weight = s->light_total;
    return ER_OK;
}

static int er_adaptive_info_impl(ErScene* s, ErAdaptiveInfo* out) {
    if (!s || !out) return fail(ER_ERR_INVALID_ARG, "er_adaptive_info: NULL argument");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_adaptive_info: er_render_begin has not succeeded");
    *out = ErAdaptiveInfo{};
    out->enabled = s->ad_on ? 1u : 0u;
    out->owned_tiles = s->dev.owned_tile_count;
    out->samples_rendered = s->rendered;
    out->max_active_error = -1.0f;
    if (s->ad_on) {
        out->active_tiles = (uint32_t)s->ad_active.size();
        out->tests_done = s->ad_tests;
        out->next_test = s->ad_next;
        out->pixel_samples = s->ad_pixel_samples;
        out->max_active_error = s->ad_max_error;
    } else {
        out->active_tiles = s->dev.owned_tile_count;
        out->pixel_samples = s->owned_pixels() * s->rendered;
    }
    return ER_OK;
}

static int er_read_tile_state_impl(ErScene* s, float* error, uint32_t* samples) {
    if (!s) return fail(ER_ERR_INVALID_ARG, "er_read_tile_state: NULL scene");
    std::lock_guard<std::mutex> lk(s->mtx);
    if (!s->begun) return fail(ER_ERR_STATE, "er_read_tile_state: er_render_begin has not succeeded");
    const size_t n_tiles = (size_t)s->dev.tiles_x * s->dev.tiles_y;
    if (samples) {
        if (s->ad_on) {
            std::copy(s->ad_tile_samples.begin(), s->ad_tile_samples.end(), samples);
        } else {
            std::fill(samples, samples + n_tiles, 0u);
            for (uint32_t t : s->tiles_of(s->params.rank, s->params.world)) samples[t] = s->rendered;
        }
    }
    if (error) {
        if (s->ad_on) return read_back_locked(s, s->d_ad_err.p, error, n_tiles * sizeof(float), "er_read_tile_state");
        std::fill(error, error + n_tiles, -1.0f);
    }
    return ER_OK;
}

// ---- the exported entry points: every body above runs inside guarded() (no exception crosses the C ABI) ----
extern "C" {
int er_device_info(int index, ErDeviceInfo* out) { return guarded("er_device_info", [&]() -> int { return er_device_info_impl(index, out); }); }
int er_device_find(const char* selector) { return guarded("er_device_find", [&]() -> int { return er_device_find_impl(selector); }); }
int er_scene_create(const ErSceneDesc* d, ErScene** out) { return guarded("er_scene_create", [&]() -> int { return er_scene_create_impl(d, out); }); }
int er_render_begin(ErScene* s, const ErRenderParams* p) { return guarded("er_render_begin", [&]() -> int { return er_render_begin_impl(s, p); }); }
int er_render_samples_async(ErScene* s, uint32_t n) { return guarded("er_render_samples_async", [&]() -> int { return er_render_samples_async_impl(s, n); }); }
int er_wait(ErScene* s, float* elapsed_ms) { return guarded("er_wait", [&]() -> int { return er_wait_impl(s, elapsed_ms); }); }
int er_render_samples(ErScene* s, uint32_t n) { return guarded("er_render_samples", [&]() -> int { return er_render_samples_impl(s, n); }); }
int er_samples_done(ErScene* s, uint32_t* out) { return guarded("er_samples_done", [&]() -> int { return er_samples_done_impl(s, out); }); }
int er_read_pass(ErScene* s, int pass, float* dst) { return guarded("er_read_pass", [&]() -> int { return er_read_pass_impl(s, pass, dst); }); }
int er_state_size(ErScene* s, uint64_t* bytes) { return guarded("er_state_size", [&]() -> int { return er_state_size_impl(s, bytes); }); }
int er_state_export(ErScene* s, void* dst, uint64_t bytes) { return guarded("er_state_export", [&]() -> int { return er_state_export_impl(s, dst, bytes); }); }
int er_state_import(ErScene* s, const void* src, uint64_t bytes) { return guarded("er_state_import", [&]() -> int { return er_state_import_impl(s, src, bytes); }); }
int er_denoise(ErScene* s, uint32_t levels, float colour_sigma) { return guarded("er_denoise", [&]() -> int { return er_denoise_impl(s, levels, colour_sigma); }); }
int er_read_samples(ErScene* s, uint32_t* dst) { return guarded("er_read_samples", [&]() -> int { return er_read_samples_impl(s, dst); }); }
int er_read_rng(ErScene* s, uint32_t* dst) { return guarded("er_read_rng", [&]() -> int { return er_read_rng_impl(s, dst); }); }
int er_owned_count(ErScene* s, uint32_t rank, uint64_t* out) { return guarded("er_owned_count", [&]() -> int { return er_owned_count_impl(s, rank, out); }); }
int er_pack_owned(ErScene* s, int pass, void* dev_dst) { return guarded("er_pack_owned", [&]() -> int { return er_pack_owned_impl(s, pass, dev_dst); }); }
int er_unpack_owned(ErScene* s, int pass, uint32_t src_rank, const void* dev_src) { return guarded("er_unpack_owned", [&]() -> int { return er_unpack_owned_impl(s, pass, src_rank, dev_src); }); }
int er_get_counters(ErScene* s, ErCounters* out) { return guarded("er_get_counters", [&]() -> int { return er_get_counters_impl(s, out); }); }
int er_get_profile(ErScene* s, ErProfile* out) { return guarded("er_get_profile", [&]() -> int { return er_get_profile_impl(s, out); }); }
int er_accel_info(ErScene* s, ErAccelInfo* out) { return guarded("er_accel_info", [&]() -> int { return er_accel_info_impl(s, out); }); }
int er_adaptive_set(ErScene* s, const ErAdaptiveParams* p) { return guarded("er_adaptive_set", [&]() -> int { return er_adaptive_set_impl(s, p); }); }
int er_adaptive_info(ErScene* s, ErAdaptiveInfo* out) { return guarded("er_adaptive_info", [&]() -> int { return er_adaptive_info_impl(s, out); }); }
int er_light_info(ErScene* s, ErLightInfo* out) { return guarded("er_light_info", [&]() -> int { return er_light_info_impl(s, out); }); }
int er_read_tile_state(ErScene* s, float* error, uint32_t* samples) { return guarded("er_read_tile_state", [&]() -> int { return er_read_tile_state_impl(s, error, samples); }); }
}  // extern "C"
