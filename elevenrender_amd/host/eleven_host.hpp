// eleven_host.hpp -- C++ host mirror of the reference's scene/render objects on top of the C ABI.
//
// The reference is a C++ program; this header gives a reference-shaped host API (same class and member
// names, same call order) whose device side is libeleven_hip.so instead of SYCL:
//
//   reference                                            here
//   Vector3 / Camera / Material / Texture / HDRI / Tri   same names, plain data (src/Vector.h, Camera.h:5-25,
//   MeshObject / PointLight / Scene                       Material.h:6-56, Texture.h:12-73, HDRI.h:9-42, Tri.h:8-21,
//                                                         MeshObject.hpp:14-22, Scene.h:24-73)
//   RenderParameters (src/kernel.h:51-69)                same fields (+ max_bounces, rank, world)
//   RenderingManager::start_rendering / get_pass /       same methods (src/Managers.h:41-66, Managers.cpp:211-302)
//     get_render_info
//
// Only what the per-sample path consumes is mirrored (OBJ ingest: eleven_obj.hpp beside this file; denoise(): the
// library's own filter in place of DenoiseManager's OIDN call); commands and TCP stay the reference's.  Errors surface as std::runtime_error carrying er_last_error(); nothing falls back to the CPU.
#pragma once
#include <mutex>
#include <thread>
#include <algorithm>
#include <cctype>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/eleven_hip.h"

namespace eleven {

struct Vector3 {
    float x = 0, y = 0, z = 0;
    Vector3() = default;
    Vector3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
    explicit Vector3(float v) : x(v), y(v), z(v) {}
};

struct Camera {   // defaults of src/Camera.h:9-19
    float focalLength = 35 * 0.001, sensorWidth = 36 * 0.001, sensorHeight = 24 * 0.001, aperture = 2.8, focusDistance = 1000000;
    Vector3 rotation;
    bool bokeh = false;
    Vector3 position;
};

struct Material {   // defaults of src/Material.h:20-47
    std::string name;
    int albedoTextureID = -1, emissionTextureID = -1, roughnessTextureID = -1, metallicTextureID = -1,
        normalTextureID = -1, opacityTextureID = -1, transmissionTextureID = -1, albedoShaderID = -1;
    Vector3 albedo{0.5f, 0.5f, 0.5f}, emission;
    float opacity = 1, roughness = 1, metallic = 0, clearcoatGloss = 0, clearcoat = 0, anisotropic = 0, eta = 0,
          transmission = 0, specular = 0.5, specularTint = 0, sheenTint = 0.5, subsurface = 0, sheen = 0, ax = 0, ay = 0;
    static Material DefaultMaterial() { Material m; m.name = "default"; return m; }
};

struct Texture {
    enum class Filter { NO_FILTER, BILINEAR };
    std::string name;
    int width = 1, height = 1;
    unsigned channels = 3;
    Filter filter = Filter::NO_FILTER;
    std::vector<float> data{0.5f, 0.5f, 0.5f};
    Texture() = default;
    explicit Texture(Vector3 c) : data{c.x, c.y, c.z} {}
    Texture(std::string n, int w, int h, int ch, std::vector<float> d, Filter f = Filter::NO_FILTER)
        : name(std::move(n)), width(w), height(h), channels((unsigned)ch), filter(f), data(std::move(d)) {}
};

struct HDRI {   // HDRI() = 1x1 texel (0.5,0.5,0.5), src/HDRI.cpp:18; the CDF is built by the library (src/HDRI.cpp:62-83)
    Texture texture{Vector3(0.5f)};
    HDRI() = default;
    explicit HDRI(Texture t) : texture(std::move(t)) {}
};

struct Tri {
    Vector3 vertices[3], uv[3], normals[3], tangents[3];
    float tangentsSign = 1;
    int objectID = 0, materialID = 0;
    std::string matName;
};

struct MeshObject {
    std::string name;
    std::vector<Tri> tris;
    int objectID = 0;
};

struct PointLight { Vector3 position, radiance; };

class Scene {
public:
    std::vector<Material> materials{Material::DefaultMaterial()};   // Scene() pushes the default material, src/Scene.h:45
    std::vector<MeshObject> meshObjects;
    std::vector<Texture> textures;
    std::vector<Tri> tris;
    std::vector<PointLight> pointLights;
    unsigned x_res = 1280, y_res = 720;
    HDRI hdri;
    Camera camera;

    void addPointLight(const PointLight& p) { pointLights.push_back(p); }
    void addTexture(const Texture& t) {   // by name, first one wins (src/Scene.cpp:44-51)
        for (const Texture& e : textures) if (e.name == t.name) return;
        textures.push_back(t);
    }
    void addMaterial(const Material& m) { materials.push_back(m); }
    void addMeshObject(MeshObject m) {     // src/Scene.cpp:54-71
        m.objectID = (int)meshObjects.size();
        for (Tri& t : m.tris) { t.objectID = m.objectID; tris.push_back(t); }
        meshObjects.push_back(std::move(m));
    }
    void addHDRI(const HDRI& h) { hdri = h; }
    void pair_materials() {                // src/Scene.cpp:104-120: materialID by name, 0 if none
        for (Tri& t : tris) {
            t.materialID = 0;
            for (size_t j = 0; j < materials.size(); j++) if (materials[j].name == t.matName) t.materialID = (int)j;
        }
    }
};

struct RenderParameters {   // src/kernel.h:51-69
    unsigned width = 1280, height = 720, sampleTarget = 100, block_size = 8;
    std::string device;     // "name|platform" (src/Managers.cpp:201); empty = device 0
    bool denoise = false;
    unsigned max_bounces = 5, rank = 0, world = 1, flags = 0;
    // Several GPUs of this node driven by this one process (north_star: pixel tiles shard over the GPUs of a node, one combine
    // per read-back): `gpus` ranks, rank r on devices[r] (default: ordinals 0 .. gpus-1 after `device`; an ordinal may repeat --
    // several ranks on one GPU, which is how a one-GPU box tests this path).  transport: "rccl" (ncclSend/ncclRecv over xGMI),
    // "local" (in-process peer copies) or "auto" = rccl when every rank has its own device and RCCL loads, else local.
    unsigned gpus = 1;
    std::vector<int> devices;
    std::string transport = "auto";
    // adaptive sampling (extension, off by default): applied to every rank after er_render_begin (er_adaptive_set)
    bool adaptive = false;
    ErAdaptiveParams adaptive_params{};
    // the denoise guided by first-hit albedo and depth (extension, off by default): `denoise: true` / get_pass denoise then run
    // er_denoise_guided on feature planes of feature_samples camera rays per pixel (0 = the library's default, 4)
    bool denoise_guided = false;
    unsigned feature_samples = 0;
    // the first-hit passes see through cut-outs (extension, off by default): applied to every rank after er_render_begin
    // (er_first_hit_set; the library keeps it through every edit in place); cutout_threshold 0 = the library's default, 0.5
    bool cutouts = false;
    float cutout_threshold = 0;
    // temporal reprojection (extension, off by default): a --start answered by the camera-update path captures the frame before the
    // update and resolves it after (er_history_capture / er_history_resolve); --get_pass blended then answers er_read_blended.  One GPU.
    bool history = false;
    // the variance plane and the denoise guided by it (extension, off by default): the render thread cuts its calls at multiples of
    // variance_batch samples (0 = 2) and folds there (er_variance_fold), so the plane depends on the parameters and not on how the thread
    // sized its calls; `denoise: true` / get_pass denoise then run er_denoise_variance once two folds exist (before that: the guided
    // filter), and get_pass variance answers er_read_variance.  One GPU.
    bool denoise_variance = false;
    unsigned variance_batch = 0;
    unsigned fold_every() const { return denoise_variance ? (variance_batch ? variance_batch : 2u) : 0u; }
    // with `history` and `denoise_variance`: `denoise: true` / get_pass denoise answer er_denoise_blended -- the blended frame filtered by
    // its own variance, which the history carried across the camera update -- whenever a resolved history exists
    bool denoise_blended = false;
};

// What a session sent since its last successful --start.  A --start after nothing but --load_camera restarts the render in place
// (RenderingManager::update_camera: er_render_update on every rank -- no build, no uploads); after nothing but --load_camera,
// --load_hdri, --load_brdf_material and --load_texture it edits the begun scenes in place (RenderingManager::edit_scene:
// er_render_edit on every rank -- no build; the texture pool is rebuilt on the device only if an assignment or a texture changed);
// after object loads beside those (--load_object appends triangles and never touches the ones there are) it changes the begun scenes'
// topology in place (RenderingManager::append_scene: er_render_topology on every rank -- the appended triangles, the complete material
// and texture lists in its `rest`; the one build this edit needs, nothing else of a start); after anything else (--load_config), or before
// the first render, it is the full start_rendering.
struct SessionEdits {
    bool rendering = false;      // a --start has succeeded and its scenes are alive
    bool camera = false;         // --load_camera arrived since
    bool hdri = false;           // ... --load_hdri
    bool materials = false;      // ... --load_brdf_material or --load_texture
    bool objects = false;        // ... --load_object
    bool other = false;          // ... and anything else that changes the scene or the parameters
    void on_camera() { camera = true; }
    void on_hdri() { hdri = true; }
    void on_materials() { materials = true; }
    void on_object() { objects = true; }
    void on_other() { other = true; }
    void on_started() { rendering = true; camera = hdri = materials = objects = other = false; }
    void on_failed() { rendering = false; }
    bool camera_only() const { return rendering && !other && !objects && !hdri && !materials; }      // (no edit at all: the same render again, also without a rebuild)
    bool editable() const { return rendering && !other && !objects && (hdri || materials); }         // (a camera may have come as well)
    bool appendable() const { return rendering && !other && objects; }                               // (and so may an HDRI, materials and textures)
};

inline int parseFeature(std::string s) {   // the feature planes of er_render_features by name, -1 = not one
    std::transform(s.begin(), s.end(), s.begin(), [](unsigned char c) { return (char)std::tolower(c); });
    if (s == "albedo") return ER_FEATURE_ALBEDO;
    if (s == "depth") return ER_FEATURE_DEPTH;
    return -1;
}

inline int parsePass(std::string s) {   // src/kernel.cpp:50-73: unknown names -> BEAUTY
    std::transform(s.begin(), s.end(), s.begin(), [](unsigned char c) { return (char)std::tolower(c); });
    if (s == "denoise") return ER_PASS_DENOISE;
    if (s == "normal") return ER_PASS_NORMAL;
    if (s == "tangent") return ER_PASS_TANGENT;
    if (s == "bitangent") return ER_PASS_BITANGENT;
    return ER_PASS_BEAUTY;
}

class RenderingManager {
public:
    struct RenderInfo { unsigned samples = 0; };
    RenderParameters pars;
    std::string transport_used;      // "" (one GPU), "rccl" or "in-process"

    ~RenderingManager() { release(); }

    static std::vector<ErMaterial> er_materials(const Scene& scene) {      // the scene's materials as the library takes them
        std::vector<ErMaterial> ms;
        for (const Material& m : scene.materials) {
            ErMaterial e{};
            e.albedo_tex = m.albedoTextureID; e.emission_tex = m.emissionTextureID; e.roughness_tex = m.roughnessTextureID;
            e.metallic_tex = m.metallicTextureID; e.normal_tex = m.normalTextureID; e.opacity_tex = m.opacityTextureID;
            e.transmission_tex = m.transmissionTextureID; e.albedo_shader_id = m.albedoShaderID;
            e.albedo = {m.albedo.x, m.albedo.y, m.albedo.z}; e.emission = {m.emission.x, m.emission.y, m.emission.z};
            e.opacity = m.opacity; e.roughness = m.roughness; e.metallic = m.metallic; e.clearcoat_gloss = m.clearcoatGloss;
            e.clearcoat = m.clearcoat; e.anisotropic = m.anisotropic; e.eta = m.eta; e.transmission = m.transmission;
            e.specular = m.specular; e.specular_tint = m.specularTint; e.sheen_tint = m.sheenTint; e.subsurface = m.subsurface;
            e.sheen = m.sheen; e.ax = m.ax; e.ay = m.ay;
            ms.push_back(e);
        }
        return ms;
    }
    static ErTexture er_texture(const Texture& t) {
        return ErTexture{t.width, t.height, (int32_t)t.channels, t.filter == Texture::Filter::BILINEAR ? 1 : 0, t.data.data()};
    }

    // the scene's triangles [from, to) as the library's six flat arrays
    struct TriArrays {
        std::vector<float> v, nn, tt, uv, sign;
        std::vector<int32_t> mat;
    };
    static TriArrays tri_arrays(const Scene& scene, size_t from, size_t to) {
        const size_t n = to - from;
        TriArrays A;
        A.v.resize(n * 9); A.nn.resize(n * 9); A.tt.resize(n * 9); A.uv.resize(n * 6); A.sign.resize(n); A.mat.resize(n);
        for (size_t i = 0; i < n; i++) {
            const Tri& t = scene.tris[from + i];
            for (int k = 0; k < 3; k++) {
                const Vector3* src[3] = {&t.vertices[k], &t.normals[k], &t.tangents[k]};
                float* dst[3] = {&A.v[i * 9 + k * 3], &A.nn[i * 9 + k * 3], &A.tt[i * 9 + k * 3]};
                for (int a = 0; a < 3; a++) { dst[a][0] = src[a]->x; dst[a][1] = src[a]->y; dst[a][2] = src[a]->z; }
                A.uv[i * 6 + k * 2] = t.uv[k].x;
                A.uv[i * 6 + k * 2 + 1] = t.uv[k].y;
            }
            A.sign[i] = t.tangentsSign;
            A.mat[i] = t.materialID;
        }
        return A;
    }

    void start_rendering(Scene* scene) {   // src/Managers.cpp:234-275 (without spawning the render thread)
        release();
        size_t n = scene->tris.size();
        TriArrays A = tri_arrays(*scene, 0, n);
        std::vector<float>&v = A.v, &nn = A.nn, &tt = A.tt, &uv = A.uv, &sign = A.sign;
        std::vector<int32_t>& mat = A.mat;
        const std::vector<ErMaterial> ms = er_materials(*scene);
        std::vector<ErTexture> ts;
        for (const Texture& t : scene->textures)
            ts.push_back(ErTexture{t.width, t.height, (int32_t)t.channels, t.filter == Texture::Filter::BILINEAR ? 1 : 0, t.data.data()});
        ErSceneDesc d{};
        d.tri_count = (uint32_t)n;
        d.vertices = v.data(); d.normals = nn.data(); d.tangents = tt.data(); d.uvs = uv.data();
        d.tangent_sign = sign.data(); d.material_id = mat.data();
        d.material_count = (uint32_t)ms.size(); d.materials = ms.data();
        d.texture_count = (uint32_t)ts.size(); d.textures = ts.data();
        const Texture& ht = scene->hdri.texture;
        d.hdri.texture = ErTexture{ht.width, ht.height, (int32_t)ht.channels, ht.filter == Texture::Filter::BILINEAR ? 1 : 0, ht.data.data()};
        const Camera& c = scene->camera;
        d.camera = ErCamera{c.focalLength, c.sensorWidth, c.sensorHeight, c.aperture, c.focusDistance,
                            {c.rotation.x, c.rotation.y, c.rotation.z}, c.bokeh ? 1 : 0, {c.position.x, c.position.y, c.position.z}};
        std::vector<ErPointLight> pls;      // evaluated only with ER_FLAG_POINT_LIGHTS (src/PointLight.h:4-16; no reference command loads one)
        for (const PointLight& p : scene->pointLights) pls.push_back(ErPointLight{{p.position.x, p.position.y, p.position.z}, {p.radiance.x, p.radiance.y, p.radiance.z}});
        d.point_light_count = (uint32_t)pls.size(); d.point_lights = pls.empty() ? nullptr : pls.data();
        d.x_res = scene->x_res; d.y_res = scene->y_res;
        pars.width = scene->x_res; pars.height = scene->y_res;
        if (er_abi_version() != ER_ABI_VERSION)      // the library fills caller-allocated structs completely: never run against another layout
            throw std::runtime_error("libeleven_hip.so has ABI version " + std::to_string(er_abi_version()) + ", this host was built for " + std::to_string(ER_ABI_VERSION));

        // ---- which ranks on which devices ----
        const bool multi = pars.gpus > 1;
        const unsigned world = multi ? pars.gpus : pars.world;
        if (world == 0 || world > 64) throw std::runtime_error("config gpus out of range (1 .. 64)");
        int first = 0;
        if (!pars.device.empty()) { first = er_device_find(pars.device.c_str()); check(first < 0 ? first : ER_OK); }
        std::vector<int> devs;
        if (multi) {
            devs = pars.devices;
            if (devs.empty()) {
                const int have = er_device_count();
                if (have <= 0) check(ER_ERR_NO_DEVICE, "no gfx950 device is visible");
                if ((int)world > have)
                    throw std::runtime_error("config asks for " + std::to_string(world) + " gpus, " + std::to_string(have) + " visible (name the ordinals in \"devices\" to put several ranks on one GPU)");
                for (unsigned r = 0; r < world; r++) devs.push_back((first + (int)r) % have);
            }
            if (devs.size() != world) throw std::runtime_error("config devices must list one ordinal per gpu");
        }
        // ---- one scene per rank (the scene is replicated, the pixel tiles are dealt (tx + ty) % world); begun side by side ----
        const unsigned ranks = multi ? world : 1;
        ers_.assign(ranks, nullptr);
        std::vector<std::string> errs(ranks);
        std::vector<std::thread> th;
        for (unsigned r = 0; r < ranks; r++)
            th.emplace_back([&, r] {
                ErRenderParams p{};
                p.sample_target = pars.sampleTarget; p.block_size = pars.block_size; p.max_bounces = pars.max_bounces;
                p.rank = multi ? r : pars.rank; p.world = world; p.flags = pars.flags;
                p.device = multi ? devs[r] : first;
                int rc = er_scene_create(&d, &ers_[r]);
                if (rc == ER_OK) rc = er_render_begin(ers_[r], &p);
                if (rc != ER_OK) errs[r] = er_last_error();
            });
        for (auto& t : th) t.join();
        for (unsigned r = 0; r < ranks; r++) if (!errs[r].empty()) { std::string e = errs[r]; release(); throw std::runtime_error(e); }
        textures_sent_ = scene->textures.size();
        mats_sent_ = mat;
        if (pars.adaptive)
            for (ErScene* e : ers_) if (er_adaptive_set(e, &pars.adaptive_params) != ER_OK) { std::string m = er_last_error(); release(); throw std::runtime_error(m); }
        if (pars.cutouts) {
            const ErFirstHitParams fh{1u, pars.cutout_threshold};
            for (ErScene* e : ers_) if (er_first_hit_set(e, &fh) != ER_OK) { std::string m = er_last_error(); release(); throw std::runtime_error(m); }
        }
        // ---- the combine's communicators ----
        if (multi) {
            bool distinct = true;
            for (unsigned a = 0; a < world; a++) for (unsigned b = a + 1; b < world; b++) if (devs[a] == devs[b]) distinct = false;
            std::string tr = pars.transport;
            if (tr != "auto" && tr != "rccl" && tr != "local") throw std::runtime_error("config transport '" + tr + "' not recognised");
            comms_.assign(world, nullptr);
            if (tr == "rccl" && !distinct) { release(); throw std::runtime_error("transport rccl needs one device per rank"); }
            if (tr != "local" && distinct) {
                uint8_t id[ER_COMM_ID_BYTES];
                int rc = er_comm_unique_id(id);
                if (rc == ER_OK) {
                    std::vector<int> rcs(world, ER_OK);
                    std::vector<std::thread> ct;        // ncclCommInitRank blocks until every rank has joined: one thread per rank
                    for (unsigned r = 0; r < world; r++) ct.emplace_back([&, r] { rcs[r] = er_comm_create(id, r, world, devs[r], &comms_[r]); if (rcs[r] != ER_OK) errs[r] = er_last_error(); });
                    for (auto& t : ct) t.join();
                    for (unsigned r = 0; r < world; r++) if (rcs[r] != ER_OK) rc = rcs[r];
                }
                if (rc == ER_OK) transport_used = "rccl";
                else if (tr == "rccl") { std::string e = er_last_error(); for (auto& x : errs) if (!x.empty()) e = x; release(); throw std::runtime_error(e); }
                else for (auto*& cm : comms_) { if (cm) er_comm_destroy(cm); cm = nullptr; }
            }
            if (transport_used.empty()) {
                check(er_comm_create_local(world, comms_.data()));
                transport_used = "in-process";
            }
        }
    }
    // A --start after nothing but --load_camera: er_render_update(ER_UPDATE_CAMERA) on every rank side by side, then what
    // start_rendering does after er_render_begin (the update turns adaptive sampling off, as a begin does).  The communicators stay.
    // Returns false -- the ranks are then no longer begun, the caller starts over with start_rendering -- if any rank's update failed.
    bool update_camera(const Camera& c) {
        if (ers_.empty()) return false;
        ErSceneUpdate u{};
        u.what = ER_UPDATE_CAMERA;
        u.camera = ErCamera{c.focalLength, c.sensorWidth, c.sensorHeight, c.aperture, c.focusDistance,
                            {c.rotation.x, c.rotation.y, c.rotation.z}, c.bokeh ? 1 : 0, {c.position.x, c.position.y, c.position.z}};
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        // `history`: the frame as it is goes into a capture first (a refused capture only means this restart carries nothing over)
        const ErHistoryParams hp{0.0f, 0.0f};
        const bool captured = pars.history && ers_.size() == 1 && er_history_capture(ers_[0], &hp) == ER_OK;
        std::vector<int> rcs(ers_.size(), ER_OK);
        std::vector<std::thread> th;
        for (size_t r = 0; r < ers_.size(); r++) th.emplace_back([&, r] { rcs[r] = er_render_update(ers_[r], &u); });
        for (auto& t : th) t.join();
        features_ready_ = false;      // (the library has invalidated the planes)
        for (int rc : rcs) if (rc != ER_OK) return false;
        if (captured && er_history_resolve(ers_[0]) == ER_OK) history_resolves++;
        if (pars.adaptive)
            for (ErScene* e : ers_) if (er_adaptive_set(e, &pars.adaptive_params) != ER_OK) return false;
        return true;
    }
    // A --start after nothing but --load_camera, --load_hdri, --load_brdf_material and --load_texture: er_render_edit on every rank
    // side by side.  What goes over: the camera; the COMPLETE material list and the triangles' material ids as pair_materials left
    // them (a material sent again under its name is appended, and pair_materials takes the last match: the ids move to the new
    // entry); the texture list with data = NULL for the textures the ranks already have (addTexture never replaces one: the first of
    // a name wins); the HDRI if one came.  Returns false -- the caller starts over with start_rendering -- if any rank refused or
    // failed.
    bool edit_scene(Scene* scene, bool hdri) {
        if (ers_.empty() || scene->materials.empty() || scene->textures.size() < textures_sent_ || scene->tris.size() != mats_sent_.size()) return false;
        const std::vector<ErMaterial> ms = er_materials(*scene);
        std::vector<int32_t> mat(scene->tris.size());
        for (size_t i = 0; i < mat.size(); i++) mat[i] = scene->tris[i].materialID;
        std::vector<ErTexture> ts;
        for (size_t i = 0; i < scene->textures.size(); i++) {
            ts.push_back(er_texture(scene->textures[i]));
            if (i < textures_sent_) ts.back().data = nullptr;      // (keep)
        }
        const Camera& c = scene->camera;
        ErSceneEdit e{};
        e.what = ER_EDIT_CAMERA | ER_EDIT_MATERIALS | ER_EDIT_TEXTURES | (hdri ? ER_EDIT_HDRI : 0u);
        e.camera = ErCamera{c.focalLength, c.sensorWidth, c.sensorHeight, c.aperture, c.focusDistance,
                            {c.rotation.x, c.rotation.y, c.rotation.z}, c.bokeh ? 1 : 0, {c.position.x, c.position.y, c.position.z}};
        e.material_count = (uint32_t)ms.size(); e.materials = ms.data();
        e.material_id = mat.data();
        e.texture_count = (uint32_t)ts.size(); e.textures = ts.data();
        if (hdri) e.hdri.texture = er_texture(scene->hdri.texture);
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        std::vector<int> rcs(ers_.size(), ER_OK);
        std::vector<std::thread> th;
        for (size_t r = 0; r < ers_.size(); r++) th.emplace_back([&, r] { rcs[r] = er_render_edit(ers_[r], &e); });
        for (auto& t : th) t.join();
        features_ready_ = false;      // (the library has invalidated the planes)
        for (int rc : rcs) if (rc != ER_OK) return false;
        textures_sent_ = scene->textures.size();
        mats_sent_ = mat;
        if (pars.adaptive)
            for (ErScene* s : ers_) if (er_adaptive_set(s, &pars.adaptive_params) != ER_OK) return false;
        return true;
    }
    // A --start after object loads (and perhaps a camera, an HDRI, materials, textures): er_render_topology on every rank side by side.
    // addMeshObject only ever appends, so the triangles beyond the ranks' count are the edit; the COMPLETE material and texture lists go
    // through `rest` as in edit_scene, and the triangles' material ids only if pair_materials moved one of the triangles the ranks
    // already hold (the ranks' device-resident geometry then stays valid for the next such start).  Returns false -- the caller starts
    // over with start_rendering -- if nothing was appended or any rank refused or failed.
    bool append_scene(Scene* scene, bool hdri) {
        const size_t have = mats_sent_.size(), n = scene->tris.size();
        if (ers_.empty() || scene->materials.empty() || scene->textures.size() < textures_sent_ || n <= have) return false;
        const TriArrays A = tri_arrays(*scene, have, n);
        const std::vector<ErMaterial> ms = er_materials(*scene);
        std::vector<int32_t> mat(n);
        for (size_t i = 0; i < n; i++) mat[i] = scene->tris[i].materialID;
        const bool ids_moved = !std::equal(mats_sent_.begin(), mats_sent_.end(), mat.begin());
        std::vector<ErTexture> ts;
        for (size_t i = 0; i < scene->textures.size(); i++) {
            ts.push_back(er_texture(scene->textures[i]));
            if (i < textures_sent_) ts.back().data = nullptr;      // (keep)
        }
        const Camera& c = scene->camera;
        ErTopologyEdit t{};
        t.what = ER_TOPO_APPEND;
        t.append_count = (uint32_t)(n - have);
        t.vertices = A.v.data(); t.normals = A.nn.data(); t.tangents = A.tt.data(); t.uvs = A.uv.data(); t.tangent_sign = A.sign.data(); t.material_id = A.mat.data();
        ErSceneEdit& e = t.rest;
        e.what = ER_EDIT_CAMERA | ER_EDIT_MATERIALS | ER_EDIT_TEXTURES | (hdri ? ER_EDIT_HDRI : 0u);
        e.camera = ErCamera{c.focalLength, c.sensorWidth, c.sensorHeight, c.aperture, c.focusDistance,
                            {c.rotation.x, c.rotation.y, c.rotation.z}, c.bokeh ? 1 : 0, {c.position.x, c.position.y, c.position.z}};
        e.material_count = (uint32_t)ms.size(); e.materials = ms.data();
        e.material_id = ids_moved ? mat.data() : nullptr;
        e.texture_count = (uint32_t)ts.size(); e.textures = ts.data();
        if (hdri) e.hdri.texture = er_texture(scene->hdri.texture);
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        std::vector<int> rcs(ers_.size(), ER_OK);
        std::vector<std::thread> th;
        for (size_t r = 0; r < ers_.size(); r++) th.emplace_back([&, r] { rcs[r] = er_render_topology(ers_[r], &t); });
        for (auto& x : th) x.join();
        features_ready_ = false;      // (the library has invalidated the planes)
        for (int rc : rcs) if (rc != ER_OK) return false;
        textures_sent_ = scene->textures.size();
        mats_sent_ = mat;
        if (pars.adaptive)
            for (ErScene* s : ers_) if (er_adaptive_set(s, &pars.adaptive_params) != ER_OK) return false;
        return true;
    }
    // Object transforms (er_objects_set / er_render_transform; no wire command names an object, so these are for hosts that link this
    // mirror).  set_objects: the same table on every rank -- object o = tri_ids[first[o] .. first[o + 1]), the rest pose is what the ranks
    // hold now.  transform_objects: the listed objects posed by their 3x4 matrices on every rank side by side, then what
    // start_rendering does after er_render_begin, as update_camera.  Both return false if any rank refused or failed (after a failed
    // transform the caller starts over with start_rendering, as after a failed update_camera).
    bool set_objects(const std::vector<uint32_t>& first, const std::vector<uint32_t>& tri_ids) {
        if (ers_.empty()) return false;
        const uint32_t objects = first.empty() ? 0u : (uint32_t)first.size() - 1u;
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        std::vector<int> rcs(ers_.size(), ER_OK);
        std::vector<std::thread> th;
        for (size_t r = 0; r < ers_.size(); r++) th.emplace_back([&, r] { rcs[r] = er_objects_set(ers_[r], objects, first.data(), tri_ids.data()); });
        for (auto& t : th) t.join();
        for (int rc : rcs) if (rc != ER_OK) return false;
        return true;
    }
    bool transform_objects(const std::vector<ErObjectTransform>& poses) {
        if (ers_.empty() || poses.empty()) return false;
        ErTransformUpdate u{};
        u.what = ER_UPDATE_GEOMETRY;
        u.count = (uint32_t)poses.size();
        u.transforms = poses.data();
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        std::vector<int> rcs(ers_.size(), ER_OK);
        std::vector<std::thread> th;
        for (size_t r = 0; r < ers_.size(); r++) th.emplace_back([&, r] { rcs[r] = er_render_transform(ers_[r], &u); });
        for (auto& t : th) t.join();
        features_ready_ = false;      // (the library has invalidated the planes)
        for (int rc : rcs) if (rc != ER_OK) return false;
        if (pars.adaptive)
            for (ErScene* e : ers_) if (er_adaptive_set(e, &pars.adaptive_params) != ER_OK) return false;
        return true;
    }
    // body of kernel_render_enqueue's loop: n more samples on every rank (the launches go out side by side, then the waits).
    // With several ranks a read-back is a SEQUENCE of library calls (gathers, denoise, read) that must see one frame: if the
    // render thread enqueued samples on rank 0 between the gathers and er_denoise, the library would refuse the denoise
    // (its gathered planes are stale, ER_ERR_STATE) and the tiles of a preview would mix sample counts.  frame_mtx_
    // makes render() and such a sequence take turns; the render thread sizes its calls to about 50 ms, so a read-back waits
    // that long at most.  One rank needs none of this: er_read_pass is a sample-boundary snapshot by itself.
    void render(unsigned n_samples) {
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        std::string err;
        for (ErScene* e : ers_) if (er_render_samples_async(e, n_samples) != ER_OK && err.empty()) err = er_last_error();
        for (ErScene* e : ers_) if (er_wait(e, nullptr) != ER_OK && err.empty()) err = er_last_error();
        if (!err.empty()) throw std::runtime_error(err);
    }
    // er_read_blended: the reprojected history and the current BEAUTY combined (`history`; throws until a camera update has resolved one)
    std::vector<float> get_blended() {
        if (ers_.empty()) throw std::runtime_error("get_blended: no render has been started");
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        std::vector<float> out((size_t)pars.width * pars.height * 4);
        check(er_read_blended(ers_[0], out.data()));
        return out;
    }
    unsigned history_resolves = 0;      // camera updates whose frame was carried over (reported by --get_info)
    // er_variance_fold / er_variance_info / er_read_variance (`denoise_variance`; one GPU: a sharded frame has no variance plane)
    void variance_fold() {
        if (ers_.empty()) throw std::runtime_error("variance_fold: no render has been started");
        check(er_variance_fold(ers_[0]));
    }
    unsigned variance_folds() {
        ErVarianceInfo i{};
        if (ers_.empty() || er_variance_info(ers_[0], &i) != ER_OK) return 0;
        return i.folds;
    }
    std::vector<float> get_variance() {
        if (ers_.empty()) throw std::runtime_error("get_variance: no render has been started");
        std::vector<float> out((size_t)pars.width * pars.height * 4);
        check(er_read_variance(ers_[0], out.data()));
        return out;
    }
    // features if there are none yet + er_denoise_variance + read of the DENOISE plane; until two folds exist (ER_ERR_STATE) the guided
    // filter answers instead
    std::vector<float> get_denoised_variance(unsigned feature_samples = 0, unsigned levels = 0, float colour_sigma = 0, float albedo_sigma = 0, float depth_sigma = 0) {
        if (ers_.empty()) throw std::runtime_error("denoise_variance: no render has been started");
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        if (!features_ready_) render_features_unlocked(feature_samples);
        const ErDenoiseVariance p{levels, colour_sigma, albedo_sigma, depth_sigma};
        const int rc = ers_.size() == 1 ? er_denoise_variance(ers_[0], &p) : ER_ERR_STATE;
        if (rc == ER_ERR_STATE) denoise_guided_unlocked(levels, 0.0f, albedo_sigma, depth_sigma);      // (its own colour_sigma: another unit)
        else check(rc);
        return get_pass_unlocked(ER_PASS_DENOISE);
    }
    // features if there are none yet + er_denoise_blended + read of the DENOISE plane (`denoise_blended`); false, and nothing done, while
    // no resolved history exists: the caller answers as it does without the key
    bool get_denoised_blended(std::vector<float>& out, unsigned feature_samples = 0, unsigned levels = 0, float colour_sigma = 0, float albedo_sigma = 0, float depth_sigma = 0) {
        if (ers_.size() != 1) return false;
        ErHistoryInfo hi{};
        if (er_history_info(ers_[0], &hi) != ER_OK || !hi.resolved) return false;
        if (!features_ready_) render_features_unlocked(feature_samples);
        const ErDenoiseVariance p{levels, colour_sigma, albedo_sigma, depth_sigma};
        check(er_denoise_blended(ers_[0], &p));
        out = get_pass_unlocked(ER_PASS_DENOISE);
        blended_denoises++;
        return true;
    }
    unsigned blended_denoises = 0;      // answers er_denoise_blended gave (reported by --get_info)
    std::vector<float> get_pass(const std::string& pass) {   // src/Managers.cpp:287-302
        if (ers_.empty()) throw std::runtime_error("get_pass: no render has been started");
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        return get_pass_unlocked(parsePass(pass));
    }
    // DenoiseManager::denoise (src/Managers.cpp:319-343) called OIDN on the host; here the device fills the DENOISE plane --
    // on a sharded frame on rank 0, after BEAUTY and NORMAL have been gathered there
    void denoise(unsigned levels = 0, float colour_sigma = 0) {
        if (ers_.empty()) throw std::runtime_error("denoise: no render has been started");
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        denoise_unlocked(levels, colour_sigma);
    }
    // denoise + read of the DENOISE plane as ONE step against the render thread (get_pass denoise / `denoise: true`)
    std::vector<float> get_denoised(unsigned levels = 0, float colour_sigma = 0) {
        if (ers_.empty()) throw std::runtime_error("denoise: no render has been started");
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        denoise_unlocked(levels, colour_sigma);
        return get_pass_unlocked(ER_PASS_DENOISE);
    }
    // The feature pass (er_render_features) on every rank side by side, then both planes gathered to rank 0.  The planes depend on the
    // scene and the camera alone, not on the samples: once per start_rendering / update_camera is enough.
    void render_features(unsigned n = 0) {
        if (ers_.empty()) throw std::runtime_error("render_features: no render has been started");
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        render_features_unlocked(n);
    }
    // ... and lazily: only if no pass has run since the last start_rendering / update_camera (get_pass albedo / depth, `denoise_guided`)
    void ensure_features(unsigned n = 0) {
        if (ers_.empty()) throw std::runtime_error("render_features: no render has been started");
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        if (!features_ready_) render_features_unlocked(n);
    }
    std::vector<float> get_feature(const std::string& name) {      // "albedo" | "depth"; render_features first
        if (ers_.empty()) throw std::runtime_error("get_feature: no render has been started");
        const int f = parseFeature(name);
        if (f < 0) throw std::runtime_error("get_feature: '" + name + "' is not a feature plane (albedo, depth)");
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        std::vector<float> out((size_t)pars.width * pars.height * 4);
        check(er_read_feature(ers_[0], f, out.data()));
        return out;
    }
    ErFeatureInfo feature_info() {      // over the ranks: rays summed, the slowest rank's time
        ErFeatureInfo sum{};
        sum.valid = ers_.empty() ? 0u : 1u;
        for (ErScene* e : ers_) {
            ErFeatureInfo i{};
            check(er_feature_info(e, &i));
            sum.valid = sum.valid && i.valid ? 1u : 0u;
            sum.samples = i.samples;
            sum.rays += i.rays;
            sum.ms = std::max(sum.ms, i.ms);
        }
        return sum;
    }
    // er_first_hit_set on every rank of a begun render (a change invalidates the feature planes: the next ensure_features runs a pass)
    void set_first_hit(bool cutouts = true, float opacity_threshold = 0) {
        if (ers_.empty()) throw std::runtime_error("set_first_hit: no render has been started");
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        const ErFirstHitParams p{cutouts ? 1u : 0u, opacity_threshold};
        for (ErScene* e : ers_) check(er_first_hit_set(e, &p));
        pars.cutouts = cutouts;
        pars.cutout_threshold = opacity_threshold;
        features_ready_ = false;
    }
    ErFirstHitInfo first_hit_info() {      // over the ranks: the counters summed (each rank counts its own rays)
        ErFirstHitInfo sum{};
        for (ErScene* e : ers_) {
            ErFirstHitInfo i{};
            check(er_first_hit_info(e, &i));
            sum.cutouts = i.cutouts;
            sum.opacity_threshold = i.opacity_threshold;
            sum.rays += i.rays; sum.rays_through += i.rays_through; sum.layers_skipped += i.layers_skipped;
            sum.rays_capped += i.rays_capped; sum.rays_through_to_miss += i.rays_through_to_miss;
        }
        return sum;
    }
    // er_denoise_guided where the whole frame is: on a sharded frame on rank 0, after BEAUTY and NORMAL have been gathered there
    // (the features were when the pass ran)
    void denoise_guided(unsigned levels = 0, float colour_sigma = 0, float albedo_sigma = 0, float depth_sigma = 0) {
        if (ers_.empty()) throw std::runtime_error("denoise_guided: no render has been started");
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        denoise_guided_unlocked(levels, colour_sigma, albedo_sigma, depth_sigma);
    }
    // features if there are none yet + guided denoise + read of the DENOISE plane as ONE step against the render thread
    std::vector<float> get_denoised_guided(unsigned feature_samples = 0, unsigned levels = 0, float colour_sigma = 0, float albedo_sigma = 0, float depth_sigma = 0) {
        if (ers_.empty()) throw std::runtime_error("denoise_guided: no render has been started");
        std::unique_lock<std::mutex> lk(frame_mtx_, std::defer_lock);
        if (ers_.size() > 1) lk.lock();
        if (!features_ready_) render_features_unlocked(feature_samples);
        denoise_guided_unlocked(levels, colour_sigma, albedo_sigma, depth_sigma);
        return get_pass_unlocked(ER_PASS_DENOISE);
    }
    // adaptive sampling over the ranks: the ranks' tiles summed, samples_rendered of the rank that is furthest ahead (each rank stops
    // only its own tiles; the frame goes on while any rank has an active tile)
    uint32_t emitters() {      // the emitter table of ER_FLAG_MESH_LIGHTS (every rank builds the same one)
        ErLightInfo li{};
        if (!ers_.empty() && ers_[0] && er_light_info(ers_[0], &li) != ER_OK) return 0;
        return li.emitters;
    }
    ErAdaptiveInfo adaptive_info() {
        ErAdaptiveInfo sum{};
        for (ErScene* e : ers_) {
            ErAdaptiveInfo i{};
            check(er_adaptive_info(e, &i));
            sum.enabled = i.enabled;
            sum.owned_tiles += i.owned_tiles;
            sum.active_tiles += i.active_tiles;
            sum.samples_rendered = std::max(sum.samples_rendered, i.samples_rendered);
            sum.pixel_samples += i.pixel_samples;
        }
        return sum;
    }
    RenderInfo get_render_info() {   // src/Managers.cpp:211-232; several ranks: the one that is furthest behind
        RenderInfo i;
        if (ers_.empty()) throw std::runtime_error("get_info: no render has been started");
        i.samples = ~0u;
        for (ErScene* e : ers_) {
            unsigned s = 0;
            check(er_samples_done(e, &s));
            i.samples = std::min(i.samples, s);
        }
        return i;
    }
    // er_update_policy_set on every rank (every rank holds the whole structure): what a geometry edit does to it -- ER_REBUILD_NEVER the
    // refit, ALWAYS a fresh build in the same call, AUTO a fresh build once the refitted tree's measured cost exceeds max_cost_ratio x
    // the last built tree's.  Lasts for these scenes, i.e. until the next start_rendering.
    void set_update_policy(uint32_t mode, float max_cost_ratio = 0) {
        if (ers_.empty()) throw std::runtime_error("set_update_policy: no render has been started");
        const ErUpdatePolicy p{mode, max_cost_ratio};
        for (ErScene* e : ers_) check(er_update_policy_set(e, &p));
    }
    ErAccelCost accel_cost() {      // the ranks hold the same structure: rank 0's figures, the slowest rank's time
        if (ers_.empty()) throw std::runtime_error("accel_cost: no render has been started");
        ErAccelCost out{};
        for (size_t r = 0; r < ers_.size(); r++) {
            ErAccelCost c{};
            check(er_accel_cost(ers_[r], &c));
            const float ms = std::max(out.ms, c.ms);
            if (r == 0) out = c;
            out.ms = ms;
        }
        return out;
    }
    ErRebuildInfo rebuild_info() {      // rank 0's decisions (the same on every rank: the same bytes measured), the slowest rank's times
        if (ers_.empty()) throw std::runtime_error("rebuild_info: no render has been started");
        ErRebuildInfo out{};
        for (size_t r = 0; r < ers_.size(); r++) {
            ErRebuildInfo i{};
            check(er_rebuild_info(ers_[r], &i));
            const float cms = std::max(out.cost_ms, i.cost_ms), rms = std::max(out.rebuild_ms, i.rebuild_ms);
            if (r == 0) out = i;
            out.cost_ms = cms; out.rebuild_ms = rms;
        }
        return out;
    }
    unsigned ranks() const { return (unsigned)ers_.size(); }

private:
    std::vector<ErScene*> ers_;
    std::vector<ErComm*> comms_;
    std::mutex frame_mtx_;
    size_t textures_sent_ = 0;         // textures of the scene the ranks hold (start_rendering / edit_scene / append_scene)
    std::vector<int32_t> mats_sent_;   // the material id of every triangle the ranks hold (the same three)
    bool features_ready_ = false;      // a feature pass has run (and been gathered) since the last start_rendering / update_camera
    void render_features_unlocked(unsigned n) {
        features_ready_ = false;
        std::vector<std::string> errs(ers_.size());
        std::vector<std::thread> th;
        for (size_t r = 0; r < ers_.size(); r++)
            th.emplace_back([&, r] { if (er_render_features(ers_[r], n) != ER_OK) errs[r] = er_last_error(); });
        for (auto& t : th) t.join();
        for (auto& e : errs) if (!e.empty()) throw std::runtime_error(e);
        gather(ER_FEATURE_ALBEDO, true);
        gather(ER_FEATURE_DEPTH, true);
        features_ready_ = true;
    }
    void denoise_guided_unlocked(unsigned levels, float colour_sigma, float albedo_sigma, float depth_sigma) {
        gather(ER_PASS_BEAUTY);
        gather(ER_PASS_NORMAL);
        const ErDenoiseGuided p{levels, colour_sigma, albedo_sigma, depth_sigma};
        check(er_denoise_guided(ers_[0], &p));
    }
    std::vector<float> get_pass_unlocked(int pass) {
        std::vector<float> out((size_t)pars.width * pars.height * 4);
        gather(pass);
        check(er_read_pass(ers_[0], pass, out.data()));
        return out;
    }
    void denoise_unlocked(unsigned levels, float colour_sigma) {
        gather(ER_PASS_BEAUTY);
        gather(ER_PASS_NORMAL);
        check(er_denoise(ers_[0], levels, colour_sigma));
    }
    static void check(int rc, const char* what = nullptr) { if (rc != ER_OK) throw std::runtime_error(what ? what : er_last_error()); }
    // every rank's owned pixels of one plane -> rank 0's plane: one er_gather_pass per rank, side by side (the RCCL sends block until
    // the root has posted its receives, so the ranks cannot take turns on one thread)
    // (feature: `pass` names a feature plane, er_gather_feature)
    void gather(int pass, bool feature = false) {
        if (ers_.size() < 2 || (!feature && pass == ER_PASS_DENOISE)) return;      // (the DENOISE plane is only ever written on rank 0)
        std::vector<std::string> errs(ers_.size());
        std::vector<std::thread> th;
        for (size_t r = 0; r < ers_.size(); r++)
            th.emplace_back([&, r] { if ((feature ? er_gather_feature(ers_[r], pass, comms_[r], 0) : er_gather_pass(ers_[r], pass, comms_[r], 0)) != ER_OK) errs[r] = er_last_error(); });
        for (auto& t : th) t.join();
        for (auto& e : errs) if (!e.empty()) throw std::runtime_error(e);
    }
    void release() {
        for (ErComm* c : comms_) if (c) er_comm_destroy(c);
        comms_.clear();
        for (ErScene* e : ers_) if (e) er_scene_destroy(e);
        ers_.clear();
        features_ready_ = false;
        transport_used.clear();
    }
};

}  // namespace eleven
