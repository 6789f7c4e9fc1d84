// ref_driver.cpp -- runs the REFERENCE's own per-sample code on the host and writes down what it computes.
//
// TEST INFRASTRUCTURE ONLY.  This file is ours; it reaches the reference only through -I$(ER_REFERENCE_DIR)/src and through the
// reference's .cpp files that oracle/Makefile compiles, unmodified, from that directory (target `ref`, stand-in headers in
// oracle/ref_shim/).  Nothing of the reference and nothing compiled from it is committed: the two binaries live in oracle/_ref/
// and only their numbers reach tests/golden/ (tests/golden/make_golden_reference.py).
//
//   ref_libm  the sycl:: math names forward to glibc's float functions
//   ref_er    the six functions of elevenrender_amd/csrc/er_math.h are plugged in underneath; everything else is the same
//
// usage: ref_libm|ref_er <in.erkv> <out.erkv>
// A job file is a flat list of named arrays (format below).  The driver builds a dev_Scene by hand from the scene arrays, has the
// reference's own BVH.cpp build the tree, and answers every section whose input arrays are present:
//   rng_idx                      -> rng_states, rng_values          RngGenerator(idx), 16 x next()
//   cam_items [n,7]              -> cam_rays [n,6]                  calculateCameraRay
//   trihit_items [n,7]           -> trihit_ok [n], trihit_rec [n,17] Tri::hit
//   closest_o, closest_d [n,3]   -> closest_tri [n], closest_pos [n,3]  throwRay (triangle = bvh->triIndices[Hit.triIdx])
//                                   closest_alltri [n], closest_allpos [n,3]  Tri::hit over every triangle, no tree
//   disney_items [n,29], disney_rs [n,3] -> disney_eval [n,3], disney_pdf [n], disney_sample [n,3]
//   sph_p [n,3] -> sph_uv [n,2];  rev_uv [n,2] -> rev_p [n,3]
//   texfetch_items [n,4]         -> texfetch [n,3]                  getValueFromUVFiltered / getValueFromUV
//   (hdri) -> hdri_cdf, hdri_rsum;  hdri_search_vals -> hdri_search;  hdri_pdf_xy [n,2] -> hdri_pdf [n]
//   res[2] = spp > 0             -> pass_* [h,w,4] x 5, samples, rng  setupKernel + spp x renderingKernel per pixel
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "BVH.h"
#include "Camera.h"
#include "Disney.h"
#include "HDRI.h"
#include "Material.h"
#include "MeshObject.hpp"
#include "Texture.h"
#include "Tri.h"
#include "kernel.h"

// entry points of the reference's kernel.cpp that its header does not declare
void setupKernel(dev_Scene*, int);
Hit throwRay(Ray, dev_Scene*);
void calculateCameraRay(int, int, dev_Scene&, Camera&, Ray&, float, float, float, float, float);   // x, y, ..., the five randoms

// kernel.cpp's host-side entry points name these; this driver never takes those routes
[[noreturn]] static void never(const char* what) {
    fprintf(stderr, "ref_driver: %s is not part of the driven path\n", what);
    abort();
}
int Scene::materialCount() { never("Scene::materialCount"); }
int Scene::textureCount() { never("Scene::textureCount"); }
int Scene::meshObjectCount() { never("Scene::meshObjectCount"); }
int Scene::triCount() { never("Scene::triCount"); }
int Scene::pointLightCount() { never("Scene::pointLightCount"); }
Material* Scene::getMaterials() { never("Scene::getMaterials"); }
Tri* Scene::getTris() { never("Scene::getTris"); }
MeshObject* Scene::getMeshObjects() { never("Scene::getMeshObjects"); }
PointLight* Scene::getPointLights() { never("Scene::getPointLights"); }
Texture* Scene::getTextures() { never("Scene::getTextures"); }
BVH* Scene::buildBVH() { never("Scene::buildBVH"); }
void copy_scene(dev_Scene*, dev_Scene*, sycl::queue&) { never("copy_scene"); }

// ---------------------------------------------------------------- job files
// "ERKV", u32 count, then per array: u32 name length, name, u32 dtype (0 f32, 1 i32, 2 u32), u64 element count, the elements.
struct Arr {
    uint32_t dtype = 0;
    std::vector<uint32_t> w;   // 32-bit elements, whatever the type
    size_t n() const { return w.size(); }
    const float* f() const { return reinterpret_cast<const float*>(w.data()); }
    const int32_t* i() const { return reinterpret_cast<const int32_t*>(w.data()); }
    const uint32_t* u() const { return w.data(); }
};
typedef std::map<std::string, Arr> Job;

static void rd(FILE* f, void* p, size_t n) {
    if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "ref_driver: short read\n"); exit(2); }
}
static Job load(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    char magic[4];
    uint32_t count;
    rd(f, magic, 4);
    rd(f, &count, 4);
    if (memcmp(magic, "ERKV", 4)) { fprintf(stderr, "ref_driver: %s is not a job file\n", path); exit(2); }
    Job job;
    for (uint32_t k = 0; k < count; k++) {
        uint32_t len;
        rd(f, &len, 4);
        std::string name(len, ' ');
        rd(f, &name[0], len);
        Arr a;
        uint64_t n;
        rd(f, &a.dtype, 4);
        rd(f, &n, 8);
        a.w.resize(n);
        rd(f, a.w.data(), n * 4);
        job[name] = a;
    }
    fclose(f);
    return job;
}
static void save(const char* path, const Job& job) {
    FILE* f = fopen(path, "wb");
    if (!f) { perror(path); exit(2); }
    uint32_t count = (uint32_t)job.size();
    fwrite("ERKV", 1, 4, f);
    fwrite(&count, 4, 1, f);
    for (const auto& kv : job) {
        uint32_t len = (uint32_t)kv.first.size();
        uint64_t n = kv.second.n();
        fwrite(&len, 4, 1, f);
        fwrite(kv.first.data(), 1, len, f);
        fwrite(&kv.second.dtype, 4, 1, f);
        fwrite(&n, 8, 1, f);
        fwrite(kv.second.w.data(), 4, n, f);
    }
    fclose(f);
}
static Arr& out_f(Job& out, const char* name, size_t n) { Arr& a = out[name]; a.dtype = 0; a.w.assign(n, 0); return a; }
static Arr& out_i(Job& out, const char* name, size_t n) { Arr& a = out[name]; a.dtype = 1; a.w.assign(n, 0); return a; }
static Arr& out_u(Job& out, const char* name, size_t n) { Arr& a = out[name]; a.dtype = 2; a.w.assign(n, 0); return a; }
static float* F(Arr& a) { return reinterpret_cast<float*>(a.w.data()); }
static int32_t* I(Arr& a) { return reinterpret_cast<int32_t*>(a.w.data()); }
static void put3(float* d, const Vector3& v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }
static Vector3 v3(const float* p) { return Vector3(p[0], p[1], p[2]); }
static int32_t bits_i(float f) { int32_t i; memcpy(&i, &f, 4); return i; }

// ---------------------------------------------------------------- the scene, by hand
static Texture make_texture(const Arr& data, const Arr& meta) {
    Texture t;
    t.width = meta.i()[0];
    t.height = meta.i()[1];
    t.channels = (unsigned int)meta.i()[2];
    t.filter = meta.i()[3] == 1 ? Texture::Filter::BILINEAR : Texture::Filter::NO_FILTER;
    t.data = new float[data.n() ? data.n() : 1];
    memcpy(t.data, data.f(), data.n() * sizeof(float));
    return t;
}

struct Built {
    dev_Scene* scene = nullptr;
    std::vector<Tri> tris;
    std::vector<Texture> textures;
    std::vector<Material> materials;
    Camera camera;
    HDRI* hdri = nullptr;
    MeshObject mesh;
};

// materials: rows of 29 floats in the order of ErMaterial (include/eleven_hip.h); camera: the 12 floats of ErCamera
static void build_scene(const Job& job, Built& b) {
    b.scene = static_cast<dev_Scene*>(calloc(1, sizeof(dev_Scene)));
    dev_Scene* s = b.scene;
    if (job.count("camera")) {
        const float* c = job.at("camera").f();
        b.camera.focalLength = c[0]; b.camera.sensorWidth = c[1]; b.camera.sensorHeight = c[2];
        b.camera.aperture = c[3]; b.camera.focusDistance = c[4];
        b.camera.rotation = v3(c + 5);
        b.camera.bokeh = c[8] != 0.0f;
        b.camera.position = v3(c + 9);
    }
    s->camera = &b.camera;
    if (job.count("res")) { s->x_res = (unsigned int)job.at("res").i()[0]; s->y_res = (unsigned int)job.at("res").i()[1]; }
    for (int k = 0; job.count("tex" + std::to_string(k)); k++)
        b.textures.push_back(make_texture(job.at("tex" + std::to_string(k)), job.at("tex" + std::to_string(k) + "_meta")));
    s->textures = b.textures.data();
    s->textureCount = (unsigned int)b.textures.size();
    if (job.count("hdri")) {
        b.hdri = new HDRI(make_texture(job.at("hdri"), job.at("hdri_meta")));   // generateCDF runs in the constructor
        s->hdri = b.hdri;
    }
    if (job.count("materials")) {
        const Arr& m = job.at("materials");
        for (size_t k = 0; k < m.n() / 29; k++) {
            const float* r = m.f() + 29 * k;
            Material mat;
            mat.albedoTextureID = (int)r[0]; mat.emissionTextureID = (int)r[1]; mat.roughnessTextureID = (int)r[2];
            mat.metallicTextureID = (int)r[3]; mat.normalTextureID = (int)r[4]; mat.opacityTextureID = (int)r[5];
            mat.transmissionTextureID = (int)r[6]; mat.albedoShaderID = (int)r[7];
            mat.albedo = v3(r + 8); mat.emission = v3(r + 11);
            mat.opacity = r[14]; mat.roughness = r[15]; mat.metallic = r[16]; mat.clearcoatGloss = r[17]; mat.clearcoat = r[18];
            mat.anisotropic = r[19]; mat.eta = r[20]; mat.transmission = r[21]; mat.specular = r[22]; mat.specularTint = r[23];
            mat.sheenTint = r[24]; mat.subsurface = r[25]; mat.sheen = r[26]; mat.ax = r[27]; mat.ay = r[28];
            b.materials.push_back(mat);
        }
    }
    s->materials = b.materials.data();
    s->materialCount = (unsigned int)b.materials.size();
    if (job.count("vertices")) {
        const float* V = job.at("vertices").f();
        const float* N = job.at("normals").f();
        const float* T = job.at("tangents").f();
        const float* U = job.at("uvs").f();
        const float* S = job.at("tangent_sign").f();
        const int32_t* M = job.at("material_id").i();
        size_t n = job.at("tangent_sign").n();
        b.tris.resize(n);
        for (size_t i = 0; i < n; i++) {
            Tri& t = b.tris[i];
            for (int k = 0; k < 3; k++) {
                t.vertices[k] = v3(V + 9 * i + 3 * k);
                t.normals[k] = v3(N + 9 * i + 3 * k);
                t.tangents[k] = v3(T + 9 * i + 3 * k);
                t.uv[k] = Vector3(U[6 * i + 2 * k], U[6 * i + 2 * k + 1], 0);
            }
            t.tangentsSign = S[i];
            t.objectID = 0;
            t.materialID = M[i];
        }
        s->tris = b.tris.data();
        s->triCount = (unsigned int)n;
        b.mesh.tris = b.tris.data();
        b.mesh.triCount = (unsigned int)n;
        s->meshObjects = &b.mesh;
        s->meshObjectCount = 1;
        // what Scene::buildBVH does: a BVH with an index array of its own, built by the reference's BVH::build
        BVH* bvh = new BVH();
        bvh->triIndices = new int[n];
        bvh->build(&b.tris);
        bvh->tris = b.tris.data();
        s->bvh = bvh;
    }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <in.erkv> <out.erkv>\n", argv[0]); return 2; }
    Job job = load(argv[1]);
    Job out;
    Built b;
    build_scene(job, b);
    dev_Scene* s = b.scene;

    if (job.count("rng_idx")) {
        const Arr& idx = job.at("rng_idx");
        Arr& st = out_u(out, "rng_states", idx.n() * 16);
        Arr& va = out_f(out, "rng_values", idx.n() * 16);
        for (size_t k = 0; k < idx.n(); k++) {
            RngGenerator g(idx.u()[k]);
            for (int j = 0; j < 16; j++) { F(va)[16 * k + j] = g.next(); st.w[16 * k + j] = g.state; }
        }
    }
    if (job.count("cam_items")) {
        const Arr& it = job.at("cam_items");
        size_t n = it.n() / 7;
        Arr& o = out_f(out, "cam_rays", n * 6);
        for (size_t k = 0; k < n; k++) {
            const float* r = it.f() + 7 * k;
            Ray ray;
            calculateCameraRay((int)r[0], (int)r[1], *s, b.camera, ray, r[2], r[3], r[4], r[5], r[6]);
            put3(F(o) + 6 * k, ray.origin);
            put3(F(o) + 6 * k + 3, ray.direction);
        }
    }
    if (job.count("trihit_items")) {
        const Arr& it = job.at("trihit_items");
        size_t n = it.n() / 7;
        Arr& ok = out_i(out, "trihit_ok", n);
        Arr& rec = out_f(out, "trihit_rec", n * 17);
        for (size_t k = 0; k < n; k++) {
            const float* r = it.f() + 7 * k;
            Ray ray;                       // the direction as given: the callers pass what Ray's constructor would have produced
            ray.origin = v3(r + 1);
            ray.direction = v3(r + 4);
            Hit h;
            if (!b.tris[bits_i(r[0])].hit(ray, h)) continue;
            I(ok)[k] = 1;
            float* d = F(rec) + 17 * k;
            put3(d, h.position); put3(d + 3, h.normal); put3(d + 6, h.gnormal); put3(d + 9, h.tangent); put3(d + 12, h.bitangent);
            d[15] = h.tu; d[16] = h.tv;
        }
    }
    if (job.count("closest_o")) {
        const Arr& O = job.at("closest_o");
        const Arr& D = job.at("closest_d");
        size_t n = O.n() / 3;
        Arr& tri = out_i(out, "closest_tri", n);
        Arr& pos = out_f(out, "closest_pos", n * 3);
        Arr& atri = out_i(out, "closest_alltri", n);
        Arr& apos = out_f(out, "closest_allpos", n * 3);
        for (size_t k = 0; k < n; k++) {
            Ray ray;
            ray.origin = v3(O.f() + 3 * k);
            ray.direction = v3(D.f() + 3 * k);
            Hit h = throwRay(ray, s);
            I(tri)[k] = h.valid ? s->bvh->triIndices[h.triIdx] : -1;
            put3(F(pos) + 3 * k, h.position);
            // the same query without the tree: the reference's Tri::hit on EVERY triangle, nearest by the same metric (this loop is
            // ours).  Where the two differ, a box test of the reference's tree dropped the hit.
            Hit best;
            int best_tri = -1;
            for (size_t t = 0; t < b.tris.size(); t++) {
                Hit c;
                if (b.tris[t].hit(ray, c) && (!best.valid || (c.position - ray.origin).length() < (best.position - ray.origin).length())) {
                    best = c;
                    best_tri = (int)t;
                }
            }
            I(atri)[k] = best_tri;
            put3(F(apos) + 3 * k, best.position);
        }
    }
    if (job.count("disney_items")) {
        // 20 floats of HitData (the order of er_oracle.h's hd[]), V, N, L; disney_rs: r1, r2, r3
        const Arr& it = job.at("disney_items");
        const Arr& rs = job.at("disney_rs");
        size_t n = it.n() / 29;
        Arr& ev = out_f(out, "disney_eval", n * 3);
        Arr& pd = out_f(out, "disney_pdf", n);
        Arr& sm = out_f(out, "disney_sample", n * 3);
        for (size_t k = 0; k < n; k++) {
            const float* h = it.f() + 29 * k;
            HitData hd;
            memset(&hd, 0, sizeof(hd));
            hd.metallic = h[0]; hd.roughness = h[1]; hd.clearcoatGloss = h[2]; hd.clearcoat = h[3]; hd.anisotropic = h[4];
            hd.transmission = h[5]; hd.specular = h[6]; hd.specularTint = h[7]; hd.sheenTint = h[8]; hd.subsurface = h[9];
            hd.sheen = h[10]; hd.albedo = v3(h + 11); hd.tangent = v3(h + 14); hd.bitangent = v3(h + 17);
            Vector3 V = v3(h + 20), N = v3(h + 23), L = v3(h + 26);
            HitData a = hd, c = hd, d = hd;
            put3(F(ev) + 3 * k, DisneyEval(a, V, N, L));
            F(pd)[k] = DisneyPdf(c, V, N, L);
            put3(F(sm) + 3 * k, DisneySample(d, V, N, rs.f()[3 * k], rs.f()[3 * k + 1], rs.f()[3 * k + 2]));
        }
    }
    if (job.count("sph_p")) {
        const Arr& p = job.at("sph_p");
        size_t n = p.n() / 3;
        Arr& uv = out_f(out, "sph_uv", n * 2);
        for (size_t k = 0; k < n; k++) Texture::sphericalMapping(Vector3(), v3(p.f() + 3 * k), 1, F(uv)[2 * k], F(uv)[2 * k + 1]);
    }
    if (job.count("rev_uv")) {
        const Arr& uv = job.at("rev_uv");
        size_t n = uv.n() / 2;
        Arr& p = out_f(out, "rev_p", n * 3);
        Texture any;
        for (size_t k = 0; k < n; k++) put3(F(p) + 3 * k, any.reverseSphericalMapping(uv.f()[2 * k], uv.f()[2 * k + 1]));
    }
    if (job.count("texfetch_items")) {
        // texture id as float bits (-1 = the HDRI's texture), u, v, filtered
        const Arr& it = job.at("texfetch_items");
        size_t n = it.n() / 4;
        Arr& o = out_f(out, "texfetch", n * 3);
        for (size_t k = 0; k < n; k++) {
            const float* r = it.f() + 4 * k;
            int tid = bits_i(r[0]);
            Texture& t = tid < 0 ? b.hdri->texture : b.textures[tid];
            put3(F(o) + 3 * k, r[3] != 0.0f ? t.getValueFromUVFiltered(r[1], r[2]) : t.getValueFromUV(r[1], r[2]));
        }
    }
    if (b.hdri) {
        size_t n = (size_t)b.hdri->texture.width * b.hdri->texture.height;
        Arr& cdf = out_f(out, "hdri_cdf", n + 1);
        memcpy(F(cdf), b.hdri->cdf, (n + 1) * sizeof(float));
        F(out_f(out, "hdri_rsum", 1))[0] = b.hdri->radianceSum;
        if (job.count("hdri_search_vals")) {
            const Arr& v = job.at("hdri_search_vals");
            Arr& o = out_i(out, "hdri_search", v.n());
            for (size_t k = 0; k < v.n(); k++) I(o)[k] = b.hdri->binarySearch(b.hdri->cdf, v.f()[k], (int)n);
        }
        if (job.count("hdri_pdf_xy")) {
            const Arr& xy = job.at("hdri_pdf_xy");
            Arr& o = out_f(out, "hdri_pdf", xy.n() / 2);
            for (size_t k = 0; k < xy.n() / 2; k++) F(o)[k] = b.hdri->pdf(xy.i()[2 * k], xy.i()[2 * k + 1]);
        }
    }
    if (job.count("res") && job.at("res").i()[2] > 0) {
        int spp = job.at("res").i()[2];
        size_t npx = (size_t)s->x_res * s->y_res;
        std::vector<float> passes(npx * 4 * PASSES_COUNT);
        std::vector<unsigned int> samples(npx);
        std::vector<RngGenerator> rng(npx, RngGenerator(0));
        s->dev_passes = passes.data();
        s->dev_samples = samples.data();
        s->dev_randstate = rng.data();
        for (size_t idx = 0; idx < npx; idx++) setupKernel(s, (int)idx);
        for (int k = 0; k < spp; k++)
            for (size_t idx = 0; idx < npx; idx++) renderingKernel(s, (int)idx, spp);
        static const char* names[PASSES_COUNT] = {"pass_beauty", "pass_denoise", "pass_normal", "pass_tangent", "pass_bitangent"};
        for (int p = 0; p < PASSES_COUNT; p++) memcpy(F(out_f(out, names[p], npx * 4)), passes.data() + p * npx * 4, npx * 16);
        memcpy(out_u(out, "samples", npx).w.data(), samples.data(), npx * 4);
        Arr& r = out_u(out, "rng", npx);
        for (size_t idx = 0; idx < npx; idx++) r.w[idx] = rng[idx].state;
        F(out_f(out, "max_bounces", 1))[0] = (float)MAXBOUNCES;
    }
    save(argv[2], out);
    return 0;
}
