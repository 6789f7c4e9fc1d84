// er_texstage.hip -- the texture stage on the device (er_texstage.h): what er_render_edit runs instead of the host loops of
// er_render_begin's texture stage when a texture assignment or a texture changes.  The layout is the texture plan's (er_texplan.h);
// the values are the host fill's, bit for bit: copies move floats, and the one computed value -- the first channel to the power 2.2 --
// comes from er_math.h's er_pow, one implementation for host and device (tests/test_gpu_function_kat.py compares its bits).
//
// How the texels reach the pool:
//   mode 0 (as it came)        asynchronous copy from the host texels to the texture's pool offset
//   mode 1 / 2 (first channel) raw upload to a transient staging buffer, then k_first_channel: pool[off + k] = raw[k * channels],
//                              to the power 2.2 in mode 2
//   fused records              k_fuse, after all of the above on the same stream, from the pool itself (see the kernel)
//   the HDRI                   asynchronous copy to the pool's tail
// Every kernel is a bounded grid walked with a grid stride; no workgroup waits for another; every store is one float (pool offsets
// are arbitrary float offsets and a fused record is 20 bytes: nothing wider is aligned).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "er_bvh.h"
#include "er_math.h"
#include "er_texstage.h"

namespace {

constexpr uint32_t TS_BLOCK = 256, TS_MAX_BLOCKS = 2048;

uint32_t ts_blocks(uint64_t n) { return (uint32_t)std::min<uint64_t>(TS_MAX_BLOCKS, (n + TS_BLOCK - 1) / TS_BLOCK); }

// pool[off + k] = raw[k * channels] for k < n, to the power 2.2 if `powered`
__global__ __launch_bounds__(TS_BLOCK) void k_first_channel(const float* __restrict__ raw, uint32_t channels, uint64_t n, int powered, float* __restrict__ dst) {
    const uint64_t stride = (uint64_t)gridDim.x * TS_BLOCK;
    for (uint64_t k = (uint64_t)blockIdx.x * TS_BLOCK + threadIdx.x; k < n; k += stride) {
        const float v = raw[k * channels];
        dst[k] = powered ? ermath::er_pow(v, 2.2f) : v;
    }
}

// One fused record per texel: albedo r g b, roughness, metallic.
// WHERE EACH VALUE COMES FROM -- one rule: the texture's own entry in the pool being built (the entries precede the records and are
// complete when this kernel starts: same stream), read as the table describes it.  Albedo: its entry is always "as it came" (an albedo
// use rules the compaction out), read by the channel rules of Texture::getValueFromCoordinates (src/Texture.cpp:181-197): one
// channel: the value three times; two: x, y, 0; three or more: the first three.  Roughness and metallic: the first channel of the
// entry, whatever its stride (1 for a compacted entry); if the record is `powered` (unfiltered) it holds them to the power 2.2 -- an
// entry marked 2 already holds that power and is copied, any other is raised here.  er_pow is deterministic and the raw first channel
// of a compacted entry is the texture's raw first channel, so this equals the host fill byte for byte.
__global__ __launch_bounds__(TS_BLOCK) void k_fuse(float* __restrict__ pool, DevTex ta, DevTex tr, DevTex tk, uint64_t n, int powered, uint64_t out_off) {
    const uint64_t stride = (uint64_t)gridDim.x * TS_BLOCK;
    const bool r_pow = powered && tr.filter != 2, k_pow = powered && tk.filter != 2;
    for (uint64_t k = (uint64_t)blockIdx.x * TS_BLOCK + threadIdx.x; k < n; k += stride) {
        const float* a = pool + (uint64_t)ta.offset + k * (uint64_t)ta.channels;
        const float a0 = a[0];
        const float a1 = ta.channels == 1 ? a0 : a[1];
        const float a2 = ta.channels == 1 ? a0 : (ta.channels == 2 ? 0.0f : a[2]);
        const float r = pool[(uint64_t)tr.offset + k * (uint64_t)tr.channels], m = pool[(uint64_t)tk.offset + k * (uint64_t)tk.channels];
        float* o = pool + out_off + 5 * k;
        o[0] = a0;
        o[1] = a1;
        o[2] = a2;
        o[3] = r_pow ? ermath::er_pow(r, 2.2f) : r;
        o[4] = k_pow ? ermath::er_pow(m, 2.2f) : m;
    }
}

// one thread per slot: the attribute record's material from the input triangle's
__global__ __launch_bounds__(TS_BLOCK) void k_material_ids(const float4* __restrict__ isect, float4* __restrict__ attr, uint32_t tri_count, const int32_t* __restrict__ material_id) {
    const uint64_t stride = (uint64_t)gridDim.x * TS_BLOCK;
    for (uint64_t slot = (uint64_t)blockIdx.x * TS_BLOCK + threadIdx.x; slot < tri_count; slot += stride) {
        const int32_t tri = ((const ErTriIsect*)isect)[slot].tri_id;
        ((ErTriAttr*)(attr + slot * ER_ATTR_PIECES))->material = material_id[tri];
    }
}

struct TsScratch {      // what the stage allocates for itself: gone on every way out
    float* staging = nullptr;
    float* pool = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    ~TsScratch() {
        if (staging) (void)hipFree(staging);
        if (pool) (void)hipFree(pool);
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

}  // namespace

hipError_t er_probe_texstage(const char** which) {
    hipFuncAttributes at;
    hipError_t e;
    *which = "k_first_channel (er_texstage.hip)";
    if ((e = hipFuncGetAttributes(&at, (const void*)k_first_channel)) != hipSuccess) return e;
    *which = "k_fuse (er_texstage.hip)";
    if ((e = hipFuncGetAttributes(&at, (const void*)k_fuse)) != hipSuccess) return e;
    *which = "k_material_ids (er_texstage.hip)";
    return hipFuncGetAttributes(&at, (const void*)k_material_ids);
}

void er_launch_material_ids(const float4* isect, float4* attr, uint32_t tri_count, const int32_t* material_id, hipStream_t stream) {
    if (tri_count == 0) return;
    hipLaunchKernelGGL(k_material_ids, dim3(ts_blocks(tri_count)), dim3(TS_BLOCK), 0, stream, isect, attr, tri_count, material_id);
}

#define TS_TRY(expr)                                                                   \
    do {                                                                               \
        hipError_t e__ = (expr);                                                       \
        if (e__ != hipSuccess) {                                                       \
            err = std::string(#expr) + ": " + hipGetErrorString(e__);                  \
            return e__ == hipErrorOutOfMemory ? -2 : -1;                               \
        }                                                                              \
    } while (0)

int er_texstage_build(const erh::TexPlan& P, const ErTexSource* tex, size_t ntex, const ErMaterial* mats, size_t nmat, const ErTexSource& hdri,
                      hipStream_t stream, float** pool_out, float* ms, std::string& err) {
    *pool_out = nullptr;
    *ms = 0;
    if (P.pool_floats >= (1ull << 32) || P.table.size() != ntex || P.mode.size() != ntex || P.fused.size() < nmat) {
        err = "er_texstage_build: the plan does not fit its arguments";
        return -1;
    }
    TsScratch S;
    TS_TRY(hipEventCreate(&S.a));
    TS_TRY(hipEventCreate(&S.b));
    TS_TRY(hipMalloc((void**)&S.pool, std::max<uint64_t>(P.pool_floats, 1) * sizeof(float)));
    // the raw texels of the textures kept by their first channel, back to back in a transient staging buffer
    std::vector<uint64_t> stage_off(ntex, 0);
    uint64_t stage_floats = 0;
    auto floats_of = [](const ErTexSource& t) { return (uint64_t)std::max(0, t.width) * (uint64_t)std::max(0, t.height) * (uint64_t)std::max(0, t.channels); };
    for (size_t i = 0; i < ntex; i++) {
        if (tex[i].width != P.table[i].width || tex[i].height != P.table[i].height) {
            err = "er_texstage_build: a texture is not the size the plan was made for";
            return -1;
        }
        if (!P.mode[i]) continue;
        stage_off[i] = stage_floats;
        stage_floats += floats_of(tex[i]);
    }
    if (stage_floats) TS_TRY(hipMalloc((void**)&S.staging, stage_floats * sizeof(float)));
    TS_TRY(hipEventRecord(S.a, stream));
    for (size_t i = 0; i < ntex; i++) {
        const uint64_t nf = floats_of(tex[i]), n = (uint64_t)tex[i].width * (uint64_t)tex[i].height;
        if (nf == 0) continue;
        if (!P.mode[i]) {
            TS_TRY(hipMemcpyAsync(S.pool + P.table[i].offset, tex[i].data, nf * sizeof(float), hipMemcpyHostToDevice, stream));
            continue;
        }
        float* raw = S.staging + stage_off[i];
        TS_TRY(hipMemcpyAsync(raw, tex[i].data, nf * sizeof(float), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_first_channel, dim3(ts_blocks(n)), dim3(TS_BLOCK), 0, stream, (const float*)raw, (uint32_t)tex[i].channels, n, P.mode[i] == 2 ? 1 : 0,
                           S.pool + P.table[i].offset);
    }
    for (size_t m = 0; m < nmat; m++) {
        const DevFused& f = P.fused[m];
        if (f.width <= 0) continue;
        const ErMaterial& M = mats[m];
        const DevTex ta = P.table[(size_t)M.albedo_tex], tr = P.table[(size_t)M.roughness_tex], tk = P.table[(size_t)M.metallic_tex];
        const uint64_t n = (uint64_t)f.width * (uint64_t)f.height;
        hipLaunchKernelGGL(k_fuse, dim3(ts_blocks(n)), dim3(TS_BLOCK), 0, stream, S.pool, ta, tr, tk, n, f.filter == 2 ? 1 : 0, (uint64_t)f.offset);
    }
    TS_TRY(hipGetLastError());
    {
        const uint64_t nf = floats_of(hdri);
        if (nf) TS_TRY(hipMemcpyAsync(S.pool + P.hdri.offset, hdri.data, nf * sizeof(float), hipMemcpyHostToDevice, stream));
    }
    TS_TRY(hipEventRecord(S.b, stream));
    TS_TRY(hipStreamSynchronize(stream));      // (the staging buffer is released, by S, only now)
    (void)hipEventElapsedTime(ms, S.a, S.b);
    *pool_out = S.pool;
    S.pool = nullptr;
    return 0;
}
