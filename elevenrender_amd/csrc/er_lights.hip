// er_lights.hip -- the emitter table of ER_FLAG_MESH_LIGHTS (er_shade.h rule 1; layout: er_lights.h), built on the device from the
// triangle records either builder has placed, so that a scene of millions of triangles never routes it through the host.
//
// Five steps, all on one stream:
//   1. mean luminance of every texture some material uses as emission_tex: one workgroup of 256 per texture;
//   2. per slot: the weight w = A * lum (0 for a triangle that is no emitter), and per workgroup of 1024 slots the number of emitters
//      (ballot per wave, the 16 wave counts in LDS);
//   3. an exclusive prefix over the workgroups' counts (one workgroup) -- the host reads the total once, to size the table;
//   4. ordered compaction: an emitter's place is its workgroup's offset + its wave's offset in the workgroup + mbcnt in the wave, so the
//      emitters come out in ascending slot order (the leaf order of the traversal);
//   5. the CDF over the compacted weights and P = w / W per slot.
//
// Float arithmetic, in this exact order (tests/mesh_light_scenes.py replays it for tests/test_gpu_mesh_lights.py, and so does the oracle):
//   lum(r, g, b) = (0.2126f * r + 0.7152f * g) + 0.0722f * b, no fused multiply-add (the Makefile's -ffp-contract=off);
//   texel values as tex_coords reads them: one channel c -> (c, c, c), two -> (r, g, 0), three or more -> the first three;
//   texture mean: thread t of 256 sums the luminances of texels t, t + 256, t + 512, ... in ascending order starting from 0.0f; the
//     256 partial sums are added pairwise in LDS, s[t] += s[t + h] for h = 128, 64, ..., 1; mean = s[0] / (float)(width * height);
//   area: c = cross(v1 - v0, v2 - v0) (er_device.h), A = 0.5f * sqrtf(c.x * c.x + c.y * c.y + c.z * c.z);
//   weight: A * lum, with lum = the texture mean for emission_tex >= 0, else lum(emission);
//   CDF over the n compacted weights, one workgroup of 1024 threads: chunk = ceil(n / 1024) entries per thread, thread t owns
//     [t * chunk, (t + 1) * chunk); s_t = its weights summed in ascending order from 0.0f; off_0 = 0.0f, off_{t+1} = off_t + s_t in
//     ascending t (one thread); W = off_1024; then thread t runs r = off_t, r = r + w_i over its chunk ascending, cdf_i = r / W;
//   P per slot: w / W.
#include "er_lights.h"
#include "er_device.h"

using namespace erd;

namespace {

__device__ __forceinline__ float er_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

__global__ __launch_bounds__(256) void er_lights_tex_mean_kernel(const DevTex* __restrict__ textures, const float* __restrict__ pool,
                                                                 const int32_t* __restrict__ ids, float* __restrict__ mean) {
    __shared__ float s[256];
    const uint32_t t = threadIdx.x;
    const int32_t id = ids[blockIdx.x];
    const DevTex tx = textures[id];
    const size_t texels = (size_t)tx.width * (size_t)tx.height;
    const float* d = pool + tx.offset;
    float acc = 0.0f;
    for (size_t i = t; i < texels; i += 256) {
        float r = 0.0f, g = 0.0f, b = 0.0f;
        if (tx.channels == 1) { r = g = b = d[i]; }
        else if (tx.channels == 2) { r = d[2 * i]; g = d[2 * i + 1]; }
        else if (tx.channels >= 3) { r = d[(size_t)tx.channels * i]; g = d[(size_t)tx.channels * i + 1]; b = d[(size_t)tx.channels * i + 2]; }
        acc = acc + er_lum(r, g, b);
    }
    s[t] = acc;
    __syncthreads();
    for (uint32_t h = 128; h >= 1; h >>= 1) {
        if (t < h) s[t] = s[t] + s[t + h];
        __syncthreads();
    }
    if (t == 0) mean[id] = s[0] / (float)texels;
}

// per slot: weight (0: no entry) and the workgroup's emitter count
__global__ __launch_bounds__(1024) void er_lights_weight_kernel(const float4* __restrict__ isect, const float4* __restrict__ attr, uint32_t n,
                                                                const ErMaterial* __restrict__ materials, const float* __restrict__ tex_mean,
                                                                float* __restrict__ w, uint32_t* __restrict__ block_count) {
    __shared__ uint32_t s_wave[16];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint32_t i = blockIdx.x * 1024u + t;
    float weight = 0.0f;
    if (i < n) {
        const int32_t m = __builtin_bit_cast(int32_t, attr[(size_t)i * ER_ATTR_PIECES + 6].x);
        const ErMaterial& mat = materials[m];
        float lum = 0.0f;
        bool emitter = false;
        if (mat.emission_tex >= 0) { lum = tex_mean[mat.emission_tex]; emitter = true; }
        else { lum = er_lum(mat.emission.x, mat.emission.y, mat.emission.z); emitter = lum > 0.0f; }
        if (emitter) {
            const float4 a = isect[(size_t)i * 3], b = isect[(size_t)i * 3 + 1], c = isect[(size_t)i * 3 + 2];
            const F3 v0 = f3(a.x, a.y, a.z), v1 = f3(b.x, b.y, b.z), v2 = f3(c.x, c.y, c.z);
            const float area = 0.5f * length(cross(v1 - v0, v2 - v0));
            weight = area * lum;
            if (!(area > 0.0f) || !(weight > 0.0f)) weight = 0.0f;      // (zero area or zero weight: no entry; NaN too)
        }
        w[i] = weight;
    }
    const unsigned long long mk = __ballot(weight > 0.0f);
    if (lane == 0) s_wave[wv] = (uint32_t)__popcll(mk);
    __syncthreads();
    if (t == 0) {
        uint32_t sum = 0;
        for (uint32_t x = 0; x < 16u; x++) sum += s_wave[x];
        block_count[blockIdx.x] = sum;
    }
}

// exclusive prefix over the workgroups' counts: off[b], and off[nb] = the total
__global__ __launch_bounds__(1024) void er_lights_scan_kernel(const uint32_t* __restrict__ block_count, uint32_t nb, uint32_t* __restrict__ off) {
    __shared__ uint32_t s[1025];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (nb + 1023u) / 1024u, lo = t * chunk, hi = lo + chunk < nb ? lo + chunk : nb;
    uint32_t sum = 0;
    for (uint32_t b = lo; b < hi; b++) sum += block_count[b];
    s[t + 1] = sum;
    __syncthreads();
    if (t == 0) {
        s[0] = 0;
        for (uint32_t x = 1; x <= 1024u; x++) s[x] += s[x - 1];
    }
    __syncthreads();
    uint32_t run = s[t];
    for (uint32_t b = lo; b < hi; b++) { off[b] = run; run += block_count[b]; }
    if (t == 0) off[nb] = s[1024];
}

// ordered compaction: slots and weights of the emitters, ascending
__global__ __launch_bounds__(1024) void er_lights_scatter_kernel(const float* __restrict__ w, uint32_t n, const uint32_t* __restrict__ off,
                                                                 float* __restrict__ w_out, uint32_t* __restrict__ slot_out) {
    __shared__ uint32_t s_wave[16];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint32_t i = blockIdx.x * 1024u + t;
    const float weight = i < n ? w[i] : 0.0f;
    const bool k = weight > 0.0f;
    const unsigned long long mk = __ballot(k);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
    if (lane == 0) s_wave[wv] = (uint32_t)__popcll(mk);
    __syncthreads();
    uint32_t pos = off[blockIdx.x];
    for (uint32_t x = 0; x < wv; x++) pos += s_wave[x];
    if (k) { w_out[pos + below] = weight; slot_out[pos + below] = i; }
}

// in place: the compacted weights become the CDF; *total <- W
__global__ __launch_bounds__(1024) void er_lights_cdf_kernel(float* __restrict__ cdf, uint32_t n, float* __restrict__ total) {
    __shared__ float s[1025];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (n + 1023u) / 1024u, lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    float sum = 0.0f;
    for (uint32_t i = lo; i < hi; i++) sum = sum + cdf[i];
    s[t + 1] = sum;
    __syncthreads();
    if (t == 0) {
        s[0] = 0.0f;
        for (uint32_t x = 1; x <= 1024u; x++) s[x] = s[x - 1] + s[x];
        *total = s[1024];
    }
    __syncthreads();
    const float W = s[1024];
    float run = s[t];
    for (uint32_t i = lo; i < hi; i++) { run = run + cdf[i]; cdf[i] = run / W; }
}

__global__ __launch_bounds__(256) void er_lights_prob_kernel(const float* __restrict__ w, uint32_t n, const float* __restrict__ total, float* __restrict__ prob) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) prob[i] = w[i] / *total;
}

__global__ __launch_bounds__(256) void er_lights_read_kernel(const float4* __restrict__ isect, const float* __restrict__ table, uint32_t tri_count,
                                                             uint32_t count, uint32_t m, int32_t* __restrict__ out, float* __restrict__ cdf_out,
                                                             float* __restrict__ prob_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const uint32_t slot = __builtin_bit_cast(uint32_t, table[(size_t)tri_count + count + i]);
    // (a slot that is none -- a table that a defect left unwritten -- is reported as triangle -1 and P NaN, not followed)
    out[i] = slot < tri_count ? __builtin_bit_cast(int32_t, isect[(size_t)slot * 3].w) : -1;
    cdf_out[i] = table[(size_t)tri_count + i];
    if (prob_out) prob_out[i] = slot < tri_count ? table[slot] : __builtin_nanf("");      // (P at the emitter's slot, what mesh_prob reads)
}

}  // namespace

hipError_t er_lights_build(const float4* isect, const float4* attr, uint32_t tri_count, const ErMaterial* materials, const DevTex* textures,
                           const float* tex_pool, const int32_t* emission_textures, uint32_t n_etex, uint32_t texture_count,
                           float** table, uint32_t* count, float* total, hipStream_t stream) {
    *table = nullptr;
    *count = 0;
    *total = 0.0f;
    if (tri_count == 0) return hipSuccess;
    const uint32_t nb = (tri_count + 1023u) / 1024u;
    // scratch: texture means, weights per slot, workgroup counts and offsets, W
    float *mean = nullptr, *w = nullptr, *d_total = nullptr;
    uint32_t *bc = nullptr, *off = nullptr;
    float* tab = nullptr;
    hipError_t e = hipSuccess;
    auto done = [&](hipError_t r) {
        (void)hipFree(mean); (void)hipFree(w); (void)hipFree(d_total); (void)hipFree(bc); (void)hipFree(off);
        if (r != hipSuccess) (void)hipFree(tab);
        else *table = tab;
        return r;
    };
    if ((e = hipMalloc((void**)&mean, sizeof(float) * (texture_count + 1))) != hipSuccess) return done(e);
    if ((e = hipMalloc((void**)&w, sizeof(float) * tri_count)) != hipSuccess) return done(e);
    if ((e = hipMalloc((void**)&d_total, sizeof(float))) != hipSuccess) return done(e);
    if ((e = hipMalloc((void**)&bc, sizeof(uint32_t) * nb)) != hipSuccess) return done(e);
    if ((e = hipMalloc((void**)&off, sizeof(uint32_t) * (nb + 1))) != hipSuccess) return done(e);
    if (n_etex) hipLaunchKernelGGL(er_lights_tex_mean_kernel, dim3(n_etex), dim3(256), 0, stream, textures, tex_pool, emission_textures, mean);
    hipLaunchKernelGGL(er_lights_weight_kernel, dim3(nb), dim3(1024), 0, stream, isect, attr, tri_count, materials, mean, w, bc);
    hipLaunchKernelGGL(er_lights_scan_kernel, dim3(1), dim3(1024), 0, stream, bc, nb, off);
    if ((e = hipGetLastError()) != hipSuccess) return done(e);
    uint32_t n = 0;
    if ((e = hipMemcpyAsync(&n, off + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, stream)) != hipSuccess) return done(e);
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return done(e);
    if (n == 0) return done(hipSuccess);
    if ((e = hipMalloc((void**)&tab, sizeof(float) * ((size_t)tri_count + 2 * (size_t)n))) != hipSuccess) return done(e);
    float* cdf = tab + tri_count;
    hipLaunchKernelGGL(er_lights_scatter_kernel, dim3(nb), dim3(1024), 0, stream, w, tri_count, off, cdf, (uint32_t*)(cdf + n));
    hipLaunchKernelGGL(er_lights_cdf_kernel, dim3(1), dim3(1024), 0, stream, cdf, n, d_total);
    hipLaunchKernelGGL(er_lights_prob_kernel, dim3((tri_count + 255u) / 256u), dim3(256), 0, stream, w, tri_count, d_total, tab);
    if ((e = hipGetLastError()) != hipSuccess) return done(e);
    if ((e = hipMemcpyAsync(total, d_total, sizeof(float), hipMemcpyDeviceToHost, stream)) != hipSuccess) return done(e);
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return done(e);
    *count = n;
    return done(hipSuccess);
}

void er_launch_light_table_read(const float4* isect, const float* table, uint32_t tri_count, uint32_t count, uint32_t cap,
                                int32_t* out, float* cdf_out, float* prob_out, hipStream_t stream) {
    const uint32_t m = count < cap ? count : cap;
    if (m == 0 || !table) return;
    hipLaunchKernelGGL(er_lights_read_kernel, dim3((m + 255u) / 256u), dim3(256), 0, stream, isect, table, tri_count, count, m, out, cdf_out, prob_out);
}
