// er_adaptive.hip -- adaptive sampling (include/eleven_hip.h er_adaptive_set): the per-tile convergence test and the compaction of
// the tiles that go on.  The render kernels are untouched: they are handed the compacted list of active tiles (er_api.cpp).
//
// A pixel's samples are one RNG stream and its planes a running mean, so a pixel that received k samples in an adaptive render
// is, bit for bit, the pixel of a uniform render of k samples: the test only decides WHICH tiles get more samples.
#include "er_adaptive.h"
#include "er_device.h"

// One wave per tile, one lane per pixel: BEAUTY rgb and the samples-plane value, compact [tile][64] (lanes outside the frame: zero).
__global__ __launch_bounds__(64) void er_adaptive_snapshot_kernel(DevScene S, const uint32_t* __restrict__ tiles, float4* __restrict__ snap) {
    const uint32_t lane = threadIdx.x, tile = tiles[blockIdx.x];
    const uint32_t px = (tile % S.tiles_x) * ER_TILE + (lane & 7u), py = (tile / S.tiles_x) * ER_TILE + (lane >> 3);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (px < S.x_res && py < S.y_res) {
        const size_t npx = (size_t)S.x_res * S.y_res, idx = (size_t)py * S.x_res + px;
        const float4 b = S.passes[er_pass_index(npx, ER_PASS_BEAUTY, idx)];
        v = make_float4(b.x, b.y, b.z, __builtin_bit_cast(float, S.samples[idx]));
    }
    snap[(size_t)blockIdx.x * 64 + lane] = v;
}

// The test of one tile, one lane per pixel.  m, M: samples-plane values at the snapshot and now (both count the setup's initial 1);
// S, I: BEAUTY rgb then and now.  I - S = ((M - m) / M) (J - S) for J the mean of the new samples, so its spread times sqrt(m / (M - m))
// is the standard error of I.  Exactly these IEEE float32 operations, in this order (-ffp-contract=off; tests/test_gpu_adaptive.py
// replays them in numpy, bit for bit):
//     f   = sqrtf((float)m / (float)(M - m))                       a pixel with M == m (every new sample NaN-gated) is not testable
//     d_c = (I_c - S_c) * f                                        c = R, G, B
//     e   = sqrtf((d_R * d_R + d_G * d_G) + d_B * d_B) / sqrtf(((1e-3f + I_R) + I_G) + I_B)
//     v   = e * e  (testable pixels of the frame; 0 elsewhere),  n = 1 (testable) or 0
//     v += shfl_xor(v, k), n += shfl_xor(n, k)  for k = 32, 16, 8, 4, 2, 1        (every lane ends with the same bits: + commutes)
//     E   = sqrtf(v / (float)n)
// The tile stays active iff n == 0 or E >= threshold; tile_error[tile] = E, or -1 if n == 0.
__global__ __launch_bounds__(64) void er_adaptive_test_kernel(DevScene S, const uint32_t* __restrict__ tiles, const float4* __restrict__ snap, float threshold,
                                                              float* __restrict__ tile_error, uint32_t* __restrict__ keep) {
    const uint32_t lane = threadIdx.x, tile = tiles[blockIdx.x];
    const uint32_t px = (tile % S.tiles_x) * ER_TILE + (lane & 7u), py = (tile / S.tiles_x) * ER_TILE + (lane >> 3);
    float v = 0.0f;
    uint32_t n = 0;
    if (px < S.x_res && py < S.y_res) {
        const size_t npx = (size_t)S.x_res * S.y_res, idx = (size_t)py * S.x_res + px;
        const float4 s = snap[(size_t)blockIdx.x * 64 + lane];
        const uint32_t m = __builtin_bit_cast(uint32_t, s.w), M = S.samples[idx];
        if (M > m) {
            const float4 I = S.passes[er_pass_index(npx, ER_PASS_BEAUTY, idx)];
            const float f = __builtin_sqrtf((float)m / (float)(M - m));
            const float dr = (I.x - s.x) * f, dg = (I.y - s.y) * f, db = (I.z - s.z) * f;
            const float e = __builtin_sqrtf(dr * dr + dg * dg + db * db) / __builtin_sqrtf(1e-3f + I.x + I.y + I.z);
            v = e * e;
            n = 1;
        }
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        v = v + __shfl_xor(v, k, 64);
        n = n + __shfl_xor(n, k, 64);
    }
    if (lane == 0) {
        const float E = n ? __builtin_sqrtf(v / (float)n) : -1.0f;
        tile_error[tile] = E;
        keep[blockIdx.x] = (n == 0 || E >= threshold) ? 1u : 0u;
    }
}

// One workgroup of 16 waves compacts the kept tiles, 1024 at a time: a ballot and mbcnt give a tile's place among the kept tiles of
// its wave, a prefix over the 16 waves' counts (LDS) its wave's place in the chunk, a running base the chunk's place in the list.
// The input is in ascending tile order and so is the output.  Also the largest error among the kept tiles (a max: any order).
__global__ __launch_bounds__(1024) void er_adaptive_compact_kernel(const uint32_t* __restrict__ in, const uint32_t* __restrict__ keep, const float* __restrict__ tile_error,
                                                                   uint32_t* __restrict__ out) {
    __shared__ uint32_t s_wave[16];
    __shared__ float s_max[16];
    __shared__ uint32_t s_base;
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t count = in[0];
    const uint32_t* tiles = in + ER_AD_LIST;
    if (t == 0) s_base = 0;
    float mx = -1.0f;
    __syncthreads();
    for (uint32_t c = 0; c < count; c += 1024u) {
        const uint32_t i = c + t;
        const bool k = i < count && keep[i] != 0u;
        const uint32_t tile = k ? tiles[i] : 0u;
        if (k) mx = fmaxf(mx, tile_error[tile]);
        const unsigned long long m = __ballot(k);
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (lane == 0) s_wave[w] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = s_base;
        for (uint32_t x = 0; x < w; x++) off += s_wave[x];
        if (k) out[ER_AD_LIST + off + below] = tile;
        __syncthreads();
        if (t == 0) {
            uint32_t sum = 0;
            for (uint32_t x = 0; x < 16u; x++) sum += s_wave[x];
            s_base += sum;
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) mx = fmaxf(mx, __shfl_xor(mx, k, 64));
    if (lane == 0) s_max[w] = mx;
    __syncthreads();
    if (t == 0) {
        float r = s_max[0];
        for (uint32_t x = 1; x < 16u; x++) r = fmaxf(r, s_max[x]);
        out[0] = s_base;
        out[1] = __builtin_bit_cast(uint32_t, r);
    }
}

void er_launch_adaptive_snapshot(const DevScene& S, const uint32_t* list, uint32_t count, float4* snap, hipStream_t stream) {
    if (count == 0) return;
    hipLaunchKernelGGL(er_adaptive_snapshot_kernel, dim3(count), dim3(64), 0, stream, S, list + ER_AD_LIST, snap);
}

void er_launch_adaptive_test(const DevScene& S, const uint32_t* list, uint32_t count, const float4* snap, float threshold, float* tile_error,
                             uint32_t* keep, uint32_t* out, hipStream_t stream) {
    if (count > 0) hipLaunchKernelGGL(er_adaptive_test_kernel, dim3(count), dim3(64), 0, stream, S, list + ER_AD_LIST, snap, threshold, tile_error, keep);
    hipLaunchKernelGGL(er_adaptive_compact_kernel, dim3(1), dim3(1024), 0, stream, list, keep, tile_error, out);
}
