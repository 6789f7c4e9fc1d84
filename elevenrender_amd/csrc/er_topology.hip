// er_topology.hip -- the geometry store of er_render_topology (er_topology.h): the scene's six arrays on the device in id order, and the
// compaction that follows a topology edit: mark the removed ids in a keep array, scan it, gather the survivors of every array in order.
// The pattern is er_ids.hip's mark / scan / ordered write, with rocprim's exclusive scan as in er_gpu_build.hip.  Every array is a
// stream of 32-bit words (9, 9, 9, 6, 1, 1 per triangle): the kernels copy words and do no floating-point arithmetic, every output
// word has exactly one writer, and the grids are bounded (grid-stride loops).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>     // (before rocprim: its texture iterator calls the host memset)
#include <string>

#include <rocprim/rocprim.hpp>

#include "er_topology.h"

namespace {

const unsigned TOPO_BLOCK = 256, TOPO_MAX_BLOCKS = 256 * 32;      // a bounded grid whatever the size: 8192 blocks, the rest by the loops' stride

inline unsigned topo_blocks(size_t items) { return (unsigned)std::max<size_t>(1, std::min<size_t>((items + TOPO_BLOCK - 1) / TOPO_BLOCK, TOPO_MAX_BLOCKS)); }

__global__ __launch_bounds__(256) void k_topo_keep_all(uint32_t* __restrict__ keep, uint32_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) keep[i] = 1u;
}

// the removed ids are distinct (er_topo_check): one writer per word
__global__ __launch_bounds__(256) void k_topo_mark(uint32_t* __restrict__ keep, uint32_t n, const uint32_t* __restrict__ ids, uint32_t count) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t id = ids[i];
        if (id < n) keep[id] = 0u;
    }
}

// the ordered gather of one stream of W words per triangle: survivor i goes to row offset[i] (the exclusive scan of keep)
template <unsigned W>
__global__ __launch_bounds__(256) void k_topo_gather(const uint32_t* __restrict__ src, uint32_t n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ offset,
                                                     uint32_t* __restrict__ dst, uint32_t survivors) {
    const size_t words = (size_t)n * W;
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (size_t)gridDim.x * blockDim.x) {
        const size_t i = w / W, k = w % W;
        if (!keep[i]) continue;
        const uint32_t to = offset[i];
        if (to < survivors) dst[(size_t)to * W + k] = src[w];
    }
}

template <class T>
struct Dev {
    T* p = nullptr;
    Dev() = default;
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { if (p) (void)hipFree(p); }
};

struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

#define TP_OK(x)                                                                                     \
    do {                                                                                             \
        hipError_t e_ = (x);                                                                         \
        if (e_ != hipSuccess) {                                                                      \
            why = std::string(#x) + ": " + hipGetErrorString(e_);                                    \
            rc = e_ == hipErrorOutOfMemory ? -2 : -1;                                                \
            goto done;                                                                               \
        }                                                                                            \
    } while (0)

// six buffers for n triangles (at least one element each, so that no pointer is null)
int store_alloc(ErGeomStore& s, uint32_t n, std::string& why) {
    const size_t m = std::max<uint32_t>(n, 1u);
    int rc = 0;
    TP_OK(hipMalloc((void**)&s.vertices, m * 36));
    TP_OK(hipMalloc((void**)&s.normals, m * 36));
    TP_OK(hipMalloc((void**)&s.tangents, m * 36));
    TP_OK(hipMalloc((void**)&s.uvs, m * 24));
    TP_OK(hipMalloc((void**)&s.tangent_sign, m * 4));
    TP_OK(hipMalloc((void**)&s.material_id, m * 4));
    s.count = n;
done:
    if (rc != 0) { (void)hipGetLastError(); s.release(); }
    return rc;
}

// `count` rows of the host arrays `h` to row `at` of the store
int store_upload(ErGeomStore& s, uint32_t at, const ErGpuSceneArrays& h, uint32_t count, hipStream_t st, std::string& why) {
    int rc = 0;
    if (count == 0) return 0;
    TP_OK(hipMemcpyAsync(s.vertices + (size_t)at * 9, h.vertices, (size_t)count * 36, hipMemcpyHostToDevice, st));
    TP_OK(hipMemcpyAsync(s.normals + (size_t)at * 9, h.normals, (size_t)count * 36, hipMemcpyHostToDevice, st));
    TP_OK(hipMemcpyAsync(s.tangents + (size_t)at * 9, h.tangents, (size_t)count * 36, hipMemcpyHostToDevice, st));
    TP_OK(hipMemcpyAsync(s.uvs + (size_t)at * 6, h.uvs, (size_t)count * 24, hipMemcpyHostToDevice, st));
    TP_OK(hipMemcpyAsync(s.tangent_sign + at, h.tangent_sign, (size_t)count * 4, hipMemcpyHostToDevice, st));
    TP_OK(hipMemcpyAsync(s.material_id + at, h.material_id, (size_t)count * 4, hipMemcpyHostToDevice, st));
done:
    return rc;
}

}  // namespace

void ErGeomStore::release() {
    if (vertices) (void)hipFree(vertices);
    if (normals) (void)hipFree(normals);
    if (tangents) (void)hipFree(tangents);
    if (uvs) (void)hipFree(uvs);
    if (tangent_sign) (void)hipFree(tangent_sign);
    if (material_id) (void)hipFree(material_id);
    vertices = normals = tangents = uvs = tangent_sign = nullptr;
    material_id = nullptr;
    count = 0;
    valid = false;
}

hipError_t er_probe_topology(const char** which) {
    hipFuncAttributes at;
    *which = "k_topo_mark (er_topology.hip)";
    return hipFuncGetAttributes(&at, (const void*)k_topo_mark);
}

int er_store_fill(ErGeomStore& s, const ErGpuSceneArrays& host, uint32_t n, hipStream_t st, uint64_t* bytes, std::string& why) {
    int rc = 0;
    s.release();
    if ((rc = store_alloc(s, n, why)) != 0) return rc;
    if ((rc = store_upload(s, 0, host, n, st, why)) != 0) goto done;
    TP_OK(hipStreamSynchronize(st));
    s.valid = true;
    *bytes = (uint64_t)n * ER_STORE_BYTES_PER_TRI;
done:
    if (rc != 0) { (void)hipGetLastError(); s.release(); }
    return rc;
}

int er_store_edit(ErGeomStore& s, uint32_t remove_count, const uint32_t* remove_ids, uint32_t append_count, const ErGpuSceneArrays& appended, hipStream_t st,
                  uint64_t* bytes, float* ms, std::string& why) {
    int rc = 0;
    const uint32_t n = s.count, survivors = n - remove_count, total = survivors + append_count;
    ErGeomStore out;
    Dev<uint32_t> d_keep, d_off, d_ids;
    Dev<char> d_tmp;
    Events ev;
    *bytes = 0;
    *ms = 0;
    if (!s.valid || remove_count > n) { why = "the geometry store is not valid for this edit"; rc = -1; goto done; }
    if ((rc = store_alloc(out, total, why)) != 0) goto done;
    TP_OK(hipEventCreate(&ev.a));
    TP_OK(hipEventCreate(&ev.b));
    if (remove_count && survivors) {
        size_t tmp_bytes = 0;
        TP_OK(hipMalloc((void**)&d_keep.p, (size_t)n * 4));
        TP_OK(hipMalloc((void**)&d_off.p, (size_t)n * 4));
        TP_OK(hipMalloc((void**)&d_ids.p, (size_t)remove_count * 4));
        TP_OK(rocprim::exclusive_scan(nullptr, tmp_bytes, d_keep.p, d_off.p, 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
        TP_OK(hipMalloc((void**)&d_tmp.p, tmp_bytes ? tmp_bytes : 16));
        TP_OK(hipMemcpyAsync(d_ids.p, remove_ids, (size_t)remove_count * 4, hipMemcpyHostToDevice, st));
        TP_OK(hipEventRecord(ev.a, st));
        hipLaunchKernelGGL(k_topo_keep_all, dim3(topo_blocks(n)), dim3(TOPO_BLOCK), 0, st, d_keep.p, n);
        hipLaunchKernelGGL(k_topo_mark, dim3(topo_blocks(remove_count)), dim3(TOPO_BLOCK), 0, st, d_keep.p, n, d_ids.p, remove_count);
        TP_OK(rocprim::exclusive_scan(d_tmp.p, tmp_bytes, d_keep.p, d_off.p, 0u, (size_t)n, rocprim::plus<uint32_t>(), st));
        hipLaunchKernelGGL(k_topo_gather<9>, dim3(topo_blocks((size_t)n * 9)), dim3(TOPO_BLOCK), 0, st, (const uint32_t*)s.vertices, n, d_keep.p, d_off.p, (uint32_t*)out.vertices, survivors);
        hipLaunchKernelGGL(k_topo_gather<9>, dim3(topo_blocks((size_t)n * 9)), dim3(TOPO_BLOCK), 0, st, (const uint32_t*)s.normals, n, d_keep.p, d_off.p, (uint32_t*)out.normals, survivors);
        hipLaunchKernelGGL(k_topo_gather<9>, dim3(topo_blocks((size_t)n * 9)), dim3(TOPO_BLOCK), 0, st, (const uint32_t*)s.tangents, n, d_keep.p, d_off.p, (uint32_t*)out.tangents, survivors);
        hipLaunchKernelGGL(k_topo_gather<6>, dim3(topo_blocks((size_t)n * 6)), dim3(TOPO_BLOCK), 0, st, (const uint32_t*)s.uvs, n, d_keep.p, d_off.p, (uint32_t*)out.uvs, survivors);
        hipLaunchKernelGGL(k_topo_gather<1>, dim3(topo_blocks(n)), dim3(TOPO_BLOCK), 0, st, (const uint32_t*)s.tangent_sign, n, d_keep.p, d_off.p, (uint32_t*)out.tangent_sign, survivors);
        hipLaunchKernelGGL(k_topo_gather<1>, dim3(topo_blocks(n)), dim3(TOPO_BLOCK), 0, st, (const uint32_t*)s.material_id, n, d_keep.p, d_off.p, (uint32_t*)out.material_id, survivors);
        TP_OK(hipGetLastError());
    } else {
        TP_OK(hipEventRecord(ev.a, st));
        if (survivors) {      // nothing removed: the arrays move over as they are
            TP_OK(hipMemcpyAsync(out.vertices, s.vertices, (size_t)n * 36, hipMemcpyDeviceToDevice, st));
            TP_OK(hipMemcpyAsync(out.normals, s.normals, (size_t)n * 36, hipMemcpyDeviceToDevice, st));
            TP_OK(hipMemcpyAsync(out.tangents, s.tangents, (size_t)n * 36, hipMemcpyDeviceToDevice, st));
            TP_OK(hipMemcpyAsync(out.uvs, s.uvs, (size_t)n * 24, hipMemcpyDeviceToDevice, st));
            TP_OK(hipMemcpyAsync(out.tangent_sign, s.tangent_sign, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
            TP_OK(hipMemcpyAsync(out.material_id, s.material_id, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        }
    }
    TP_OK(hipEventRecord(ev.b, st));
    if ((rc = store_upload(out, survivors, appended, append_count, st, why)) != 0) goto done;
    TP_OK(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(ms, ev.a, ev.b);
    *bytes = (uint64_t)remove_count * 4 + (uint64_t)append_count * ER_STORE_BYTES_PER_TRI;
    s.release();
    s = out;      // (a plain struct of pointers: `out` is not released below)
    s.valid = true;
    out = ErGeomStore{};
done:
    if (rc != 0) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(st);      // nothing in flight reads what is freed here
        out.release();
        s.release();
    }
    return rc;
}
