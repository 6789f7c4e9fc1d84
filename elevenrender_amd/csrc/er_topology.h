// er_topology.h -- the device-resident geometry store of er_render_topology and its compaction (er_topology.hip).
// The store is the scene's six arrays on the device in id order, 140 bytes per triangle, in the layout the device builder reads
// (er_gpu_build.h ErGpuSceneArrays with device pointers: er_gpu_build_device_arrays).  A topology edit that finds it valid gathers the
// survivors of all six arrays in order (er_topology_host.h: the numbering) into buffers sized for the new count and uploads only the
// appended rows to their tail:
//     bytes_uploaded = 4 x remove_count + 140 x append_count          (path 1: nothing of it depends on tri_count)
// A fill from the host copy uploads 140 x tri_count (path 2).  The kernels move 32-bit words and compute nothing in floating point; the
// only atomics-free scatter has one writer per word (the removed ids are distinct: er_topo_check).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <string>

#include "er_gpu_build.h"

#define ER_STORE_BYTES_PER_TRI 140u      // 3 x 36 (vertices, normals, tangents) + 24 (uvs) + 4 (tangent_sign) + 4 (material_id)

struct ErGeomStore {
    float *vertices = nullptr, *normals = nullptr, *tangents = nullptr, *uvs = nullptr, *tangent_sign = nullptr;
    int32_t* material_id = nullptr;
    uint32_t count = 0;
    bool valid = false;
    ErGpuSceneArrays arrays() const { return ErGpuSceneArrays{vertices, normals, tangents, uvs, tangent_sign, material_id}; }
    void release();      // (the caller has made the scene's stream idle, or the store was never read asynchronously)
};

// Both return 0, -2 (out of device memory) or -1 (any other HIP error) with the reason in `why`; on failure the store is released.
// They leave `st` idle.  *bytes: host-to-device bytes; *ms: device time of the compaction (HIP events; 0 for a fill).
int er_store_fill(ErGeomStore& s, const ErGpuSceneArrays& host, uint32_t n, hipStream_t st, uint64_t* bytes, std::string& why);
// remove_ids: [remove_count] distinct ids below s.count (host memory); appended: host arrays of append_count triangles
int er_store_edit(ErGeomStore& s, uint32_t remove_count, const uint32_t* remove_ids, uint32_t append_count, const ErGpuSceneArrays& appended, hipStream_t st,
                  uint64_t* bytes, float* ms, std::string& why);
hipError_t er_probe_topology(const char** which);      // as er_probe_kernels (er_kernels.h)
