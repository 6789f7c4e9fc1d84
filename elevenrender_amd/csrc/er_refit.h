// er_refit.h -- device refit of a built acceleration structure after its triangles moved (er_refit.hip; er_render_update, er_api_edit.cpp).
// The topology stays -- child references, slot assignment, triangle order --; the triangle records, every box of the binary tree and
// every wide node's origin, exponents and quantised child boxes are recomputed from the new arrays, bottom-up, one launch per tree level.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "er_bvh.h"

// Per topology: the nodes of either tree by level, as index lists on the device (level L of a tree = entries [off[L], off[L + 1])).
// Derived at the first refit after an er_render_begin, kept until the next one.
struct ErRefitTopo {
    bool valid = false;
    uint32_t* d_lv2 = nullptr;      // binary nodes, by depth
    uint32_t* d_lv8 = nullptr;      // wide nodes, by depth
    std::vector<uint32_t> off2, off8;
    void release() {
        if (d_lv2) (void)hipFree(d_lv2);
        if (d_lv8) (void)hipFree(d_lv8);
        d_lv2 = d_lv8 = nullptr;
        off2.clear(); off8.clear();
        valid = false;
    }
};

struct ErRefitBuffers {             // the structure as the kernels read it, whichever builder made it
    ErNode* nodes = nullptr;        // binary tree
    uint32_t node_count = 0, depth2 = 0;
    float4* nodes8 = nullptr;       // wide nodes at a stride of ER_NODE8_PIECES pieces
    uint32_t node8_count = 0, depth8 = 0;
    ErTriIsect* isect = nullptr;    // tri_count + 1 records in slot order
    ErTriAttr* attr = nullptr;
    uint32_t tri_count = 0;
};

struct ErRefitArrays {              // host arrays per original triangle, [n][3][3] each
    const float* vertices = nullptr;
    const float* normals = nullptr;      // the scene's current normals (the lift bound needs them either way) ...
    bool write_normals = false;          // ... written into the attribute records only if they are new
    const float* tangents = nullptr;     // NULL = keep
};

struct ErRefitResult {
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, lift_bound = 0;
    float refit_ms = 0;             // device time from the first upload to the last level's kernel (HIP events on `stream`)
};

// Returns 0; -2 = out of device memory, -1 = any other HIP error or a guard of the refit itself (`err` says which).  Blocks until done.
int er_refit_device(ErRefitTopo& topo, const ErRefitBuffers& b, const ErRefitArrays& a, hipStream_t stream, ErRefitResult* out, std::string& err);
hipError_t er_probe_refit(const char** which);   // see er_kernels.h
