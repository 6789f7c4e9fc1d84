// er_refit.h -- device refit of a built acceleration structure after its triangles moved (er_refit.hip; er_render_update, er_api_edit.cpp).
// The topology stays -- child references, slot assignment, triangle order --; the triangle records, every box of the binary tree and
// every wide node's origin, exponents and quantised child boxes are recomputed from the new arrays, bottom-up, one launch per tree level.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "er_bvh.h"
#include "er_sparse_host.h"      // ErSparseList: the listed triangles of er_render_update_sparse, already checked
#include "er_xform.h"            // ErXformEntry, ErObjectTable: the listed objects of er_render_transform, already checked
#include "er_skin.h"             // ErSkinEntry, ErSkinTable: the listed objects of er_render_skin, already checked

// Per topology: the nodes of either tree by level, as index lists on the device (level L of a tree = entries [off[L], off[L + 1])),
// and what the sparse refit needs to find its way UP from a triangle: the slot of every triangle id, the binary and the wide node that
// hold each slot, and every node's parent (0xffffffff: none).  Each target has one writer, because the structure is a tree.
// Derived at the first refit after an er_render_begin, kept until the next one.
// Kept boxes: every refit, full or sparse, leaves the per-slot padded boxes (six floats each), the per-slot term of the lift maximum and
// the per-wide-node float boxes here (the float boxes cannot be recovered from the quantised nodes, and a requantised parent needs its
// clean children's exact boxes to reproduce the full refit's bytes).  They describe the structure only after a refit has filled them
// (`boxes_valid`), under the largest |coordinate| they were padded with (`vmax_bits`).
// The dirty marks hold the epoch of the sparse refit that set them, so nothing is cleared between calls.
struct ErRefitTopo {
    bool valid = false;
    uint32_t* d_lv2 = nullptr;      // binary nodes, by depth
    uint32_t* d_lv8 = nullptr;      // wide nodes, by depth
    std::vector<uint32_t> off2, off8;
    uint32_t *d_slot_of = nullptr, *d_leaf2 = nullptr, *d_leaf8 = nullptr;      // [tri_count] each
    uint32_t *d_par2 = nullptr, *d_mark2 = nullptr;                               // [node_count]
    uint32_t *d_par8 = nullptr, *d_mark8 = nullptr;                               // [node8_count]
    float *d_sbox = nullptr, *d_slift = nullptr, *d_nbox = nullptr;               // [tri_count][6], [tri_count], [node8_count][6]
    bool boxes_valid = false;
    uint32_t vmax_bits = 0, epoch = 0;
    void release() {
        void* all[] = {d_lv2, d_lv8, d_slot_of, d_leaf2, d_leaf8, d_par2, d_mark2, d_par8, d_mark8, d_sbox, d_slift, d_nbox};
        for (void* q : all) if (q) (void)hipFree(q);
        d_lv2 = d_lv8 = d_slot_of = d_leaf2 = d_leaf8 = d_par2 = d_mark2 = d_par8 = d_mark8 = nullptr;
        d_sbox = d_slift = d_nbox = nullptr;
        off2.clear(); off8.clear();
        valid = boxes_valid = false;
        vmax_bits = epoch = 0;
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

struct ErSparseResult {
    ErRefitResult refit;
    uint32_t path = 0, why_full = 0;     // ErSparseInfo's
    uint32_t dirty_nodes2 = 0, dirty_nodes8 = 0;
    uint64_t bytes_uploaded = 0;
};

// Returns 0; -2 = out of device memory, -1 = any other HIP error or a guard of the refit itself (`err` says which).  Blocks until done.
int er_refit_device(ErRefitTopo& topo, const ErRefitBuffers& b, const ErRefitArrays& a, hipStream_t stream, ErRefitResult* out, std::string& err);
// The same structure as er_refit_device of the complete arrays would leave, byte for byte, from the listed triangles alone.
int er_refit_sparse(ErRefitTopo& topo, const ErRefitBuffers& b, const ErSparseList& a, hipStream_t stream, ErSparseResult* out, std::string& err);

// The object table of er_objects_set on the device, built at the first er_render_transform after it or after an er_render_begin: the
// rest pose of every listed triangle in CSR order as SEVEN 16-byte pieces -- 27 floats (vertices, normals, tangents) and the triangle's
// id in the last word -- piece-major: piece p of CSR position j lies at d_rest[p * total + j], so the 64 lanes of a wave load 1 KiB
// of consecutive bytes per piece.  112 bytes per listed triangle (108 of pose + the id, no padding) + 4 bytes per object for `first`.
struct ErXformDev {
    bool valid = false;
    float4* d_rest = nullptr;        // [7][total]
    uint32_t* d_first = nullptr;     // [objects + 1]
    uint32_t total = 0, objects = 0;
    void release() {
        if (d_rest) (void)hipFree(d_rest);
        if (d_first) (void)hipFree(d_first);
        d_rest = nullptr; d_first = nullptr;
        total = objects = 0;
        valid = false;
    }
};
constexpr uint32_t ER_XFORM_PIECES = 7;

struct ErXformCall {                 // one er_render_transform: the listed objects' entries (host) over the device-resident table
    const ErXformDev* table = nullptr;
    uint32_t entries = 0;
    const ErXformEntry* list = nullptr;
    uint32_t moved = 0;              // triangles of the listed objects
};

// `dev` from the host table (one upload of 112 bytes per listed triangle).  Blocks until done.  Returns as er_refit_device.
int er_xform_table_build(ErXformDev& dev, const ErObjectTable& t, hipStream_t stream, std::string& err);
// er_refit_sparse with the listed triangles posed ON THE DEVICE from the rest copy (k_xform_scatter): nothing but the entries is uploaded.
// The same structure, byte for byte, as er_refit_sparse given the listed objects' ids with their posed vertices, normals and tangents.
int er_refit_xform(ErRefitTopo& topo, const ErRefitBuffers& b, const ErXformCall& x, hipStream_t stream, ErSparseResult* out, std::string& err);

// The influences of er_skin_set on the device, beside the rest copy, built at the first er_render_skin after an er_skin_set or an
// er_render_begin: the rows of the SKINNED objects only, in object order (ErSkinTable::row_first), 72 bytes per triangle as six pieces,
// piece-major like the rest copy -- corner c of row r has its four weights at d_w[c * rows + r] (16 bytes) and its four 16-bit bone
// indices at d_b[c * rows + r] (8 bytes, as they lie in the caller's array: bone k in the low or high half, by k & 1, of word k / 2) --
// so the 64 lanes of a wave load 1 KiB and 512 consecutive bytes per piece.
struct ErSkinDev {
    bool valid = false;
    float4* d_w = nullptr;           // [3][rows]
    uint2* d_b = nullptr;            // [3][rows]
    uint32_t rows = 0;
    void release() {
        if (d_w) (void)hipFree(d_w);
        if (d_b) (void)hipFree(d_b);
        d_w = nullptr; d_b = nullptr;
        rows = 0;
        valid = false;
    }
};

struct ErSkinCall {                  // one er_render_skin: the listed objects' entries and palettes (host) over the two device tables
    const ErXformDev* table = nullptr;
    const ErSkinDev* skin = nullptr;
    uint32_t entries = 0;
    const ErSkinEntry* list = nullptr;
    uint32_t bones = 0;              // matrices in `palette`: the listed objects' bone counts added up
    const float* palette = nullptr;  // [bones][12]
    uint32_t moved = 0;              // triangles of the listed objects
};

// `dev` from the host tables (one upload of 72 bytes per triangle of a skinned object; *bytes gets that figure).  Blocks until done.
int er_skin_table_build(ErSkinDev& dev, const ErObjectTable& t, const ErSkinTable& k, hipStream_t stream, uint64_t* bytes, std::string& err);
// er_refit_sparse with the listed triangles skinned ON THE DEVICE from the rest copy (k_skin_scatter): 32 bytes per listed object and 48
// per listed bone are uploaded.  The same structure, byte for byte, as er_refit_sparse given the listed objects' ids with their posed
// vertices, normals and tangents.
int er_refit_skin(ErRefitTopo& topo, const ErRefitBuffers& b, const ErSkinCall& x, hipStream_t stream, ErSparseResult* out, std::string& err);
hipError_t er_probe_skin(const char** which);
hipError_t er_probe_refit(const char** which);          // see er_kernels.h
hipError_t er_probe_xform(const char** which);
hipError_t er_probe_refit_sparse(const char** which);
