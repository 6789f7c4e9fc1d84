// er_texstage.h -- the texture stage on the device (er_texstage.hip; er_render_edit, er_api_edit.cpp): the pool of a texture plan
// (er_texplan.h) filled by copies and kernels instead of by the host loops of er_render_begin.  Same layout, same bytes.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <string>

#include "er_texplan.h"

struct ErTexSource {      // a texture's texels on the host: width x height x channels floats (the plan's table holds a compacted
    const float* data;    // texture with ONE channel; the upload needs the channels of the array)
    int32_t width, height, channels;
};

// Builds the pool of `plan` in a NEW device buffer (*pool_out, max(1, plan.pool_floats) floats, hipMalloc'd: the caller owns it) from
// the host texels `tex[ntex]` (in the order of the plan's table) and `hdri`.  Enqueues on `stream`, waits for it, releases its staging
// buffer.  *ms = device time of the stage (HIP events on `stream`: first upload to last kernel).
// Returns 0; -2 = out of device memory, -1 = any other HIP error (`err` says which).  plan.pool_floats must be below 2^32.
int er_texstage_build(const erh::TexPlan& plan, const ErTexSource* tex, size_t ntex, const ErMaterial* mats, size_t nmat, const ErTexSource& hdri,
                      hipStream_t stream, float** pool_out, float* ms, std::string& err);

// attr[slot].material = material_id[isect[slot].tri_id] for every slot < tri_count; `isect` at 3 pieces and `attr` at ER_ATTR_PIECES
// pieces of 16 bytes per slot, `material_id` (device) per input triangle.  Enqueues on `stream`.
void er_launch_material_ids(const float4* isect, float4* attr, uint32_t tri_count, const int32_t* material_id, hipStream_t stream);

hipError_t er_probe_texstage(const char** which);   // see er_kernels.h
