// er_api_stages.h -- the stages of er_render_begin (er_api.cpp) that an edit in place (er_api_edit.cpp) runs again, and their staging.
// Internal to the two files.  er_scene.h, included here, has what every translation unit of the boundary shares: fail, guarded,
// HIP_TRY, EventPair, upload.  Every stage is called with the scene's mutex held and the device set, takes what earlier stages left
// from the scene (ErScene::kept) and reports a failure under `who`, the entry point that was called.
#pragma once
#include "er_scene.h"
#include "er_hdri_trig.h"

namespace erh {

// Staging buffers of the asynchronous uploads.  They live in the frame of the entry point, not in the stages', until the stream has
// been synchronised at its end (HIP happens to make pageable host-to-device copies host-synchronous; this code does not rely on it).
struct BeginStaging {
    ErBvhBuild bvh;
    std::vector<ErTriIsect> isect;
    std::vector<ErTriAttr> attr;
    std::vector<float4> geom, mat_pre;
    std::vector<DevTex> table;
    std::vector<float> pool;
    std::vector<DevFused> fused;
    std::vector<uint32_t> guide, owned;
    std::vector<int32_t> etex;      // ER_FLAG_MESH_LIGHTS: the textures that emit
    StreamDeal deal;      // the owned share dealt to the CUs: what the schedule is chosen on, and what the streaming schedule starts with
};

// a texture pool's offsets are 32-bit
inline int check_pool_floats(uint64_t floats, const char* who) {
    return floats >= (1ull << 32) ? fail(ER_ERR_INVALID_ARG, std::string(who) + ": texture pool exceeds 2^32 floats") : ER_OK;
}

// stage 2: the acceleration structure of the host copy into the scene's three buffers, described in s->kept.accel; `built_ev` is
// recorded when the tree is there and the uploads begin.  accel_publish: what er_accel_info and er_debug_read_accel report of it.
// `device_arrays` (er_render_topology's geometry store): the scene's six arrays as they already lie on the device -- the device
// builder, where it is the one chosen, reads them instead of uploading the host copy; everything else is the same.
int begin_accel(ErScene* s, BeginStaging& B, hipEvent_t built_ev, const char* who, const ErGpuSceneArrays* device_arrays = nullptr);
// whether begin_accel would ask the device builder first, for the scene as it is now (flags, environment, thresholds)
bool accel_device_first(const ErScene* s);
void accel_publish(ErScene* s, float up_ms);
// stage 3 without the point lights: the materials and their precomputed constants
int upload_materials(ErScene* s, BeginStaging& B);
// the HDRI's search guide and, behind it, its row and column tables (er_hdri_trig.h) for the descriptor s->kept.hdri: the end of the
// texture stage, and of an edit's pool stage when the HDRI changes
int upload_hdri_guide(ErScene* s, BeginStaging& B);
// the scene's host textures as the texture plan (er_texplan.h) takes them
void plan_of_scene(const ErScene* s, TexPlan& P);
// stage 5, ER_FLAG_MESH_LIGHTS: the emitter table from the placed triangle records, materials and texture pool
int begin_emitters(ErScene* s, BeginStaging& B, const char* who);
// stages 6-8 and the set-up launch: the render's own state -- planes, schedule, descriptor -- on a structure, materials and textures that
// are in place (s->kept says where).  `uploads_done` (may be null) is recorded before the descriptor goes up.  Leaves the stream idle.
int begin_render_state(ErScene* s, BeginStaging& B, hipEvent_t uploads_done);

}  // namespace erh
