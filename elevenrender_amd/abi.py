"""ctypes mirror of include/eleven_hip.h and loader of libeleven_hip.so.

The library is the product; this module only declares its C ABI for Python callers
(tests, bench.py, the Python host mirror in render.py).  There is no fallback: if the
shared library is missing, `load()` raises -- build it with `python -c "import
__graft_entry__ as g; g.build()"` or `make -C elevenrender_amd/csrc`.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ELEVEN_HIP_LIB: load another build of the same library (tools/sanitize_cpu.sh points it at the ASan + UBSan build)
LIB_PATH = os.environ.get("ELEVEN_HIP_LIB") or os.path.join(_HERE, "libeleven_hip.so")

ER_OK = 0
ER_ERR_INVALID_ARG, ER_ERR_NO_DEVICE, ER_ERR_HIP, ER_ERR_STATE, ER_ERR_OOM = -1, -2, -3, -4, -5
PASS_BEAUTY, PASS_DENOISE, PASS_NORMAL, PASS_TANGENT, PASS_BITANGENT, PASS_COUNT = 0, 1, 2, 3, 4, 5
PASS_NAMES = {"beauty": 0, "denoise": 1, "normal": 2, "tangent": 3, "bitangent": 4}
FLAG_POINT_LIGHTS, FLAG_COUNTERS, FLAG_MEGAKERNEL, FLAG_PROFILE, FLAG_FUSED, FLAG_WAVEFRONT, FLAG_GPU_BUILD, FLAG_MIS, FLAG_STREAM = 1, 2, 4, 8, 16, 32, 64, 128, 256
FLAG_HOST_BUILD = 512
FLAG_MESH_LIGHTS = 1024     # next-event estimation of emissive triangles (csrc/er_shade.h)
MAX_BOUNCES = 65535         # ER_MAX_BOUNCES: er_render_begin refuses a larger ErRenderParams.max_bounces
UPDATE_CAMERA, UPDATE_GEOMETRY = 1, 2     # ErSceneUpdate.what
EDIT_CAMERA, EDIT_GEOMETRY, EDIT_MATERIALS, EDIT_TEXTURES, EDIT_HDRI = 1, 2, 4, 8, 16     # ErSceneEdit.what
REBUILD_NEVER, REBUILD_ALWAYS, REBUILD_AUTO = 0, 1, 2     # ErUpdatePolicy.mode
TOPO_REMOVE, TOPO_APPEND = 1, 2     # ErTopologyEdit.what
FEATURE_ALBEDO, FEATURE_DEPTH, FEATURE_COUNT = 0, 1, 2     # er_render_features (csrc/er_features.hip)
FEATURE_NAMES = {"albedo": 0, "depth": 1}
ID_NONE, ID_SLOTS = 0xFFFFFFFF, 4     # er_render_ids (csrc/er_ids.hip)
ID_TRIANGLE, ID_OBJECT, ID_MATERIAL, ID_KIND_COUNT = 0, 1, 2, 3
ID_KIND_NAMES = {"triangle": 0, "object": 1, "material": 2}


class ErVec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class ErCamera(C.Structure):
    _fields_ = [("focal_length", C.c_float), ("sensor_width", C.c_float), ("sensor_height", C.c_float),
                ("aperture", C.c_float), ("focus_distance", C.c_float), ("rotation", ErVec3),
                ("bokeh", C.c_int32), ("position", ErVec3)]


class ErMaterial(C.Structure):
    _fields_ = [("albedo_tex", C.c_int32), ("emission_tex", C.c_int32), ("roughness_tex", C.c_int32),
                ("metallic_tex", C.c_int32), ("normal_tex", C.c_int32), ("opacity_tex", C.c_int32),
                ("transmission_tex", C.c_int32), ("albedo_shader_id", C.c_int32),
                ("albedo", ErVec3), ("emission", ErVec3),
                ("opacity", C.c_float), ("roughness", C.c_float), ("metallic", C.c_float),
                ("clearcoat_gloss", C.c_float), ("clearcoat", C.c_float), ("anisotropic", C.c_float),
                ("eta", C.c_float), ("transmission", C.c_float), ("specular", C.c_float),
                ("specular_tint", C.c_float), ("sheen_tint", C.c_float), ("subsurface", C.c_float),
                ("sheen", C.c_float), ("ax", C.c_float), ("ay", C.c_float)]


class ErTexture(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("filter", C.c_int32),
                ("data", C.POINTER(C.c_float))]


class ErHdri(C.Structure):
    _fields_ = [("texture", ErTexture), ("cdf", C.POINTER(C.c_float)), ("radiance_sum", C.c_float)]


class ErPointLight(C.Structure):
    _fields_ = [("position", ErVec3), ("radiance", ErVec3)]


class ErSceneDesc(C.Structure):
    _fields_ = [("tri_count", C.c_uint32),
                ("vertices", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)),
                ("tangents", C.POINTER(C.c_float)), ("uvs", C.POINTER(C.c_float)),
                ("tangent_sign", C.POINTER(C.c_float)), ("material_id", C.POINTER(C.c_int32)),
                ("material_count", C.c_uint32), ("materials", C.POINTER(ErMaterial)),
                ("texture_count", C.c_uint32), ("textures", C.POINTER(ErTexture)),
                ("hdri", ErHdri), ("camera", ErCamera),
                ("point_light_count", C.c_uint32), ("point_lights", C.POINTER(ErPointLight)),
                ("x_res", C.c_uint32), ("y_res", C.c_uint32)]


class ErRenderParams(C.Structure):
    _fields_ = [("sample_target", C.c_uint32), ("block_size", C.c_uint32), ("max_bounces", C.c_uint32),
                ("device", C.c_int32), ("rank", C.c_uint32), ("world", C.c_uint32), ("flags", C.c_uint32)]


class ErDeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 256), ("platform", C.c_char * 64), ("memory_bytes", C.c_uint64),
                ("compute_units", C.c_uint32), ("compatible", C.c_int32), ("arch", C.c_char * 64)]


class ErCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("paths", "bounce_samples", "rays", "node_visits", "tri_tests",
                                          "shaded_hits", "texel_fetches", "hdri_samples", "trace_wave_steps", "trace_busy_lanes",
                                          "trace_node_lanes", "trace_tri_lanes")]


class ErProfile(C.Structure):
    _fields_ = [("trace_ms", C.c_float), ("shade_ms", C.c_float), ("trace_launches", C.c_uint32), ("shade_launches", C.c_uint32), ("schedule", C.c_uint32),
                ("concurrency", C.c_uint32), ("empty_launches", C.c_uint32), ("empty_ms", C.c_float), ("rays_logged", C.c_uint64)]


class ErAccelInfo(C.Structure):
    _fields_ = [("node_count", C.c_uint32), ("node_bytes", C.c_uint32), ("leaf_count", C.c_uint32),
                ("max_depth", C.c_uint32), ("tri_record_bytes", C.c_uint32), ("build_ms", C.c_float),
                ("upload_ms", C.c_float), ("lift_bound", C.c_float), ("builder", C.c_uint32)]


class ErAdaptiveParams(C.Structure):
    _fields_ = [("threshold", C.c_float), ("min_samples", C.c_uint32), ("interval", C.c_uint32)]


class ErAdaptiveInfo(C.Structure):
    _fields_ = [("enabled", C.c_uint32), ("owned_tiles", C.c_uint32), ("active_tiles", C.c_uint32), ("tests_done", C.c_uint32),
                ("samples_rendered", C.c_uint32), ("next_test", C.c_uint32), ("pixel_samples", C.c_uint64), ("max_active_error", C.c_float)]


class ErLightInfo(C.Structure):
    _fields_ = [("emitters", C.c_uint32), ("total_weight", C.c_float)]


class ErSceneUpdate(C.Structure):
    _fields_ = [("what", C.c_uint32), ("camera", ErCamera), ("vertices", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)),
                ("tangents", C.POINTER(C.c_float))]


class ErUpdateInfo(C.Structure):
    _fields_ = [("updates", C.c_uint32), ("refits", C.c_uint32), ("refit_ms", C.c_float), ("update_ms", C.c_float)]


class ErSparseUpdate(C.Structure):
    _fields_ = [("what", C.c_uint32), ("camera", ErCamera), ("count", C.c_uint32), ("tri_ids", C.POINTER(C.c_uint32)), ("vertices", C.POINTER(C.c_float)),
                ("normals", C.POINTER(C.c_float)), ("tangents", C.POINTER(C.c_float))]


class ErSparseInfo(C.Structure):
    _fields_ = [("calls", C.c_uint32), ("path", C.c_uint32), ("why_full", C.c_uint32), ("moved", C.c_uint32), ("dirty_nodes2", C.c_uint32),
                ("dirty_nodes8", C.c_uint32), ("bytes_uploaded", C.c_uint64), ("refit_ms", C.c_float)]


class ErObjectTransform(C.Structure):   # row-major 3x4: x' = L x + t
    _fields_ = [("object", C.c_uint32), ("m", C.c_float * 12)]


class ErTransformUpdate(C.Structure):
    _fields_ = [("what", C.c_uint32), ("camera", ErCamera), ("count", C.c_uint32), ("transforms", C.POINTER(ErObjectTransform))]


class ErTransformInfo(C.Structure):
    _fields_ = [("calls", C.c_uint32), ("objects", C.c_uint32), ("moved", C.c_uint32), ("path", C.c_uint32), ("why_full", C.c_uint32), ("dirty_nodes2", C.c_uint32),
                ("dirty_nodes8", C.c_uint32), ("reserved", C.c_uint32), ("bytes_uploaded", C.c_uint64), ("refit_ms", C.c_float)]


class ErSkin(C.Structure):   # [size_of(object)][3][4] bones and weights, the object's tri_ids order
    _fields_ = [("object", C.c_uint32), ("bone_count", C.c_uint32), ("bones", C.POINTER(C.c_uint16)), ("weights", C.POINTER(C.c_float))]


class ErSkinPose(C.Structure):   # palette: [bone_count][12], row-major 3x4 each
    _fields_ = [("object", C.c_uint32), ("bone_count", C.c_uint32), ("palette", C.POINTER(C.c_float))]


class ErSkinUpdate(C.Structure):
    _fields_ = [("what", C.c_uint32), ("camera", ErCamera), ("count", C.c_uint32), ("poses", C.POINTER(ErSkinPose))]


class ErSkinInfo(C.Structure):
    _fields_ = [("calls", C.c_uint32), ("skinned", C.c_uint32), ("objects", C.c_uint32), ("bones", C.c_uint32), ("moved", C.c_uint32), ("path", C.c_uint32),
                ("why_full", C.c_uint32), ("dirty_nodes2", C.c_uint32), ("dirty_nodes8", C.c_uint32), ("refit_ms", C.c_float), ("bytes_uploaded", C.c_uint64),
                ("influence_bytes", C.c_uint64)]


class ErSceneEdit(C.Structure):
    _fields_ = [("what", C.c_uint32), ("camera", ErCamera), ("vertices", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)),
                ("tangents", C.POINTER(C.c_float)), ("material_count", C.c_uint32), ("materials", C.POINTER(ErMaterial)),
                ("material_id", C.POINTER(C.c_int32)), ("texture_count", C.c_uint32), ("textures", C.POINTER(ErTexture)), ("hdri", ErHdri)]


class ErEditInfo(C.Structure):
    _fields_ = [("edits", C.c_uint32), ("texture_stage", C.c_uint32), ("texture_stage_ms", C.c_float), ("edit_ms", C.c_float), ("pool_floats", C.c_uint64)]


class ErTopologyEdit(C.Structure):
    _fields_ = [("what", C.c_uint32), ("remove_count", C.c_uint32), ("remove_ids", C.POINTER(C.c_uint32)), ("append_count", C.c_uint32),
                ("vertices", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)), ("tangents", C.POINTER(C.c_float)), ("uvs", C.POINTER(C.c_float)),
                ("tangent_sign", C.POINTER(C.c_float)), ("material_id", C.POINTER(C.c_int32)), ("append_as_object", C.c_uint32), ("rest", ErSceneEdit)]


class ErTopologyInfo(C.Structure):
    _fields_ = [("calls", C.c_uint32), ("removed", C.c_uint32), ("appended", C.c_uint32), ("tri_count", C.c_uint32), ("path", C.c_uint32),
                ("texture_stage", C.c_uint32), ("bytes_uploaded", C.c_uint64), ("build_ms", C.c_float), ("store_ms", C.c_float), ("edit_ms", C.c_float),
                ("texture_stage_ms", C.c_float)]


class ErAccelCost(C.Structure):
    _fields_ = [("node_area", C.c_double), ("leaf_area", C.c_double), ("tri_area", C.c_double), ("cost", C.c_double), ("ms", C.c_float), ("builder", C.c_uint32)]


class ErUpdatePolicy(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("max_cost_ratio", C.c_float)]


class ErRebuildInfo(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("max_cost_ratio", C.c_float), ("rebuilds", C.c_uint32), ("last_decision", C.c_uint32), ("cost_built", C.c_double),
                ("cost_refit", C.c_double), ("cost_after", C.c_double), ("cost_ms", C.c_float), ("rebuild_ms", C.c_float)]


class ErCostSumsDebug(C.Structure):   # include/eleven_hip_debug.h: er_debug_accel_cost_terms / er_debug_accel_cost_host
    _fields_ = [("node_area", C.c_double), ("leaf_area", C.c_double), ("tri_area", C.c_double), ("cost", C.c_double), ("ms", C.c_float), ("reserved", C.c_uint32)]


class ErTexEntry(C.Structure):   # include/eleven_hip_debug.h (csrc/er_device.h DevTex)
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("filter", C.c_int32), ("offset", C.c_uint32)]


class ErTexturePlan(C.Structure):   # include/eleven_hip_debug.h: er_debug_texture_plan
    _fields_ = [("texture_count", C.c_uint32), ("fused_count", C.c_uint32), ("fused_any", C.c_uint32), ("reserved", C.c_uint32), ("hdri", ErTexEntry),
                ("pool_floats", C.c_uint64)]


class ErTextureDump(C.Structure):   # include/eleven_hip_debug.h: er_debug_read_textures
    _fields_ = [("texture_count", C.c_uint32), ("material_count", C.c_uint32), ("fused_count", C.c_uint32), ("cdf_count", C.c_uint32), ("guide_count", C.c_uint32),
                ("tex_pow2", C.c_uint32), ("fused_any", C.c_uint32), ("hdri_buckets", C.c_int32), ("hdri_radiance_sum", C.c_float), ("hdri_tex", ErTexEntry),
                ("pool_floats", C.c_uint64)]


# numpy mirrors of the texture table's and the fused records' descriptors (elevenrender_amd/csrc/er_device.h: DevTex, DevFused)
TEX_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("channels", "<i4"), ("filter", "<i4"), ("offset", "<u4")])
FUSED_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("filter", "<i4"), ("offset", "<u4")])
assert TEX_DTYPE.itemsize == 20 and FUSED_DTYPE.itemsize == 16


class ErFeatureInfo(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("samples", C.c_uint32), ("rays", C.c_uint64), ("ms", C.c_float)]


class ErDenoiseGuided(C.Structure):
    _fields_ = [("levels", C.c_uint32), ("colour_sigma", C.c_float), ("albedo_sigma", C.c_float), ("depth_sigma", C.c_float)]


class ErIdInfo(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("samples", C.c_uint32), ("rays", C.c_uint64), ("ms", C.c_float), ("objects", C.c_uint32),
                ("overflow_pixels", C.c_uint32 * ID_KIND_COUNT)]


class ErHistoryParams(C.Structure):
    _fields_ = [("depth_tolerance", C.c_float), ("max_weight", C.c_float)]


class ErHistoryInfo(C.Structure):
    _fields_ = [("captured", C.c_uint32), ("resolved", C.c_uint32), ("moved_objects", C.c_uint32), ("pixels_valid", C.c_uint64), ("pixels_partial", C.c_uint64),
                ("pixels_offscreen", C.c_uint64), ("pixels_rejected", C.c_uint64), ("pixels_sky", C.c_uint64), ("capture_ms", C.c_float), ("resolve_ms", C.c_float)]


class ErVarianceInfo(C.Structure):
    _fields_ = [("folds", C.c_uint32), ("reserved", C.c_uint32), ("pixels_folded", C.c_uint64), ("pixels_known", C.c_uint64), ("fold_ms", C.c_float),
                ("filter_ms", C.c_float)]


class ErDenoiseVariance(C.Structure):
    _fields_ = [("levels", C.c_uint32), ("colour_sigma", C.c_float), ("albedo_sigma", C.c_float), ("depth_sigma", C.c_float)]


class ErHistoryVarianceInfo(C.Structure):
    _fields_ = [("captured", C.c_uint32), ("resolved", C.c_uint32), ("pixels_known_captured", C.c_uint64), ("pixels_known_history", C.c_uint64),
                ("pixels_known_blended", C.c_uint64), ("filter_ms", C.c_float)]


class ErFirstHitParams(C.Structure):
    _fields_ = [("cutouts", C.c_uint32), ("opacity_threshold", C.c_float)]


class ErFirstHitInfo(C.Structure):
    _fields_ = [("cutouts", C.c_uint32), ("opacity_threshold", C.c_float), ("rays", C.c_uint64), ("rays_through", C.c_uint64), ("layers_skipped", C.c_uint64),
                ("rays_capped", C.c_uint64), ("rays_through_to_miss", C.c_uint64)]


class ErPick(C.Structure):
    _fields_ = [("hit", C.c_uint32), ("triangle", C.c_uint32), ("object", C.c_uint32), ("material", C.c_uint32), ("distance", C.c_float),
                ("position", C.c_float * 3), ("uv", C.c_float * 2)]


class ErStreamInfo(C.Structure):   # include/eleven_hip_debug.h
    _fields_ = [("waves", C.c_uint32), ("tracers", C.c_uint32), ("large_regions", C.c_uint32), ("deal_pending", C.c_uint32), ("launches", C.c_uint32),
                ("pixels_per_cu", C.c_uint32), ("lanes_busy", C.c_double), ("launch_ms", C.c_double), ("cost_spread", C.c_double),
                ("spec_started", C.c_uint64), ("spec_right", C.c_uint64), ("spec_wrong", C.c_uint64),
                ("form", C.c_uint32), ("reserved", C.c_uint32)]


class ErStreamBalance(C.Structure):   # include/eleven_hip_debug.h
    _fields_ = [("blocks", C.c_uint32), ("most", C.c_uint32), ("levelled", C.c_uint32), ("counting", C.c_uint32), ("cost_tiles", C.c_uint32), ("cap", C.c_uint32),
                ("launch_ticks", C.c_uint64)]


class ErStreamForm(C.Structure):   # include/eleven_hip_debug.h
    _fields_ = [("waves", C.c_uint32), ("tracers", C.c_uint32), ("adapt", C.c_uint32), ("keep", C.c_uint32), ("spec", C.c_uint32), ("reserved", C.c_uint32)]


class ErAccelDump(C.Structure):   # include/eleven_hip_debug.h: er_debug_read_accel / er_debug_bvh_dump
    _fields_ = [("tri_count", C.c_uint32), ("node_count", C.c_uint32), ("node8_count", C.c_uint32), ("node8_pieces", C.c_uint32),
                ("attr_pieces", C.c_uint32), ("max_depth", C.c_uint32), ("max_depth8", C.c_uint32), ("builder", C.c_uint32),
                ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("lift_bound", C.c_float), ("max_lift", C.c_float)]


# numpy mirrors of the structure's records (elevenrender_amd/csrc/er_bvh.h: ErNode, ErNode8, ErTriIsect, ErTriAttr)
NODE_DTYPE = np.dtype([("lo0", "<f4", 3), ("hi0", "<f4", 3), ("lo1", "<f4", 3), ("hi1", "<f4", 3), ("c0", "<i4"), ("c1", "<i4"), ("pad", "<i4", 2)])
NODE8_DTYPE = np.dtype([("p", "<f4", 3), ("e", "u1", 3), ("imask", "u1"), ("child_base", "<u4"), ("tri_base", "<u4"), ("tri_present", "<u4"),
                        ("reserved", "<u4"), ("qlo", "u1", (3, 8)), ("qhi", "u1", (3, 8))])
ISECT_DTYPE = np.dtype([("v0", "<f4", 3), ("tri_id", "<i4"), ("v1", "<f4", 3), ("lift", "<f4"), ("v2", "<f4", 3), ("sign", "<f4")])
assert NODE_DTYPE.itemsize == 64 and NODE8_DTYPE.itemsize == 80 and ISECT_DTYPE.itemsize == 48


def attr_dtype(pieces):
    """ErTriAttr at a stride of `pieces` 16-byte pieces (ER_ATTR_PIECES: 7 packed, 8 one record per 128-byte line)."""
    dt = np.dtype([("n", "<f4", (3, 3)), ("t", "<f4", (3, 3)), ("uv", "<f4", (3, 2)), ("material", "<i4"), ("pad", "<u4", 4 * pieces - 25)])
    assert dt.itemsize == 16 * pieces
    return dt


def accel_dump_dict(info, **arrays):
    """The Python form of an ErAccelDump and its arrays: what tests/accel_check.py takes."""
    d = {n: int(getattr(info, n)) for n in ("tri_count", "node_count", "node8_count", "max_depth", "max_depth8", "builder")}
    d["lo"], d["hi"] = np.array(list(info.lo), np.float32), np.array(list(info.hi), np.float32)
    d["lift_bound"], d["max_lift"] = np.float32(info.lift_bound), np.float32(info.max_lift)
    d.update(arrays)
    return d


def debug_bvh_dump(vertices, normals, threads=0):
    """include/eleven_hip_debug.h er_debug_bvh_dump: the HOST builder's structure for [n][3][3] vertices / normals (no device needed) as
    a dict: nodes (NODE_DTYPE), nodes8 (NODE8_DTYPE), slot_to_tri uint32[n], tri_lift float32[n] (per original triangle), lo, hi,
    lift_bound, max_depth, max_depth8, counts."""
    lib = load()
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3, 3)
    nn = np.ascontiguousarray(normals, np.float32).reshape(-1, 3, 3)
    assert v.shape == nn.shape
    n = len(v)
    info = ErAccelDump()
    args = (_fptr(v), _fptr(nn), n, threads, C.byref(info))
    check(lib.er_debug_bvh_dump(*args, None, 0, None, 0, None, 0, None, 0))
    assert info.node8_pieces * 16 == NODE8_DTYPE.itemsize
    nodes, nodes8 = np.zeros(info.node_count, NODE_DTYPE), np.zeros(info.node8_count, NODE8_DTYPE)
    s2t, lift = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib.er_debug_bvh_dump(*args, vp(nodes), nodes.nbytes, vp(nodes8), nodes8.nbytes, s2t.ctypes.data_as(C.POINTER(C.c_uint32)), s2t.nbytes,
                                _fptr(lift), lift.nbytes))
    return accel_dump_dict(info, nodes=nodes, nodes8=nodes8, slot_to_tri=s2t, tri_lift=lift)


def debug_spill_levels(spilled, n, usable):
    """include/eleven_hip_debug.h er_debug_spill_levels: what er_debug_trace_rays_levels says about a spill area read back, on a caller's
    buffer (uint32 [ceil(n / 64)][stack levels][64][2], 0xFFFFFFFF where nothing was written; no device needed).  Returns uint32[n]
    levels; raises ErError(ER_ERR_STATE) for an entry that should not be there."""
    buf = np.ascontiguousarray(spilled, np.uint32)
    levels = np.zeros(n, np.uint32)
    check(load().er_debug_spill_levels(buf.ctypes.data_as(C.c_void_p), buf.nbytes, n, usable, levels.ctypes.data_as(C.POINTER(C.c_uint32))))
    return levels


def debug_transform_apply(m, vertices, normals, tangents):
    """include/eleven_hip_debug.h er_debug_transform_apply: the host form of er_render_transform's arithmetic (csrc/er_xform.h; no device
    needed) on [n][3][3] rest arrays: the posed (vertices, normals, tangents)."""
    lib = load()
    mm = np.ascontiguousarray(m, np.float32).reshape(12)
    v, n, t = (np.ascontiguousarray(a, np.float32).reshape(-1, 3, 3) for a in (vertices, normals, tangents))
    assert v.shape == n.shape == t.shape
    out = [np.empty_like(v) for _ in range(3)]
    check(lib.er_debug_transform_apply(_fptr(mm), len(v), _fptr(v), _fptr(n), _fptr(t), *(_fptr(o) for o in out)))
    return tuple(out)


def debug_skin_apply(palette, bones, weights, vertices, normals, tangents):
    """include/eleven_hip_debug.h er_debug_skin_apply: the host form of er_render_skin's arithmetic (csrc/er_skin.h; no device needed) on
    [n][3][3] rest arrays with [n][3][4] bones and weights: the skinned (vertices, normals, tangents)."""
    lib = load()
    P = np.ascontiguousarray(palette, np.float32).reshape(-1, 12)
    v, n, t = (np.ascontiguousarray(a, np.float32).reshape(-1, 3, 3) for a in (vertices, normals, tangents))
    b = np.ascontiguousarray(bones, np.uint16).reshape(-1, 3, 4)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1, 3, 4)
    assert v.shape == n.shape == t.shape and len(b) == len(w) == len(v)
    out = [np.empty_like(v) for _ in range(3)]
    check(lib.er_debug_skin_apply(_fptr(P), len(P), len(v), b.ctypes.data_as(C.POINTER(C.c_uint16)), _fptr(w), _fptr(v), _fptr(n), _fptr(t), *(_fptr(o) for o in out)))
    return tuple(out)


def debug_id_rank(ids):
    """include/eleven_hip_debug.h er_debug_id_rank: the ranking er_render_ids gives a pixel (csrc/er_ids.h, the function the kernel calls;
    no device needed) for the ids of its rays that hit, at most 64: (slot ids uint32[4], slot counts uint32[4], distinct ids)."""
    lib = load()
    a = np.ascontiguousarray(ids, np.uint32).reshape(-1)
    oi, oc, distinct = np.zeros(ID_SLOTS, np.uint32), np.zeros(ID_SLOTS, np.uint32), C.c_uint32()
    up = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))
    check(lib.er_debug_id_rank(up(a) if a.size else None, a.size, up(oi), up(oc), C.byref(distinct)))
    return oi, oc, distinct.value


def debug_history_camera(camera):
    """include/eleven_hip_debug.h er_debug_history_camera: the 12 floats the reprojection projects through (csrc/er_reproject.h) for an
    ErCamera: position, sensor size, focal length and the rotation's cosines and sines as the library evaluates them."""
    out = np.zeros(12, np.float32)
    check(load().er_debug_history_camera(C.byref(camera), _fptr(out)))
    return out


def debug_history_project(cam, x_res, y_res, points):
    """er_debug_history_project: (xy float32[n][2], ok bool[n]) -- elevenrender_amd/history.py project() restates it"""
    c, p = np.ascontiguousarray(cam, np.float32).reshape(12), np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    xy, ok = np.zeros((len(p), 2), np.float32), np.zeros(len(p), np.uint32)
    check(load().er_debug_history_project(_fptr(c), x_res, y_res, len(p), _fptr(p), _fptr(xy), ok.ctypes.data_as(_UP)))
    return xy, ok != 0


def debug_history_back_matrix(m_capture, m_now):
    """er_debug_history_back_matrix: float32[12], or None where the library refuses the pair"""
    a, b = np.ascontiguousarray(m_capture, np.float32).reshape(12), np.ascontiguousarray(m_now, np.float32).reshape(12)
    out = np.zeros(12, np.float32)
    rc = load().er_debug_history_back_matrix(_fptr(a), _fptr(b), _fptr(out))
    if rc == ER_ERR_INVALID_ARG:
        return None
    check(rc)
    return out


def debug_history_taps(cam, x_res, y_res, tol, hit, obj, P, moved, back, old_hit, old_obj, old_dist, old_cw):
    """er_debug_history_taps: (rgbw float32[n][4], state uint32[n][4], class uint32[n]) -- history.py resolve() restates it"""
    u32 = lambda a: np.ascontiguousarray(a, np.uint32).reshape(-1)
    f32 = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1)
    c, hit, obj, P, moved, back = f32(cam), u32(hit), u32(obj), f32(P), u32(moved), f32(back)
    old_hit, old_obj, old_dist, old_cw = u32(old_hit), u32(old_obj), f32(old_dist), f32(old_cw)
    n = len(hit)
    assert len(P) == 3 * n and len(back) == 12 * n and len(moved) == n and len(obj) == n
    assert len(old_hit) == len(old_obj) == len(old_dist) == x_res * y_res and len(old_cw) == 4 * x_res * y_res
    rgbw, state, cls = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32)
    up = lambda a: a.ctypes.data_as(_UP)
    check(load().er_debug_history_taps(_fptr(c), x_res, y_res, float(tol), n, up(hit), up(obj), _fptr(P), up(moved), _fptr(back), up(old_hit), up(old_obj),
                                       _fptr(old_dist), _fptr(old_cw), _fptr(rgbw), up(state), up(cls)))
    return rgbw, state, cls


def debug_history_capture(beauty, samples, hist, max_weight):
    """er_debug_history_capture: (C.rgb, W) float32[n][4]; hist None = no resolved history"""
    b, s = np.ascontiguousarray(beauty, np.float32).reshape(-1, 4), np.ascontiguousarray(samples, np.uint32).reshape(-1)
    h = None if hist is None else np.ascontiguousarray(hist, np.float32).reshape(-1, 4)
    out = np.zeros((len(s), 4), np.float32)
    check(load().er_debug_history_capture(len(s), _fptr(b), s.ctypes.data_as(_UP), None if h is None else _fptr(h), float(max_weight), _fptr(out)))
    return out


def debug_history_blend(beauty, samples, hist):
    """er_debug_history_blend: float32[n][4]"""
    b, s = np.ascontiguousarray(beauty, np.float32).reshape(-1, 4), np.ascontiguousarray(samples, np.uint32).reshape(-1)
    h = np.ascontiguousarray(hist, np.float32).reshape(-1, 4)
    out = np.zeros((len(s), 4), np.float32)
    check(load().er_debug_history_blend(len(s), _fptr(b), s.ctypes.data_as(_UP), _fptr(h), _fptr(out)))
    return out


def _opt4(a, width=4):
    return None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1, width)


def _optp(a):
    return None if a is None else _fptr(a)


def debug_history_variance_current(state):
    """include/eleven_hip_debug.h er_debug_history_variance_current: (s2.rgb, K >= 2) float32[n][4] of states [n][12]
    (csrc/er_history_variance.h; no device needed) -- elevenrender_amd/history_variance.py current() restates it"""
    st = _opt4(state, 12)
    out = np.zeros((len(st), 4), np.float32)
    check(load().er_debug_history_variance_current(len(st), _fptr(st), _fptr(out)))
    return out


def debug_history_variance_pool(s_h, w, s_c, n):
    """er_debug_history_variance_pool: (pool.rgb, flag) float32[n][4]"""
    a, b = _opt4(s_h), _opt4(s_c)
    w, n = np.ascontiguousarray(w, np.float32).reshape(-1), np.ascontiguousarray(n, np.float32).reshape(-1)
    out = np.zeros((len(a), 4), np.float32)
    check(load().er_debug_history_variance_pool(len(a), _fptr(a), _fptr(w), _fptr(b), _fptr(n), _fptr(out)))
    return out


def debug_history_variance_capture(state, samples, hist, hv):
    """er_debug_history_variance_capture: SV float32[n][4]; state None = K 0, hist None = w 0, hv None = no carried variance"""
    st, h, v = _opt4(state, 12), _opt4(hist), _opt4(hv)
    s = np.ascontiguousarray(samples, np.uint32).reshape(-1)
    out = np.zeros((len(s), 4), np.float32)
    check(load().er_debug_history_variance_capture(len(s), _optp(st), s.ctypes.data_as(_UP), _optp(h), _optp(v), _fptr(out)))
    return out


def debug_history_variance_mean(tap_state, tap_w, tap_sv):
    """er_debug_history_variance_mean: HV float32[n][4] from tap states [n][4], tap weights [n][4] and the taps' SV [n][4][4]"""
    st = np.ascontiguousarray(tap_state, np.uint32).reshape(-1, 4)
    tw, sv = _opt4(tap_w), _opt4(tap_sv, 16)
    out = np.zeros((len(st), 4), np.float32)
    check(load().er_debug_history_variance_mean(len(st), st.ctypes.data_as(_UP), _fptr(tw), _fptr(sv), _fptr(out)))
    return out


def debug_history_variance_taps(cam, x_res, y_res, tol, hit, obj, P, moved, back, old_hit, old_obj, old_dist, old_cw, old_sv):
    """er_debug_history_variance_taps: (rgbw, hv float32[n][4], state uint32[n][4], class uint32[n]) -- history_variance.py resolve()"""
    u32 = lambda a: np.ascontiguousarray(a, np.uint32).reshape(-1)
    f32 = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1)
    c, hit, obj, P, moved, back = f32(cam), u32(hit), u32(obj), f32(P), u32(moved), f32(back)
    old_hit, old_obj, old_dist, old_cw, old_sv = u32(old_hit), u32(old_obj), f32(old_dist), f32(old_cw), f32(old_sv)
    n = len(hit)
    assert len(P) == 3 * n and len(back) == 12 * n and len(moved) == n and len(obj) == n
    assert len(old_hit) == len(old_obj) == len(old_dist) == x_res * y_res and len(old_cw) == len(old_sv) == 4 * x_res * y_res
    rgbw, hv, state, cls = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32)
    up = lambda a: a.ctypes.data_as(_UP)
    check(load().er_debug_history_variance_taps(_fptr(c), x_res, y_res, float(tol), n, up(hit), up(obj), _fptr(P), up(moved), _fptr(back), up(old_hit), up(old_obj),
                                                _fptr(old_dist), _fptr(old_cw), _fptr(old_sv), _fptr(rgbw), _fptr(hv), up(state), up(cls)))
    return rgbw, hv, state, cls


def debug_history_variance_blend(state, samples, hist, hv):
    """er_debug_history_variance_blend: VB float32[n][4]"""
    st, h, v = _opt4(state, 12), _opt4(hist), _opt4(hv)
    s = np.ascontiguousarray(samples, np.uint32).reshape(-1)
    out = np.zeros((len(s), 4), np.float32)
    check(load().er_debug_history_variance_blend(len(s), _optp(st), s.ctypes.data_as(_UP), _fptr(h), _optp(v), _fptr(out)))
    return out


def debug_history_variance_split(blend, vb, albedo):
    """er_debug_history_variance_split: (e, ve) float32[n][4]"""
    b, v, a = _opt4(blend), _opt4(vb), _opt4(albedo)
    e, ve = np.zeros_like(b), np.zeros_like(b)
    check(load().er_debug_history_variance_split(len(b), _fptr(b), _fptr(v), _fptr(a), _fptr(e), _fptr(ve)))
    return e, ve


def debug_cutout_threshold(t):
    """include/eleven_hip_debug.h er_debug_cutout_threshold: (ok uint32[n], resolved float32[n]) of thresholds as er_first_hit_set takes them
    (csrc/er_cutout.h; no device needed) -- elevenrender_amd/first_hit.py restates it"""
    t = np.ascontiguousarray(t, np.float32).reshape(-1)
    ok, res = np.zeros(len(t), np.uint32), np.zeros(len(t), np.float32)
    check(load().er_debug_cutout_threshold(len(t), _fptr(t), ok.ctypes.data_as(_UP), _fptr(res)))
    return ok, res


def debug_cutout_stops(opacity, threshold):
    """er_debug_cutout_stops: uint32[n], 1 where a hit of this opacity stops the ray"""
    a, t = np.ascontiguousarray(opacity, np.float32).reshape(-1), np.ascontiguousarray(threshold, np.float32).reshape(-1)
    out = np.zeros(len(a), np.uint32)
    check(load().er_debug_cutout_stops(len(a), _fptr(a), _fptr(t), out.ctypes.data_as(_UP)))
    return out


def debug_cutout_continue(position, d):
    """er_debug_cutout_continue: (origin, direction) float32[n][3] of the ray that goes on past a hit at `position` along `d`"""
    p, d = np.ascontiguousarray(position, np.float32).reshape(-1, 3), np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    o2, d2 = np.zeros_like(p), np.zeros_like(p)
    check(load().er_debug_cutout_continue(len(p), _fptr(p), _fptr(d), _fptr(o2), _fptr(d2)))
    return o2, d2


def debug_variance_mark(beauty, samples):
    """include/eleven_hip_debug.h er_debug_variance_mark: the state float32[n][12] of a reset (csrc/er_variance.h; no device needed) --
    elevenrender_amd/variance.py mark() restates it"""
    b, s = np.ascontiguousarray(beauty, np.float32).reshape(-1, 4), np.ascontiguousarray(samples, np.uint32).reshape(-1)
    st = np.zeros((len(s), 12), np.float32)
    check(load().er_debug_variance_mark(len(s), _fptr(b), s.ctypes.data_as(_UP), _fptr(st)))
    return st


def debug_variance_fold(state, beauty, samples):
    """er_debug_variance_fold: (new state float32[n][12], folded bool[n]); `state` is not changed"""
    st = np.ascontiguousarray(state, np.float32).reshape(-1, 12).copy()
    b, s = np.ascontiguousarray(beauty, np.float32).reshape(-1, 4), np.ascontiguousarray(samples, np.uint32).reshape(-1)
    assert len(st) == len(b) == len(s)
    folded = np.zeros(len(s), np.uint32)
    check(load().er_debug_variance_fold(len(s), _fptr(b), s.ctypes.data_as(_UP), _fptr(st), folded.ctypes.data_as(_UP)))
    return st, folded != 0


def debug_variance_value(state, samples):
    """er_debug_variance_value: float32[n][4] = er_read_variance's pixels"""
    st, s = np.ascontiguousarray(state, np.float32).reshape(-1, 12), np.ascontiguousarray(samples, np.uint32).reshape(-1)
    assert len(st) == len(s)
    out = np.zeros((len(s), 4), np.float32)
    check(load().er_debug_variance_value(len(s), _fptr(st), s.ctypes.data_as(_UP), _fptr(out)))
    return out


def debug_variance_split(value, albedo):
    """er_debug_variance_split: the demodulated variance float32[n][4] (w: the K >= 2 flag)"""
    v, a = np.ascontiguousarray(value, np.float32).reshape(-1, 4), np.ascontiguousarray(albedo, np.float32).reshape(-1, 4)
    assert len(v) == len(a)
    out = np.zeros((len(v), 4), np.float32)
    check(load().er_debug_variance_split(len(v), _fptr(v), _fptr(a), _fptr(out)))
    return out


def debug_variance_level(e, ve, normal, albedo, depth, w, h, step, kc, ka, kz):
    """er_debug_variance_level_px: one level of er_denoise_variance over a frame of w x h pixels: (e', ve') float32[h * w][4]"""
    planes = [np.ascontiguousarray(a, np.float32).reshape(-1, 4) for a in (e, ve, normal, albedo, depth)]
    assert all(len(a) == w * h for a in planes)
    oe, ov = np.zeros((w * h, 4), np.float32), np.zeros((w * h, 4), np.float32)
    check(load().er_debug_variance_level_px(w, h, step, float(kc), float(ka), float(kz), *(_fptr(a) for a in planes), _fptr(oe), _fptr(ov)))
    return oe, ov


def _cost_dict(sums, node_terms, tri_terms):
    d = {n: getattr(sums, n) for n in ("node_area", "leaf_area", "tri_area", "cost", "ms")}
    d.update(node_terms=node_terms, tri_terms=tri_terms)
    return d


def debug_accel_cost_host(nodes8, isect, tri_count):
    """include/eleven_hip_debug.h er_debug_accel_cost_host: the host compilation of csrc/er_cost.h over a dump's wide nodes (NODE8_DTYPE,
    packed) and intersection records (ISECT_DTYPE; the first tri_count are read) -- no device needed.  A dict: node_area, leaf_area,
    tri_area, cost, node_terms float64[N, 2] (node_i, leaf_i), tri_terms float32[tri_count]."""
    lib = load()
    n8 = np.ascontiguousarray(nodes8, NODE8_DTYPE)
    rec = np.ascontiguousarray(isect, ISECT_DTYPE)
    n = int(tri_count)
    assert len(rec) >= n
    sums, nt, tt = ErCostSumsDebug(), np.zeros((len(n8), 2), np.float64), np.zeros(n, np.float32)
    check(lib.er_debug_accel_cost_host(n8.ctypes.data_as(C.c_void_p), len(n8), NODE8_DTYPE.itemsize // 16, rec.ctypes.data_as(C.c_void_p), n, C.byref(sums),
                                       nt.ctypes.data_as(C.POINTER(C.c_double)), nt.nbytes, _fptr(tt), tt.nbytes))
    return _cost_dict(sums, nt, tt)


def debug_texture_plan(scene):
    """include/eleven_hip_debug.h er_debug_texture_plan: the texture plan of a SceneData (or of an ErSceneDesc whose textures declare
    sizes only: no texel is read; no device needed) as a dict: modes uint8[textures], table (TEX_DTYPE), fused (FUSED_DTYPE, one per
    material), hdri (dict of the HDRI's entry), hdri_offset, pool_floats, fused_any."""
    lib = load()
    d = scene if isinstance(scene, ErSceneDesc) else scene.desc()
    plan = ErTexturePlan()
    check(lib.er_debug_texture_plan(C.byref(d), C.byref(plan), None, 0, None, 0, None, 0))
    modes, table, fused = np.zeros(plan.texture_count, np.uint8), np.zeros(plan.texture_count, TEX_DTYPE), np.zeros(plan.fused_count, FUSED_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib.er_debug_texture_plan(C.byref(d), C.byref(plan), vp(modes), modes.nbytes, vp(table), table.nbytes, vp(fused), fused.nbytes))
    hdri = {n: int(getattr(plan.hdri, n)) for n, _ in ErTexEntry._fields_}
    return dict(modes=modes, table=table, fused=fused, hdri=hdri, hdri_offset=hdri["offset"], pool_floats=int(plan.pool_floats), fused_any=int(plan.fused_any))


class ErTraceRec(C.Structure):   # include/eleven_hip_debug.h; same layout as the oracle's OracleTraceRec
    _fields_ = [("bounce", C.c_int32), ("tri", C.c_int32), ("shadow_tri", C.c_int32), ("opaque", C.c_int32),
                ("position", C.c_float * 3), ("wi", C.c_float * 3), ("light", C.c_float * 3), ("reduction", C.c_float * 3),
                ("shadow_occ", C.c_int32), ("light_occ", C.c_int32)]


# every symbol include/eleven_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_FP, _IP, _UP = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
SYMBOLS = {
    "er_abi_version": (C.c_int, []),
    "er_last_error": (C.c_char_p, []),
    "er_device_count": (C.c_int, []),
    "er_device_info": (C.c_int, [C.c_int, C.POINTER(ErDeviceInfo)]),
    "er_device_find": (C.c_int, [C.c_char_p]),
    "er_scene_create": (C.c_int, [C.POINTER(ErSceneDesc), C.POINTER(_P)]),
    "er_scene_destroy": (None, [_P]),
    "er_render_begin": (C.c_int, [_P, C.POINTER(ErRenderParams)]),
    "er_render_samples": (C.c_int, [_P, C.c_uint32]),
    "er_render_samples_async": (C.c_int, [_P, C.c_uint32]),
    "er_wait": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "er_samples_done": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "er_read_pass": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float)]),
    "er_read_samples": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "er_read_rng": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "er_owned_count": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint64)]),
    "er_pack_owned": (C.c_int, [_P, C.c_int, _P]),
    "er_unpack_owned": (C.c_int, [_P, C.c_int, C.c_uint32, _P]),
    "er_get_counters": (C.c_int, [_P, C.POINTER(ErCounters)]),
    "er_accel_info": (C.c_int, [_P, C.POINTER(ErAccelInfo)]),
    "er_render_update": (C.c_int, [_P, C.POINTER(ErSceneUpdate)]),
    "er_update_info": (C.c_int, [_P, C.POINTER(ErUpdateInfo)]),
    "er_render_update_sparse": (C.c_int, [_P, C.POINTER(ErSparseUpdate)]),
    "er_sparse_info": (C.c_int, [_P, C.POINTER(ErSparseInfo)]),
    "er_objects_set": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "er_render_transform": (C.c_int, [_P, C.POINTER(ErTransformUpdate)]),
    "er_transform_info": (C.c_int, [_P, C.POINTER(ErTransformInfo)]),
    "er_skin_set": (C.c_int, [_P, C.POINTER(ErSkin)]),
    "er_render_skin": (C.c_int, [_P, C.POINTER(ErSkinUpdate)]),
    "er_skin_info": (C.c_int, [_P, C.POINTER(ErSkinInfo)]),
    "er_render_edit": (C.c_int, [_P, C.POINTER(ErSceneEdit)]),
    "er_edit_info": (C.c_int, [_P, C.POINTER(ErEditInfo)]),
    "er_accel_cost": (C.c_int, [_P, C.POINTER(ErAccelCost)]),
    "er_update_policy_set": (C.c_int, [_P, C.POINTER(ErUpdatePolicy)]),
    "er_rebuild_info": (C.c_int, [_P, C.POINTER(ErRebuildInfo)]),
    "er_render_topology": (C.c_int, [_P, C.POINTER(ErTopologyEdit)]),
    "er_topology_info": (C.c_int, [_P, C.POINTER(ErTopologyInfo)]),
    "er_adaptive_set": (C.c_int, [_P, C.POINTER(ErAdaptiveParams)]),
    "er_adaptive_info": (C.c_int, [_P, C.POINTER(ErAdaptiveInfo)]),
    "er_read_tile_state": (C.c_int, [_P, _FP, C.POINTER(C.c_uint32)]),
    "er_light_info": (C.c_int, [_P, C.POINTER(ErLightInfo)]),
    "er_get_profile": (C.c_int, [_P, C.POINTER(ErProfile)]),
    "er_denoise": (C.c_int, [_P, C.c_uint32, C.c_float]),
    "er_render_features": (C.c_int, [_P, C.c_uint32]),
    "er_feature_info": (C.c_int, [_P, C.POINTER(ErFeatureInfo)]),
    "er_read_feature": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float)]),
    "er_gather_feature": (C.c_int, [_P, C.c_int, _P, C.c_uint32]),
    "er_denoise_guided": (C.c_int, [_P, C.POINTER(ErDenoiseGuided)]),
    "er_render_ids": (C.c_int, [_P, C.c_uint32]),
    "er_id_info": (C.c_int, [_P, C.POINTER(ErIdInfo)]),
    "er_read_ids": (C.c_int, [_P, C.c_int, _UP, _UP]),
    "er_gather_ids": (C.c_int, [_P, C.c_int, _P, C.c_uint32]),
    "er_id_matte": (C.c_int, [_P, C.c_int, _UP, C.c_uint32, _FP]),
    "er_pick_rect": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _UP, C.c_uint32, _UP]),
    "er_pick": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(ErPick)]),
    "er_history_capture": (C.c_int, [_P, C.POINTER(ErHistoryParams)]),
    "er_history_resolve": (C.c_int, [_P]),
    "er_history_info": (C.c_int, [_P, C.POINTER(ErHistoryInfo)]),
    "er_read_history": (C.c_int, [_P, _FP]),
    "er_read_blended": (C.c_int, [_P, _FP]),
    "er_variance_fold": (C.c_int, [_P]),
    "er_variance_info": (C.c_int, [_P, C.POINTER(ErVarianceInfo)]),
    "er_read_variance": (C.c_int, [_P, _FP]),
    "er_denoise_variance": (C.c_int, [_P, C.POINTER(ErDenoiseVariance)]),
    "er_history_variance_info": (C.c_int, [_P, C.POINTER(ErHistoryVarianceInfo)]),
    "er_read_history_variance": (C.c_int, [_P, _FP]),
    "er_read_blended_variance": (C.c_int, [_P, _FP]),
    "er_denoise_blended": (C.c_int, [_P, C.POINTER(ErDenoiseVariance)]),
    "er_first_hit_set": (C.c_int, [_P, C.POINTER(ErFirstHitParams)]),
    "er_first_hit_info": (C.c_int, [_P, C.POINTER(ErFirstHitInfo)]),
    "er_state_size": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "er_state_export": (C.c_int, [_P, _P, C.c_uint64]),
    "er_state_import": (C.c_int, [_P, _P, C.c_uint64]),
    "er_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "er_comm_create": (C.c_int, [C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P)]),
    "er_comm_destroy": (None, [_P]),
    "er_gather_pass": (C.c_int, [_P, C.c_int, _P, C.c_uint32]),
    "er_debug_comm_create_local": (C.c_int, [C.c_uint32, C.POINTER(_P)]),
    "er_comm_create_local": (C.c_int, [C.c_uint32, C.POINTER(_P)]),
    "er_debug_stream_info": (C.c_int, [_P, C.POINTER(ErStreamInfo)]),
    "er_debug_gather_buffers": (C.c_int, [_P, C.c_uint32, C.POINTER(_P), C.POINTER(C.c_uint64), C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "er_debug_comm_loopback": (C.c_int, [_P, C.c_uint64, C.POINTER(C.c_double)]),
    "er_measure_hbm_peak": (C.c_int, [C.c_int, C.c_uint64, C.c_uint32, _FP, _FP]),
    "er_debug_eval": (C.c_int, [_P, C.c_int, _FP, C.c_uint32, C.c_uint32, _FP, C.c_uint32]),
    "er_debug_trace_rays": (C.c_int, [_P, _FP, _FP, C.c_uint32, _IP, _FP, _IP, _IP, _FP, _FP, _IP]),
    "er_debug_trace_pixel": (C.c_int, [_P, C.c_uint32, C.POINTER(ErTraceRec), C.c_int, C.POINTER(C.c_int)]),
    "er_debug_read_light_table": (C.c_int, [_P, _IP, _FP, C.c_uint32]),
    "er_debug_read_light_table_prob": (C.c_int, [_P, _IP, _FP, _FP, C.c_uint32]),
    "er_debug_read_hdri_trig": (C.c_int, [_P, _UP, C.c_uint32, _UP, C.c_uint32]),
    "er_debug_hdri_trig_host": (C.c_int, [C.c_int32, C.c_int32, _UP, _UP]),
    "er_debug_set_host_alloc_limit": (None, [C.c_uint64]),
    "er_debug_set_gpu_build_failure": (None, [C.c_int]),
    "er_debug_closest_hit": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                       C.POINTER(C.c_float)]),
}

_lib = None


class ErError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"eleven_hip error {code}: {msg}")
        self.code = code


ABI_VERSION = 2     # include/eleven_hip.h ER_ABI_VERSION

# Hooks of include/eleven_hip_debug.h that load() binds only if the library has them: tools/ab_libs.sh alternates this binding over
# older builds of the library (ELEVEN_HIP_LIB), which need not export the newest hooks.
OPTIONAL_SYMBOLS = {
    "er_debug_stream_form": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(ErStreamForm)]),
    "er_debug_stream_level": (C.c_int, [C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                        C.c_uint32, C.POINTER(C.c_uint32)]),
    "er_debug_stream_balance": (C.c_int, [_P, C.POINTER(ErStreamBalance), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32),
                                          C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32]),
    "er_debug_read_accel": (C.c_int, [_P, C.POINTER(ErAccelDump), _P, C.c_uint64, _P, C.c_uint64, _P, C.c_uint64, _P, C.c_uint64]),
    "er_debug_texture_plan": (C.c_int, [C.POINTER(ErSceneDesc), C.POINTER(ErTexturePlan), _P, C.c_uint64, _P, C.c_uint64, _P, C.c_uint64]),
    "er_debug_read_textures": (C.c_int, [_P, C.POINTER(ErTextureDump)] + [_P, C.c_uint64] * 7),
    "er_debug_bvh_dump": (C.c_int, [_FP, _FP, C.c_uint32, C.c_int, C.POINTER(ErAccelDump), _P, C.c_uint64, _P, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint64,
                                    _FP, C.c_uint64]),
    "er_debug_accel_cost_terms": (C.c_int, [_P, C.POINTER(ErCostSumsDebug), C.POINTER(C.c_double), C.c_uint64, _FP, C.c_uint64]),
    "er_debug_transform_apply": (C.c_int, [_FP, C.c_uint32, _FP, _FP, _FP, _FP, _FP, _FP]),
    "er_debug_skin_apply": (C.c_int, [_FP, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint16), _FP, _FP, _FP, _FP, _FP, _FP, _FP]),
    "er_debug_accel_cost_host": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.POINTER(ErCostSumsDebug), C.POINTER(C.c_double), C.c_uint64, _FP, C.c_uint64]),
    "er_debug_id_rank": (C.c_int, [_UP, C.c_uint32, _UP, _UP, _UP]),
    "er_debug_spill_levels": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint32, _UP]),
    "er_debug_trace_rays_levels": (C.c_int, [_P, _FP, _FP, C.c_uint32, _IP, _FP, _IP, _IP, _FP, _FP, _IP, _UP, _UP, _UP]),
    "er_debug_history_camera": (C.c_int, [_P, _FP]),
    "er_debug_history_project": (C.c_int, [_FP, C.c_uint32, C.c_uint32, C.c_uint32, _FP, _FP, _UP]),
    "er_debug_history_back_matrix": (C.c_int, [_FP, _FP, _FP]),
    "er_debug_history_taps": (C.c_int, [_FP, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, _UP, _UP, _FP, _UP, _FP, _UP, _UP, _FP, _FP, _FP, _UP, _UP]),
    "er_debug_history_capture": (C.c_int, [C.c_uint32, _FP, _UP, _FP, C.c_float, _FP]),
    "er_debug_history_blend": (C.c_int, [C.c_uint32, _FP, _UP, _FP, _FP]),
    "er_debug_variance_mark": (C.c_int, [C.c_uint32, _FP, _UP, _FP]),
    "er_debug_variance_fold": (C.c_int, [C.c_uint32, _FP, _UP, _FP, _UP]),
    "er_debug_variance_value": (C.c_int, [C.c_uint32, _FP, _UP, _FP]),
    "er_debug_variance_split": (C.c_int, [C.c_uint32, _FP, _FP, _FP]),
    "er_debug_variance_level_px": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, _FP, _FP, _FP, _FP, _FP, _FP, _FP]),
    "er_debug_history_variance_current": (C.c_int, [C.c_uint32, _FP, _FP]),
    "er_debug_history_variance_pool": (C.c_int, [C.c_uint32, _FP, _FP, _FP, _FP, _FP]),
    "er_debug_history_variance_capture": (C.c_int, [C.c_uint32, _FP, _UP, _FP, _FP, _FP]),
    "er_debug_history_variance_mean": (C.c_int, [C.c_uint32, _UP, _FP, _FP, _FP]),
    "er_debug_history_variance_taps": (C.c_int, [_FP, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, _UP, _UP, _FP, _UP, _FP, _UP, _UP, _FP, _FP, _FP, _FP, _FP, _UP, _UP]),
    "er_debug_history_variance_blend": (C.c_int, [C.c_uint32, _FP, _UP, _FP, _FP, _FP]),
    "er_debug_history_variance_split": (C.c_int, [C.c_uint32, _FP, _FP, _FP, _FP, _FP]),
    "er_debug_cutout_threshold": (C.c_int, [C.c_uint32, _FP, _UP, _FP]),
    "er_debug_cutout_stops": (C.c_int, [C.c_uint32, _FP, _FP, _UP]),
    "er_debug_cutout_continue": (C.c_int, [C.c_uint32, _FP, _FP, _FP, _FP]),
    "er_debug_first_hit_rays": (C.c_int, [_P, _FP, _FP, C.c_uint32, C.c_float, _IP, _UP, _FP, _FP]),
}


def load():
    """Load libeleven_hip.so and declare its prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ErError(ER_ERR_NO_DEVICE, f"{LIB_PATH} is missing: the HIP extension is not built "
                      "(run __graft_entry__.build()); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in OPTIONAL_SYMBOLS.items():
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    if lib.er_abi_version() != ABI_VERSION:      # the structs below are filled completely by the library: a layout mismatch overwrites memory
        raise ErError(ER_ERR_STATE, f"{LIB_PATH} has ABI version {lib.er_abi_version()}, this binding was written for {ABI_VERSION}: rebuild")
    _lib = lib
    return lib


def check(rc):
    if rc != ER_OK:
        raise ErError(rc, load().er_last_error().decode("utf-8", "replace"))


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        a = a.reshape(shape)
    return a


class SceneData:
    """A scene as flat numpy arrays (the layout of ErSceneDesc) + the ctypes descriptor.

    Keeps every array alive for as long as the descriptor is in use.  Used for BOTH the HIP
    library and (by tests/bench) the CPU oracle, so the two see bit-identical inputs.
    """

    def __init__(self, vertices, normals, tangents, uvs, tangent_sign, material_id, materials,
                 textures=(), hdri=None, hdri_cdf=None, hdri_radiance_sum=0.0, camera=None,
                 x_res=64, y_res=64, point_lights=()):
        n = 0 if vertices is None else int(np.asarray(vertices).size // 9)
        self.tri_count = n
        self.vertices = _f32(vertices if n else np.zeros((0, 3, 3)), (n, 3, 3))
        self.normals = _f32(normals if n else np.zeros((0, 3, 3)), (n, 3, 3))
        self.tangents = _f32(tangents if n else np.zeros((0, 3, 3)), (n, 3, 3))
        self.uvs = _f32(uvs if n else np.zeros((0, 3, 2)), (n, 3, 2))
        self.tangent_sign = _f32(tangent_sign if n else np.zeros((0,)), (n,))
        self.material_id = np.ascontiguousarray(material_id if n else np.zeros((0,)), dtype=np.int32).reshape(n)
        self.materials = list(materials)
        self.textures = [(_f32(d), int(w), int(h), int(ch), int(flt)) for (d, w, h, ch, flt) in textures]
        if hdri is None:   # HDRI() default: 1x1 texel (0.5,0.5,0.5), reference src/HDRI.cpp:18
            hdri = (np.full((1, 1, 3), 0.5, np.float32), 1, 1, 3, 0)
        d, w, h, ch, flt = hdri
        self.hdri = (_f32(d), int(w), int(h), int(ch), int(flt))
        self.hdri_cdf = None if hdri_cdf is None else _f32(hdri_cdf)
        self.hdri_radiance_sum = float(hdri_radiance_sum)
        self.camera = camera if camera is not None else default_camera()
        self.x_res, self.y_res = int(x_res), int(y_res)
        self.point_lights = list(point_lights)
        self._desc = None

    def desc(self):
        if self._desc is not None:
            return self._desc
        d = ErSceneDesc()
        d.tri_count = self.tri_count
        d.vertices, d.normals, d.tangents = _fptr(self.vertices), _fptr(self.normals), _fptr(self.tangents)
        d.uvs, d.tangent_sign = _fptr(self.uvs), _fptr(self.tangent_sign)
        d.material_id = self.material_id.ctypes.data_as(C.POINTER(C.c_int32))
        self._mats = (ErMaterial * len(self.materials))(*self.materials)
        d.material_count, d.materials = len(self.materials), self._mats
        self._texs = (ErTexture * max(1, len(self.textures)))()
        for i, (data, w, h, ch, flt) in enumerate(self.textures):
            self._texs[i] = ErTexture(w, h, ch, flt, _fptr(data))
        d.texture_count, d.textures = len(self.textures), self._texs
        data, w, h, ch, flt = self.hdri
        d.hdri.texture = ErTexture(w, h, ch, flt, _fptr(data))
        if self.hdri_cdf is not None:
            d.hdri.cdf = _fptr(self.hdri_cdf)
            d.hdri.radiance_sum = self.hdri_radiance_sum
        d.camera = self.camera
        self._pls = (ErPointLight * max(1, len(self.point_lights)))(*self.point_lights)
        d.point_light_count, d.point_lights = len(self.point_lights), self._pls
        d.x_res, d.y_res = self.x_res, self.y_res
        self._desc = d
        return d


def default_camera():
    """reference Camera defaults, src/Camera.h:9-19."""
    c = ErCamera()
    c.focal_length = 35 * 0.001     # evaluated in double, then narrowed, as the C++ initialisers are
    c.sensor_width = 36 * 0.001
    c.sensor_height = 24 * 0.001
    c.aperture = 2.8
    c.focus_distance = 1000000.0
    c.rotation = ErVec3(0, 0, 0)
    c.bokeh = 0
    c.position = ErVec3(0, 0, 0)
    return c


def default_material(**kw):
    """reference Material defaults, src/Material.h:20-47."""
    m = ErMaterial()
    for f in ("albedo_tex", "emission_tex", "roughness_tex", "metallic_tex", "normal_tex", "opacity_tex",
              "transmission_tex", "albedo_shader_id"):
        setattr(m, f, -1)
    m.albedo = ErVec3(0.5, 0.5, 0.5)
    m.emission = ErVec3(0, 0, 0)
    m.opacity, m.roughness, m.metallic = 1, 1, 0
    m.clearcoat_gloss = m.clearcoat = m.anisotropic = m.eta = m.transmission = 0
    m.specular, m.specular_tint, m.sheen_tint = 0.5, 0, 0.5
    m.subsurface = m.sheen = m.ax = m.ay = 0
    for k, v in kw.items():
        if isinstance(v, (tuple, list)):
            v = ErVec3(*v)
        setattr(m, k, v)
    return m
