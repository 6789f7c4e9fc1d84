"""er_render_edit / er_edit_info and the texture plan on a machine without a GPU: the symbols, the layouts of the new structs against
the C compiler's, the call-order and argument errors that need no device, and the texture plan (csrc/er_texplan.h: the one layout that
er_render_begin fills on the host and er_render_edit on the device) against modes, fusion and offsets derived by hand from its rules:

  a texture used only for scalar channels (opacity, roughness, metallic, transmission) is kept by its first channel (mode 1) if it has
  more than one; if it is unfiltered and used only as roughness / metallic it is kept to the power 2.2 (mode 2, also with one channel);
  any use as albedo, emission or normal keeps it as it came (mode 0).  A material is fused iff its albedo, roughness and metallic
  textures all exist and share size and filter (bilinear or not)."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np

from elevenrender_amd import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_torture():
    return scenes.torture(n_tris=600, x_res=32, y_res=24, n_materials=4, tex_size=16, hdri_size=(16, 8))


def edited(sc, materials=None, textures=None):
    """a copy of the description with per-material field changes {index: {field: value}} and per-texture replacements {index: tuple}"""
    out = copy.copy(sc)
    out._desc = None
    out.materials = [abi.ErMaterial.from_buffer_copy(m) for m in sc.materials]
    for i, fields in (materials or {}).items():
        for k, v in fields.items():
            setattr(out.materials[i], k, v)
    out.textures = list(sc.textures)
    for i, t in (textures or {}).items():
        out.textures[i] = t
    return out


def with_filter(t, flt):
    return (t[0], t[1], t[2], t[3], flt)


def test_library_exports_the_edit_entry_points():
    lib = abi.load()
    for name in ("er_render_edit", "er_edit_info"):
        assert hasattr(lib, name) and name in abi.SYMBOLS
    for name in ("er_debug_texture_plan", "er_debug_read_textures"):
        assert hasattr(lib, name)
    assert lib.er_abi_version() == 2          # an addition only
    assert (abi.EDIT_CAMERA, abi.EDIT_GEOMETRY, abi.EDIT_MATERIALS, abi.EDIT_TEXTURES, abi.EDIT_HDRI) == (1, 2, 4, 8, 16)
    assert (abi.EDIT_CAMERA, abi.EDIT_GEOMETRY) == (abi.UPDATE_CAMERA, abi.UPDATE_GEOMETRY)


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eleven_hip.h"\n#include "eleven_hip_debug.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u %u\\n", sizeof(ErSceneEdit), offsetof(ErSceneEdit, camera),\n'
                   '  offsetof(ErSceneEdit, vertices), offsetof(ErSceneEdit, material_count), offsetof(ErSceneEdit, materials), offsetof(ErSceneEdit, material_id),\n'
                   '  offsetof(ErSceneEdit, texture_count), offsetof(ErSceneEdit, textures), offsetof(ErSceneEdit, hdri), sizeof(ErEditInfo), offsetof(ErEditInfo, edit_ms),\n'
                   '  offsetof(ErEditInfo, pool_floats), sizeof(ErTexEntry), sizeof(ErFusedEntry), sizeof(ErTexturePlan), offsetof(ErTexturePlan, pool_floats),\n'
                   '  sizeof(ErTextureDump), ER_EDIT_MATERIALS, ER_EDIT_TEXTURES, ER_EDIT_HDRI); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    E, I, P, D = abi.ErSceneEdit, abi.ErEditInfo, abi.ErTexturePlan, abi.ErTextureDump
    assert got == [C.sizeof(E), E.camera.offset, E.vertices.offset, E.material_count.offset, E.materials.offset, E.material_id.offset, E.texture_count.offset,
                   E.textures.offset, E.hdri.offset, C.sizeof(I), I.edit_ms.offset, I.pool_floats.offset, abi.TEX_DTYPE.itemsize, abi.FUSED_DTYPE.itemsize, C.sizeof(P),
                   P.pool_floats.offset, C.sizeof(D), abi.EDIT_MATERIALS, abi.EDIT_TEXTURES, abi.EDIT_HDRI]
    assert C.sizeof(abi.ErTexEntry) == abi.TEX_DTYPE.itemsize


def test_edit_needs_a_begun_scene_and_arguments():
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    h = C.c_void_p()
    abi.check(lib.er_scene_create(C.byref(sc.desc()), C.byref(h)))
    try:
        e = abi.ErSceneEdit()
        e.what = abi.EDIT_MATERIALS
        mats = (abi.ErMaterial * len(sc.materials))(*sc.materials)
        e.material_count, e.materials = len(sc.materials), mats
        assert lib.er_render_edit(None, C.byref(e)) == abi.ER_ERR_INVALID_ARG
        assert lib.er_render_edit(h, None) == abi.ER_ERR_INVALID_ARG
        assert b"NULL" in lib.er_last_error()
        assert lib.er_render_edit(h, C.byref(e)) == abi.ER_ERR_STATE          # created, not begun
        assert b"er_render_begin" in lib.er_last_error()
        e.what = abi.EDIT_CAMERA
        assert lib.er_render_edit(h, C.byref(e)) == abi.ER_ERR_STATE
        info = abi.ErEditInfo(7, 7, 7.0, 7.0, 7)
        assert lib.er_edit_info(h, None) == abi.ER_ERR_INVALID_ARG and lib.er_edit_info(None, C.byref(info)) == abi.ER_ERR_INVALID_ARG
        assert lib.er_edit_info(h, C.byref(info)) == abi.ER_OK                # counts since er_scene_create: valid before a begin
        assert (info.edits, info.texture_stage, info.texture_stage_ms, info.edit_ms, info.pool_floats) == (0, 0, 0.0, 0.0, 0)
        assert lib.er_debug_read_textures(h, C.byref(abi.ErTextureDump()), *([None, 0] * 7)) == abi.ER_ERR_STATE
    finally:
        lib.er_scene_destroy(h)


def test_python_edit_checks_the_array_sizes():
    from elevenrender_amd import render
    rm = render.RenderingManager()
    rm.scene = scenes.cornell(16, 16)
    for kw in (dict(vertices=np.zeros((5, 3, 3), np.float32)), dict(materials=rm.scene.materials, material_id=np.zeros(5, np.int32)), dict(material_id=np.zeros(12, np.int32))):
        try:
            rm.edit(**kw)
        except ValueError:
            pass
        else:
            raise AssertionError(f"accepted: {list(kw)}")


# ---- the texture plan ----

def test_plan_modes_follow_the_uses_of_a_texture():
    sc = small_torture()      # material m: albedo 3m, roughness 3m + 1, metallic 3m + 2; 16 x 16, three channels, unfiltered
    p = abi.debug_texture_plan(sc)
    assert p["modes"].tolist() == [0, 2, 2] * 4                      # roughness-only / metallic-only, unfiltered, three channels: 2
    assert p["table"]["channels"].tolist() == [3, 1, 1] * 4 and p["table"]["filter"].tolist() == [0, 2, 2] * 4
    # texture 1 also some material's opacity: a scalar channel that is not raised to a power -> first channel alone
    p = abi.debug_texture_plan(edited(sc, materials={2: dict(opacity_tex=1)}))
    assert p["modes"].tolist() == [0, 1, 2] + [0, 2, 2] * 3 and tuple(p["table"][1])[:4] == (16, 16, 1, 0)
    # ... also some material's albedo: as it came
    p = abi.debug_texture_plan(edited(sc, materials={2: dict(albedo_tex=1)}))
    assert p["modes"].tolist() == [0, 0, 2] + [0, 2, 2] * 3 and tuple(p["table"][1])[:4] == (16, 16, 3, 0)
    assert p["modes"][6] == 0                                        # (texture 6 lost its only use: nothing to compact it for)
    # bilinear: the power can not be taken before the filter -> first channel alone, fetched filtered
    p = abi.debug_texture_plan(edited(sc, textures={1: with_filter(sc.textures[1], 1)}))
    assert p["modes"].tolist() == [0, 1, 2] + [0, 2, 2] * 3 and tuple(p["table"][1])[:4] == (16, 16, 1, 1)
    # one channel, roughness only, unfiltered: still raised to the power; with an opacity use there is nothing to compact
    one = (np.full((16, 16, 1), 0.5, np.float32), 16, 16, 1, 0)
    assert abi.debug_texture_plan(edited(sc, textures={1: one}))["modes"][1] == 2
    assert abi.debug_texture_plan(edited(sc, textures={1: one}, materials={2: dict(opacity_tex=1)}))["modes"][1] == 0


def ranges_of(p):
    out = [(int(t["offset"]), int(t["offset"]) + int(t["width"]) * int(t["height"]) * int(t["channels"])) for t in p["table"]]
    out += [(int(f["offset"]), int(f["offset"]) + 5 * int(f["width"]) * int(f["height"])) for f in p["fused"] if f["width"] > 0]
    return out


def test_plan_partitions_the_pool_and_the_hdri_lies_last():
    sc = small_torture()
    odd = (np.zeros((5, 3, 1), np.float32), 3, 5, 1, 0)
    variants = [sc, edited(sc, materials={2: dict(opacity_tex=1), 1: dict(metallic_tex=-1)}), edited(sc, textures={4: odd, 0: with_filter(sc.textures[0], 1)})]
    for v in variants:
        p = abi.debug_texture_plan(v)
        r = sorted(x for x in ranges_of(p) if x[1] > x[0])
        assert r[0][0] == 0
        for a, b in zip(r, r[1:]):
            assert a[1] == b[0], (a, b)                               # no gap, no overlap
        hd = p["hdri"]
        assert r[-1][1] == p["hdri_offset"] == hd["offset"]           # the HDRI after everything else ...
        assert p["pool_floats"] == hd["offset"] + hd["width"] * hd["height"] * hd["channels"]      # ... to the end of the pool
        assert (hd["width"], hd["height"], hd["channels"]) == (16, 8, 3)


def test_plan_shows_fusion():
    sc = small_torture()
    p = abi.debug_texture_plan(sc)
    assert (p["fused"]["width"] == 16).all() and (p["fused"]["filter"] == 2).all() and p["fused_any"] == 1
    assert p["fused"]["offset"].tolist() == [5120 + 1280 * m for m in range(4)]      # after 4 x (768 + 256 + 256) floats of textures
    no_metal = edited(sc, materials={1: dict(metallic_tex=-1)})
    p = abi.debug_texture_plan(no_metal)
    assert p["fused"]["width"].tolist() == [16, 0, 16, 16]
    assert p["modes"][5] == 0                                         # (its metallic texture is unused now)
    small = (np.zeros((8, 8, 3), np.float32), 8, 8, 3, 0)
    assert abi.debug_texture_plan(edited(sc, textures={5: small}))["fused"]["width"].tolist() == [16, 0, 16, 16]      # sizes differ
    assert abi.debug_texture_plan(edited(sc, textures={4: with_filter(sc.textures[4], 1)}))["fused"]["width"].tolist() == [16, 0, 16, 16]      # filters differ
    bil = {i: with_filter(sc.textures[i], 1) for i in (3, 4, 5)}
    p = abi.debug_texture_plan(edited(sc, textures=bil))
    assert p["fused"]["width"].tolist() == [16] * 4 and p["fused"]["filter"].tolist() == [2, 1, 2, 2]      # all three bilinear: fused, filtered
    back = edited(no_metal, materials={1: dict(metallic_tex=5)})
    q = abi.debug_texture_plan(back)
    assert q["fused"].tobytes() == abi.debug_texture_plan(sc)["fused"].tobytes()      # the metallic texture given back: the record again
    none = edited(sc, materials={m: dict(albedo_tex=-1, roughness_tex=-1, metallic_tex=-1) for m in range(4)})
    assert abi.debug_texture_plan(none)["fused_any"] == 0


def test_plan_reports_a_pool_beyond_32_bit_offsets_from_the_sizes_alone():
    d = abi.ErSceneDesc()
    texs = (abi.ErTexture * 2)(abi.ErTexture(65536, 21846, 3, 0, None), abi.ErTexture(4, 4, 3, 0, None))      # declared, no texels behind them
    mats = (abi.ErMaterial * 1)(abi.default_material(albedo_tex=0, emission_tex=1))
    d.material_count, d.materials = 1, mats
    d.texture_count, d.textures = 2, texs
    d.hdri.texture = abi.ErTexture(1, 1, 3, 0, None)
    p = abi.debug_texture_plan(d)
    assert p["pool_floats"] == 65536 * 21846 * 3 + 48 + 3 and p["pool_floats"] >= 2 ** 32
    texs[0].height = 21845
    p = abi.debug_texture_plan(d)
    assert p["pool_floats"] == 65536 * 21845 * 3 + 48 + 3 and p["pool_floats"] < 2 ** 32


# ---- the host server's rule ----

def test_host_edits_in_place_after_nothing_but_camera_hdri_materials_and_textures():
    """eleven::SessionEdits through tests/native/session_scene_edits.cpp: s / f = a --start that succeeds / fails, c = --load_camera,
    h = --load_hdri, m = --load_brdf_material or --load_texture, o = --load_object or --load_config; per --start c = in-place camera
    update, e = in-place scene edit, 0 = the full start."""
    exe = os.path.join(ROOT, "tests", "native", "session_scene_edits")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "native", "session_scene_edits.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "elevenrender_amd"), "-leleven_hip", "-Wl,-rpath,$ORIGIN/../../elevenrender_amd"])
    sessions = {"ochms": "0",            # the first start of a session builds
                "ochmshs": "0e",         # a new HDRI alone: edited in place
                "ochmsms": "0e",         # a material or a texture
                "ochmschms": "0e",       # all of them, the camera too
                "ochmscs": "0c",         # a camera alone stays the camera update
                "ochmss": "0c",          # ... and so does no edit at all
                "ochmshos": "00",        # an object or a configuration: full start, whatever else came
                "ochmsohs": "00",
                "ochmshsms": "0ee",      # the flags clear with the start that consumed them
                "ochmshscs": "0ec",
                "ochfhs": "00",          # a start that failed left nothing to edit
                "ochmshfhs": "0e0"}      # ... nor does an edit that failed
    out = subprocess.check_output([exe] + list(sessions), text=True).split("\n")
    assert dict(zip(sessions, out)) == sessions
