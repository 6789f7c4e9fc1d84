"""er_render_edit on the GPU: materials, textures and the HDRI of a begun scene edited in place, against the contract of
include/eleven_hip.h -- every readable output equals a fresh er_scene_create + er_render_begin of the edited description, bit for bit --
and, for everything the texture, material and HDRI stages leave in device memory (er_debug_read_textures), byte for byte: the device
fill of the texture pool (csrc/er_texstage.hip) against the host fill of er_render_begin.

The pattern is tests/test_gpu_update.py's: 4 spp, the edit, compare with a fresh manager of the edited SceneData, 4 spp more, compare
again.  Scenes: cornell_textured(48, 48); T, the small torture scene (600 triangles, 4 materials of three 16 x 16 textures each, a
16 x 8 HDRI) at 64 x 48; TP, T with its texture list prefixed by a one-channel 3 x 5 texture (material 3's opacity) and a 24 x 20 texture
(material 3's transmission: kept by its first channel) -- every later pool offset is odd, and 480 texels are no multiple of a workgroup."""
import copy
import ctypes as C
import time

import numpy as np
import pytest

from elevenrender_amd import abi, client, render, scenes
from test_gpu_update import SCHEDULES, assert_same_outputs, edit_J, manager, moved_camera, outputs

pytestmark = pytest.mark.gpu

DUMP_ARRAYS = ("table", "pool", "fused", "mat_pre", "materials", "cdf", "guide")
DUMP_FIELDS = ("hdri_tex", "hdri_buckets", "tex_pow2", "fused_any")


def T():
    return scenes.torture(n_tris=600, x_res=64, y_res=48, n_materials=4, tex_size=16, hdri_size=(16, 8))


def noise(w, h, ch, seed, flt=0):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w, ch), dtype=np.float32), w, h, ch, flt)


def TP():
    sc = T()
    sc.textures = [noise(3, 5, 1, 11), noise(24, 20, 3, 12)] + sc.textures
    for m in sc.materials:
        for f in ("albedo_tex", "roughness_tex", "metallic_tex"):
            setattr(m, f, getattr(m, f) + 2)
    sc.materials[3].opacity_tex = 0
    sc.materials[3].transmission_tex = 1
    sc._desc = None
    return sc


def changed(sc, materials=None, textures=None, material_id=None, hdri=None, hdri_cdf=None, hdri_radiance_sum=0.0, camera=None, **arrays):
    """a copy of the description: per-material field changes {index: {field: value}} (or a whole new list), per-texture replacements
    {index: tuple} (an index past the end appends), new material ids, a new HDRI, a new camera, new triangle arrays"""
    out = copy.copy(sc)
    out._desc = None
    if isinstance(materials, list):
        out.materials = [abi.ErMaterial.from_buffer_copy(m) for m in materials]
    else:
        out.materials = [abi.ErMaterial.from_buffer_copy(m) for m in sc.materials]
        for i, fields in (materials or {}).items():
            for k, v in fields.items():
                setattr(out.materials[i], k, abi.ErVec3(*v) if isinstance(v, tuple) else v)
    out.textures = list(sc.textures)
    for i, t in sorted((textures or {}).items()):
        t = (abi._f32(t[0]), int(t[1]), int(t[2]), int(t[3]), int(t[4]))
        if i == len(out.textures):
            out.textures.append(t)
        else:
            out.textures[i] = t
    if material_id is not None:
        out.material_id = np.ascontiguousarray(material_id, np.int32)
    if hdri is not None:
        out.hdri = (abi._f32(hdri[0]),) + tuple(int(x) for x in hdri[1:])
        out.hdri_cdf = None if hdri_cdf is None else abi._f32(hdri_cdf)
        out.hdri_radiance_sum = float(hdri_radiance_sum)
    if camera is not None:
        out.camera = camera
    for k, v in arrays.items():
        setattr(out, k, np.ascontiguousarray(np.asarray(v, np.float32).reshape(getattr(sc, k).shape)))
    return out


def edit_args(old, new, camera=False, geometry=False):
    """the arguments of RenderingManager.edit that turn `old` into `new`: the complete material list if a material differs, the texture
    list with None for the textures that are the same objects, the HDRI if it is another object"""
    kw = {}
    same_mats = len(old.materials) == len(new.materials) and all(bytes(a) == bytes(b) for a, b in zip(old.materials, new.materials))
    if not same_mats or new.material_id is not old.material_id:
        kw["materials"] = new.materials
        if new.material_id is not old.material_id:
            kw["material_id"] = new.material_id
    if len(new.textures) != len(old.textures) or any(a is not b for a, b in zip(old.textures, new.textures)):
        kw["textures"] = [None if i < len(old.textures) and t is old.textures[i] else t for i, t in enumerate(new.textures)]
    if new.hdri is not old.hdri:
        kw.update(hdri=new.hdri, hdri_cdf=new.hdri_cdf, hdri_radiance_sum=new.hdri_radiance_sum)
    if camera:
        kw["camera"] = new.camera
    if geometry:
        kw.update(vertices=new.vertices, normals=new.normals)
    return kw


def assert_same_dump(a, b, what, skip=()):
    for k in DUMP_ARRAYS:
        if k in skip:
            continue
        assert a[k].shape == b[k].shape, f"{what}: {k} has shape {a[k].shape}, fresh {b[k].shape}"
        diff = int((a[k].view(np.uint8) != b[k].view(np.uint8)).sum())
        assert diff == 0, f"{what}: {k} differs in {diff} bytes"
    for k in DUMP_FIELDS:
        assert a[k] == b[k], f"{what}: {k}: {a[k]} / fresh {b[k]}"
    assert a["hdri_radiance_sum"].tobytes() == b["hdri_radiance_sum"].tobytes(), what


def step(rm, old, new, flags=0, rank=0, world=1, stage=None, what="", **flags_of_args):
    """4 spp on rm (begun on `old`), the edit to `new`, everything compared with a fresh manager of `new`, 4 spp on both, compared
    again.  Returns the fresh manager, with 4 spp (the caller closes it)."""
    rm.render(4)
    rm.edit(**edit_args(old, new, **flags_of_args))
    info = rm.edit_info()
    if stage is not None:
        assert info["texture_stage"] == stage, (what, info)
    fresh = manager(new, flags, rank, world)
    try:
        assert rm.get_render_info().samples == fresh.get_render_info().samples
        assert rm.adaptive_info() == fresh.adaptive_info() and rm.adaptive_info()["enabled"] == 0
        assert_same_outputs(outputs(rm), outputs(fresh), what + ": right after the edit")
        dump = rm.debug_read_textures()
        assert_same_dump(dump, fresh.debug_read_textures(), what)
        if info["edits"]:
            assert info["pool_floats"] == len(dump["pool"])
        rm.render(4)
        fresh.render(4)
        assert_same_outputs(outputs(rm), outputs(fresh), what + ": 4 spp later")
        assert rm.counters() == fresh.counters()
        assert rm.get_render_info().samples == fresh.get_render_info().samples == 5
        assert rm.light_info() == fresh.light_info()
    except BaseException:
        fresh.close()
        raise
    return fresh


def one_edit(old, new, flags=0, rank=0, world=1, stage=None, what="", **kw):
    rm = manager(old, flags, rank, world)
    try:
        step(rm, old, new, flags, rank, world, stage, what, **kw).close()
        return rm.edit_info(), rm.update_info()
    finally:
        rm.close()


# ---- the comparison itself ----

def test_the_byte_comparison_sees_one_texel():
    """negative control: the dumps of two fresh scenes that differ in the last bit of one texel -- of a texture kept to the power 2.2
    that also feeds a fused record -- differ, in the pool alone"""
    sc = TP()
    d = sc.textures[3][0].copy()
    d[7, 9, 0] = np.nextafter(d[7, 9, 0], np.float32(2.0))
    a, b = manager(sc), manager(changed(sc, textures={3: (d,) + sc.textures[3][1:]}))
    try:
        da, db = a.debug_read_textures(), b.debug_read_textures()
    finally:
        a.close()
        b.close()
    assert int((da["pool"].view(np.uint32) != db["pool"].view(np.uint32)).sum()) == 2      # the texture's own entry and material 0's record
    with pytest.raises(AssertionError, match="pool differs"):
        assert_same_dump(da, db, "one texel")
    assert_same_dump(da, db, "one texel", skip=("pool",))


# ---- constants ----

@pytest.mark.parametrize("name", ["TP", "cornell_textured"])
def test_an_edit_of_constants_leaves_the_pool_alone(name):
    sc = TP() if name == "TP" else scenes.cornell_textured(48, 48)
    new = changed(sc, materials={0: dict(albedo=(0.2, 0.7, 0.4), roughness=0.35, clearcoat_gloss=0.8), 1: dict(metallic=0.6, opacity=0.9, clearcoat_gloss=1.0),
                                 3: dict(roughness=0.0, metallic=1.0, albedo=(0.9, 0.9, 0.1))})
    rm = manager(sc)
    try:
        before = rm.debug_read_textures()
        fresh = step(rm, sc, new, stage=0, what=name)
        after, fresh_dump = rm.debug_read_textures(), fresh.debug_read_textures()
        fresh.close()
        for k in ("pool", "table", "fused"):
            assert before[k].tobytes() == after[k].tobytes(), k
        assert after["mat_pre"].tobytes() == fresh_dump["mat_pre"].tobytes() and after["materials"].tobytes() == fresh_dump["materials"].tobytes()
        assert before["mat_pre"].tobytes() != after["mat_pre"].tobytes()
        info = rm.edit_info()
        assert info["edits"] == 1 and info["texture_stage_ms"] == 0.0 and rm.update_info()["updates"] == 1
    finally:
        rm.close()


# ---- assignments ----

def assignment_chain(sc):
    """the descriptions after each of the assignment edits, cumulative.  In TP material m has albedo 3m + 2, roughness 3m + 3, metallic
    3m + 4."""
    s1 = changed(sc, materials={0: dict(roughness_tex=5)})       # material 0's roughness <- material 1's albedo: texture 3 unused (2 -> 0), the record raises a raw value
    s2 = changed(s1, materials={1: dict(metallic_tex=-1)})       # fusion on -> off; texture 7 unused (2 -> 0)
    s3 = changed(s2, materials={2: dict(opacity_tex=9)})         # material 2's roughness texture also its opacity (2 -> 1)
    s4 = changed(s3, materials={1: dict(metallic_tex=7)})        # fusion off -> on; texture 7 (0 -> 2)
    s5 = changed(s4, materials={2: dict(opacity_tex=-1)})        # (1 -> 2)
    s6 = changed(s5, materials={0: dict(transmission_tex=3)})    # the unused texture 3 as a scalar channel (0 -> 1)
    s7 = changed(s6, materials={0: dict(transmission_tex=-1)})   # (1 -> 0)
    return [sc, s1, s2, s3, s4, s5, s6, s7]


def test_the_assignment_edits_cover_every_transition():
    """(no render: the plans alone) every mode transition and fusion on -> off and off -> on occur in the chain the next test runs"""
    chain = assignment_chain(TP())
    plans = [abi.debug_texture_plan(s) for s in chain]
    moves, fusion = set(), set()
    for a, b in zip(plans, plans[1:]):
        moves |= {(int(x), int(y)) for x, y in zip(a["modes"], b["modes"]) if x != y}
        fusion |= {(bool(x), bool(y)) for x, y in zip(a["fused"]["width"], b["fused"]["width"]) if bool(x) != bool(y)}
    assert moves == {(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)} and fusion == {(True, False), (False, True)}
    assert plans[1]["fused"]["width"][0] == 16 and plans[1]["table"][5]["filter"] == 0      # a fused record whose roughness comes from a texture kept as it came
    assert plans[3]["fused"]["width"][2] == 16 and plans[3]["table"][9]["filter"] == 0 and plans[3]["modes"][9] == 1      # ... and from one kept by its raw first channel
    assert all(p["hdri_offset"] % 2 == 1 for p in plans)          # the prefix makes the offsets odd


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_assignment_edits_equal_fresh_scenes(schedule):
    chain = assignment_chain(TP())
    flags = SCHEDULES[schedule]
    rm = manager(chain[0], flags)
    try:
        for i in range(1, len(chain)):
            step(rm, chain[i - 1], chain[i], flags, stage=2, what=f"assignment edit {i} / {schedule}").close()
        assert rm.edit_info()["edits"] == len(chain) - 1 and rm.edit_info()["texture_stage_ms"] > 0.0
    finally:
        rm.close()
    one_edit(chain[0], chain[4], flags, stage=2, what=f"the four assignment edits in one / {schedule}")


# ---- textures ----

def texture_case(name):
    if name == "not-a-power-of-two":          # T: every side a power of two until this edit
        sc = T()
        return sc, changed(sc, textures={0: noise(24, 20, 3, 21)})
    sc = TP()
    if name == "one-channel":                 # material 0's roughness texture: one channel, still raised to the power
        return sc, changed(sc, textures={3: noise(16, 16, 1, 22)})
    if name == "bilinear":                    # the same texels, filtered: the record goes, the texture is kept by its raw first channel
        return sc, changed(sc, textures={3: sc.textures[3][:4] + (1,)})
    if name == "appended":                    # a new texture at the end, material 1's roughness
        return sc, changed(sc, textures={len(sc.textures): noise(16, 16, 3, 23)}, materials={1: dict(roughness_tex=len(sc.textures))})
    if name == "one-texel":
        return sc, changed(sc, textures={10: noise(1, 1, 3, 24)})
    if name == "fused-480-texels":            # material 1 fused at 24 x 20, its roughness texture of one channel
        return sc, changed(sc, textures={5: noise(24, 20, 3, 25), 6: noise(24, 20, 1, 26), 7: noise(24, 20, 4, 27)})
    if name == "all-bilinear":                # material 2's three textures filtered: a fused record without powers
        return sc, changed(sc, textures={i: sc.textures[i][:4] + (1,) for i in (8, 9, 10)})
    if name == "cornell":
        sc = scenes.cornell_textured(48, 48)
        return sc, changed(sc, textures={0: noise(24, 20, 3, 28)})
    raise KeyError(name)


@pytest.mark.parametrize("name", ["not-a-power-of-two", "one-channel", "bilinear", "appended", "one-texel", "fused-480-texels", "all-bilinear", "cornell"])
def test_texture_edits_equal_fresh_scenes(name):
    old, new = texture_case(name)
    po, pn = abi.debug_texture_plan(old), abi.debug_texture_plan(new)
    if name == "fused-480-texels":
        assert pn["fused"]["width"][1] == 24 and pn["fused"]["height"][1] == 20 and pn["fused"]["offset"][1] % 2 == 1
    if name == "one-texel":
        assert po["fused"]["width"][2] == 16 and pn["fused"]["width"][2] == 0 and pn["modes"][10] == 2
    if name == "all-bilinear":
        assert pn["fused"]["filter"][2] == 1
    rm = manager(old)
    try:
        pow2_before = rm.debug_read_textures()["tex_pow2"]
        step(rm, old, new, stage=2, what=name).close()
        if name == "not-a-power-of-two":
            assert pow2_before == 1 and rm.debug_read_textures()["tex_pow2"] == 0
        assert rm.edit_info()["texture_stage_ms"] > 0.0
    finally:
        rm.close()


# ---- HDRI ----

def test_hdri_edits_rewrite_the_tail_of_the_pool():
    sc = TP()
    cdf = np.linspace(0.0, 1.0, 16 * 8 + 1).astype(np.float32)      # a caller's own CDF: uniform, not the library's
    chain = [sc, changed(sc, hdri=scenes.sky_hdri(32, 16)), None, None]
    chain[2] = changed(chain[1], hdri=(np.array([[[0.3, 0.5, 0.9]]], np.float32), 1, 1, 3, 0))
    chain[3] = changed(chain[2], hdri=noise(16, 8, 3, 31), hdri_cdf=cdf, hdri_radiance_sum=3.5)
    rm = manager(sc)
    try:
        head = rm.debug_read_textures()
        off = head["hdri_tex"]["offset"]
        for i in range(1, len(chain)):
            step(rm, chain[i - 1], chain[i], stage=1, what=f"hdri edit {i}").close()
            now = rm.debug_read_textures()
            assert now["hdri_tex"]["offset"] == off and now["pool"][:off].tobytes() == head["pool"][:off].tobytes()
            assert now["table"].tobytes() == head["table"].tobytes() and now["fused"].tobytes() == head["fused"].tobytes()
            w, h = chain[i].hdri[1], chain[i].hdri[2]
            assert (now["hdri_tex"]["width"], now["hdri_tex"]["height"]) == (w, h) and len(now["cdf"]) == w * h + 1
            assert now["pool"][off:].tobytes() == chain[i].hdri[0].tobytes()
        assert now["cdf"].tobytes() == cdf.tobytes() and now["hdri_radiance_sum"] == np.float32(3.5)
        assert rm.edit_info()["edits"] == 3
    finally:
        rm.close()


# ---- the wire's case: a longer material list, the triangles pointed at the new entries ----

def material_by_triangle(rm, n):
    d = rm.debug_read_accel()
    out = np.full(n, -1, np.int32)
    out[d["isect"]["tri_id"][:n]] = d["attr"]["material"]
    return out


def test_a_grown_material_list_with_new_material_ids():
    sc = TP()
    extra = abi.ErMaterial.from_buffer_copy(sc.materials[1])
    extra.albedo_tex, extra.albedo = -1, abi.ErVec3(0.1, 0.3, 0.9)
    ids = np.where(sc.material_id == 1, 4, sc.material_id).astype(np.int32)
    ids[::7] = 2
    new = changed(sc, materials=sc.materials + [extra], material_id=ids)
    rm = manager(sc)
    try:
        fresh = step(rm, sc, new, stage=2, what="grown list")
        got, want = material_by_triangle(rm, sc.tri_count), material_by_triangle(fresh, sc.tri_count)
        fresh.close()
        assert got.tolist() == want.tolist() == ids.tolist()
    finally:
        rm.close()


def test_new_material_ids_alone_are_a_constants_edit():
    sc = scenes.cornell_textured(48, 48)
    ids = sc.material_id.copy()
    ids[4:6] = 2      # the back wall green
    new = changed(sc, material_id=ids)
    rm = manager(sc)
    try:
        fresh = step(rm, sc, new, stage=0, what="ids alone")
        assert material_by_triangle(rm, sc.tri_count).tolist() == material_by_triangle(fresh, sc.tri_count).tolist() == ids.tolist()
        fresh.close()
    finally:
        rm.close()


# ---- mesh lights ----

def test_mesh_lights_follow_the_materials():
    sc = scenes.cornell(48, 48)
    lit_wall = changed(sc, materials={1: dict(emission=(0.5, 2.0, 0.5))})            # the red wall emits: 2 -> 4 emitters
    dark = changed(sc, materials={3: dict(emission=(0.0, 0.0, 0.0))})                # no emitter left: the table is empty, the query record goes
    flags = abi.FLAG_MESH_LIGHTS
    for old, new, emitters in ((sc, lit_wall, 4), (sc, dark, 0), (dark, sc, 2), (lit_wall, dark, 0)):
        rm = manager(old, flags)
        try:
            fresh = step(rm, old, new, flags, stage=0, what=f"{emitters} emitters")
            assert rm.light_info() == fresh.light_info() and rm.light_info()["emitters"] == emitters
            (tri_a, cdf_a), (tri_b, cdf_b) = rm.debug_light_table(), fresh.debug_light_table()
            fresh.close()
            assert tri_a.tolist() == tri_b.tolist() and cdf_a.tobytes() == cdf_b.tobytes()
        finally:
            rm.close()


# ---- everything at once ----

def all_bits(sc):
    new = changed(sc, camera=moved_camera(sc), hdri=scenes.sky_hdri(32, 16), textures={3: noise(24, 20, 3, 41), 12: noise(16, 16, 2, 42)},
                  materials={0: dict(roughness_tex=5, albedo=(0.3, 0.3, 0.8)), 2: dict(opacity_tex=9, roughness=0.4), 3: dict(metallic_tex=-1)}, **edit_J(sc))
    return new


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_all_bits_in_one_call(schedule):
    sc = TP()
    info, upd = one_edit(sc, all_bits(sc), SCHEDULES[schedule], stage=2, what=f"all bits / {schedule}", camera=True, geometry=True)
    assert info["edits"] == 1 and upd["updates"] == 1 and upd["refits"] == 1


def test_all_bits_on_rank_1_of_3():
    sc = TP()
    one_edit(sc, all_bits(sc), 0, rank=1, world=3, stage=2, what="all bits, rank 1 of 3", camera=True, geometry=True)


def test_camera_and_geometry_alone_are_an_update():
    sc = TP()
    new = changed(sc, camera=moved_camera(sc), **edit_J(sc))
    info, upd = one_edit(sc, new, what="the first two bits", camera=True, geometry=True)
    assert info["edits"] == 0 and upd["updates"] == 1 and upd["refits"] == 1 and upd["update_ms"] > 0.0


# ---- adaptive sampling, feature planes, edits in a row ----

def test_an_edit_turns_adaptive_sampling_off_and_invalidates_the_feature_planes():
    sc = TP()
    new = changed(sc, materials={0: dict(albedo=(0.9, 0.2, 0.2))})
    rm = manager(sc)
    try:
        rm.set_adaptive(1e-3, 3, 1)
        rm.render_features(2)
        assert rm.feature_info()["valid"] == 1 and rm.adaptive_info()["enabled"] == 1
        fresh = step(rm, sc, new, stage=0, what="after an adaptive render")
        assert rm.adaptive_info()["enabled"] == 0 and rm.feature_info()["valid"] == 0
        rm.render_features(2)
        fresh.render_features(2)
        assert rm.feature_info()["valid"] == 1
        for f in ("albedo", "depth"):
            assert rm.get_feature(f).tobytes() == fresh.get_feature(f).tobytes(), f
        fresh.close()
    finally:
        rm.close()


def test_two_edits_in_a_row_equal_one_fresh_scene():
    sc = TP()
    mid = changed(sc, textures={3: noise(16, 16, 1, 51)}, materials={1: dict(metallic_tex=-1)})
    new = changed(mid, hdri=scenes.sky_hdri(32, 16), materials={1: dict(metallic_tex=7, metallic=0.3)})
    rm = manager(sc)
    try:
        rm.render(2)
        rm.edit(**edit_args(sc, mid))
        step(rm, mid, new, stage=2, what="the second edit").close()
        assert rm.edit_info()["edits"] == 2 and rm.update_info()["updates"] == 2
    finally:
        rm.close()


# ---- refusals ----

def test_refused_edits_leave_the_render_as_it_was():
    sc = TP()
    rm, twin = manager(sc), manager(sc)
    try:
        rm.render(2)
        twin.render(2)
        n_tex, n_mat = len(sc.textures), len(sc.materials)
        mats = (abi.ErMaterial * n_mat)(*sc.materials)
        texs = (abi.ErTexture * (n_tex + 1))()      # all data NULL: keep
        ids = sc.material_id.copy()
        px = abi._f32(np.zeros((4, 4, 3)))
        big = abi._f32(np.zeros(4))
        fp = abi._fptr

        def refused(what, **fields):
            e = abi.ErSceneEdit()
            e.what = what
            for k, v in fields.items():
                setattr(e, k, v)
            rc = rm.lib.er_render_edit(rm.handle, C.byref(e))
            assert rc == abi.ER_ERR_INVALID_ARG, (what, list(fields), rc, rm.lib.er_last_error())
            assert rm.edit_info()["edits"] == 0 and rm.update_info()["updates"] == 0

        refused(0)                                                                            # nothing named
        refused(32)                                                                           # an unknown bit
        refused(abi.EDIT_MATERIALS | 64, material_count=n_mat, materials=mats)
        refused(abi.EDIT_GEOMETRY | abi.EDIT_MATERIALS, material_count=n_mat, materials=mats)  # a bit without its array: vertices
        refused(abi.EDIT_MATERIALS, material_count=n_mat)                                     # ... materials
        refused(abi.EDIT_TEXTURES, texture_count=n_tex)                                       # ... textures
        refused(abi.EDIT_HDRI)                                                                # ... the HDRI's texels
        refused(abi.EDIT_MATERIALS, material_count=0, materials=mats)
        refused(abi.EDIT_TEXTURES, texture_count=n_tex - 1, textures=texs)                    # fewer textures than the scene has
        refused(abi.EDIT_TEXTURES, texture_count=n_tex + 1, textures=texs)                    # keep a texture the scene does not have
        for bad in (abi.ErTexture(0, 4, 3, 0, fp(px)), abi.ErTexture(4, -1, 3, 0, fp(px)), abi.ErTexture(4, 4, -1, 0, fp(px))):      # what er_scene_create refuses
            texs[2] = bad
            refused(abi.EDIT_TEXTURES, texture_count=n_tex, textures=texs)
            hd = abi.ErHdri()
            hd.texture = bad
            refused(abi.EDIT_HDRI, hdri=hd)
        texs[2] = abi.ErTexture()
        ids[17] = n_mat
        refused(abi.EDIT_MATERIALS, material_count=n_mat, materials=mats, material_id=ids.ctypes.data_as(C.POINTER(C.c_int32)))      # beyond the list
        ids[17] = -1
        refused(abi.EDIT_MATERIALS, material_count=n_mat, materials=mats, material_id=ids.ctypes.data_as(C.POINTER(C.c_int32)))
        refused(abi.EDIT_MATERIALS, material_count=n_mat - 1, materials=mats)                 # the kept ids point beyond a shorter list
        mats[1].normal_tex = n_tex
        refused(abi.EDIT_MATERIALS, material_count=n_mat, materials=mats)                     # a texture id er_scene_create refuses
        mats[1].normal_tex = -1
        texs[2] = abi.ErTexture(65536, 21846, 3, 0, fp(big))                                  # 2^32 floats and more: refused on the plan, before a texel is read
        refused(abi.EDIT_TEXTURES, texture_count=n_tex, textures=texs)
        hd = abi.ErHdri()
        hd.texture = abi.ErTexture(65536, 21846, 3, 0, fp(big))
        refused(abi.EDIT_HDRI, hdri=hd)
        v = sc.vertices.copy()
        v.reshape(-1)[100] = np.inf
        with pytest.raises(abi.ErError) as err:
            rm.edit(vertices=v, materials=sc.materials)
        assert err.value.code == abi.ER_ERR_INVALID_ARG and "finite" in str(err.value)
        assert rm.edit_info() == twin.edit_info()
        rm.render(2)
        twin.render(2)
        assert_same_outputs(outputs(rm), outputs(twin), "after refused edits")
        assert_same_dump(rm.debug_read_textures(), twin.debug_read_textures(), "after refused edits")
    finally:
        rm.close()
        twin.close()


# ---- host ----

def test_host_session_answers_material_and_hdri_loads_by_an_edit():
    """start, get_pass, load_hdri (new pixels), load_brdf_material of a second "floor", start, get_pass through eleven_server: the second
    pass equals that of a session that loaded the new HDRI and the five materials from the beginning, and the server took the edit
    path (get_info: scene_edits)."""
    from test_host_server import Server

    def wait_for(c, samples):
        deadline = time.time() + 120
        while c.get_info()["samples"] < samples + 1:      # (every poll is a round trip to the server: no sleep between them)
            assert time.time() < deadline, "render did not reach the sample target"

    a = client.cornell_session_assets(48, 48)
    new_hdri = (0.2 + np.random.default_rng(9).random((8, 16, 3))).astype(np.float32)
    floor2 = dict(name="floor", albedo=dict(r=0.2, g=0.4, b=0.9), roughness=0.5)
    s = Server()
    c = client.Client(port=s.port)
    first_img = client.play_cornell_session(c, a, sample_target=4)
    assert c.get_info()["scene_edits"] == 0
    c.load_hdri(new_hdri)
    c.load_brdf_material(**floor2)
    c.start()
    wait_for(c, 4)
    edited = c.get_pass("beauty", 48, 48)
    info = c.get_info()
    c.close()
    assert s.finish() == 0
    assert info["scene_edits"] == 1 and info["camera_updates"] == 0 and info["samples"] == 5
    s = Server()
    c = client.Client(port=s.port)
    ref = client.play_cornell_session(c, dict(a, hdri=new_hdri, materials=a["materials"] + [floor2]), sample_target=4)
    info = c.get_info()
    assert info["scene_edits"] == 0 and info["camera_updates"] == 0
    c.close()
    assert s.finish() == 0
    assert (edited.view(np.uint32) == ref.view(np.uint32)).all()
    assert (edited.view(np.uint32) != first_img.view(np.uint32)).any()
