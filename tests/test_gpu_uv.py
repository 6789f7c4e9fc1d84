"""Texture coordinates that vary, tile and go negative, and mirrored tangent signs, on the GPU against the oracle, bit for bit.

Every other scene of the suite gives each triangle the unit triangle as uvs and +1 as sign (tests/uv_scenes.py says what that hides).
Here: the hit record of full_hit (csrc/er_device.h) on per-triangle mappings; whole paths on two textured scenes, one per branch of
wrap_abs, whose texture plans cover the fused, compacted, pre-powered and as-it-came fetches of generate_hit_data, in the three
schedules, under the plan's knobs, bounce by bounce, and with point lights; and the edits of a begun scene (topology, sparse, transform,
rebuild), after which every triangle must still hold its OWN uvs and sign.  tests/test_uv_scenes_cpu.py shows on the oracle alone that
the frames' rays reach coordinates outside [0, 1]^2, negative ones, ones several periods out, every material and both signs.
(The albedo feature plane on these scenes: tests/test_gpu_features.py; the structure's records: "varied-*" in tests/test_gpu_accel_structure.py;
recorded vectors of the reference's own Tri::hit: tests/test_gpu_reference_kat.py.)"""
import ctypes as C
import functools

import numpy as np
import pytest

import accel_check
import uv_scenes
from elevenrender_amd import abi, render, scenes
from test_gpu_function_kat import FN, ibits, same
from test_gpu_function_level import _rec_tuple
from test_gpu_mesh_lights import MESH, numpy_table, textured_scene
from test_gpu_mesh_lights import run as run_lights
from test_gpu_mesh_lights import same as same_lights
from test_gpu_parity import compare, gpu_render, oracle_render
from test_gpu_rebuild import assert_same_structure as assert_same_as_fresh_structure
from test_gpu_stream_handoff import COUNTS, assert_no_bit_differs
from test_gpu_stream_handoff import run as run_counted
from test_gpu_topology import edit as topology_edit
from test_gpu_topology import tail_of
from test_gpu_transform import centre_of, matrix, rotation, soup_objects
from test_gpu_transform import both as transform_both
from test_gpu_transform import pair as transform_pair
from test_gpu_update import SCHEDULES, assert_same_outputs, edit_J, manager, outputs, with_arrays
from test_gpu_update_sparse import assert_same_structure as assert_same_as_twin_structure
from test_gpu_update_sparse import both as sparse_both
from test_gpu_update_sparse import pair as sparse_pair
from test_gpu_update_sparse import tris

pytestmark = pytest.mark.gpu

SPP, BOUNCES = 5, 8
LIGHTS = abi.FLAG_POINT_LIGHTS | abi.FLAG_MIS
KINDS = list(uv_scenes.KINDS)


# ---- the hit record ----

def test_hit_records_with_varied_uvs_and_signs(oracle_mod):
    """ER_FN_TRI_HIT against oracle_tri_hit (src/Tri.h:60-140) fed the same per-triangle uvs and signs: all 18 outputs of 3 000 rays aimed
    as in test_gpu_function_kat.py::test_tri_hit_records, through vertices and along edges too.  With the unit triangle tu = u and tv = v,
    whatever the association order or the corner order; here they are not."""
    sc = uv_scenes.varied(scenes.torture(600, 48, 36, seed=9, n_materials=4, tex_size=16, hdri_size=(64, 32), smooth=True, n_lights=0), 17)
    rm = render.RenderingManager(render.RenderParameters(max_bounces=8))
    rm.start_rendering(sc)
    try:
        r = np.random.default_rng(2)
        n = 3000
        tri = r.integers(0, sc.tri_count, n)
        tri[:70] = np.repeat(np.arange(len(uv_scenes.SPECIAL)), 10)      # ten rays at each of the special mappings
        v = sc.vertices.reshape(-1, 3, 3)[tri]
        w = r.dirichlet([1, 1, 1], n).astype(np.float32)
        w[::10] = [1, 0, 0]                                          # through a vertex; [::11] along an edge
        w[::11, 2] = 0
        target = (v * w[:, :, None]).sum(1).astype(np.float32)
        origin = (target + r.normal(size=(n, 3)).astype(np.float32) * np.float32(0.7)).astype(np.float32)
        d = target - origin
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        items = np.concatenate([ibits(tri.astype(np.int32)).reshape(-1, 1), origin, d], 1)
        out = rm.debug_eval(FN["TRI_HIT"], items, 18)
    finally:
        rm.close()
    L = oracle_mod.lib()
    fp = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    refs, hit = np.zeros((n, 17), np.float32), np.zeros(n, bool)
    for k in range(n):
        t = int(tri[k])
        hit[k] = bool(L.oracle_tri_hit(fp(sc.vertices.reshape(-1, 9)[t]), fp(sc.normals.reshape(-1, 9)[t]), fp(sc.tangents.reshape(-1, 9)[t]),
                                       fp(sc.uvs.reshape(-1, 6)[t]), float(sc.tangent_sign[t]), fp(origin[k]), fp(d[k]), fp(refs[k])))
    assert ((out[:, 0] == 1.0) == hit).all(), np.nonzero((out[:, 0] == 1.0) != hit)[0][:5]
    bad = np.nonzero(hit & ~same(out[:, 1:], refs).all(1))[0]
    assert len(bad) == 0, (len(bad), [(int(k), int(tri[k]), out[k, 1:], refs[k]) for k in bad[:3]])
    assert hit.sum() > n // 2 and hit[:70].sum() >= 35
    # the coordinates are no copy of the barycentrics, as they are under the unit mapping (tu = u, tv = v): Moeller-Trumbore in float64
    tu, tv = refs[hit, 15], refs[hit, 16]
    vv = sc.vertices.reshape(-1, 3, 3)[tri[hit]].astype(np.float64)
    o64, d64 = origin[hit].astype(np.float64), d[hit].astype(np.float64)
    e1, e2 = vv[:, 1] - vv[:, 0], vv[:, 2] - vv[:, 0]
    h = np.cross(d64, e2)
    a = (e1 * h).sum(1)
    s = o64 - vv[:, 0]
    bu = (s * h).sum(1) / a
    bv = (d64 * np.cross(s, e1)).sum(1) / a
    differs = (np.abs(tu - bu) > 1e-3) & (np.abs(tv - bv) > 1e-3) & (np.abs(tu - bv) > 1e-3) & (np.abs(tv - bu) > 1e-3)
    print(f"{hit.sum()} hits; tu, tv away from both barycentrics: {differs.mean():.4f}; negative sign on {(sc.tangent_sign[tri[hit]] < 0).mean():.3f}")
    assert differs.mean() >= 0.9
    assert 0.3 < (sc.tangent_sign[tri[hit]] < 0).mean() < 0.7


# ---- paths ----

@functools.lru_cache(maxsize=None)
def tiled(kind, lights=False):
    sc = uv_scenes.tiled(kind)
    if lights:
        sc.point_lights = scenes.point_lights(5, seed=3, lo=(-0.8, -0.8, 2.2), hi=(0.8, 0.8, 3.8))
        sc._desc = None
    return sc


@functools.lru_cache(maxsize=None)
def oracle_frame(kind, flags=0):
    """the oracle's render of the frame, once per scene (not changed by the tests that share it)"""
    import oracle as orc
    sc = tiled(kind, bool(flags))
    o = orc.Oracle(sc, math_mode=orc.MATH_ER, max_bounces=BOUNCES, threads=8, flags=flags)
    o.render(SPP)
    out = {name: o.read_pass(p) for name, p in abi.PASS_NAMES.items()}
    out["samples"], out["rng"], out["counters"] = o.read_samples(), o.read_rng(), o.counters()
    o.close()
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_the_plan_on_the_device_is_what_the_scene_is_about(kind):
    """modes, fused widths and filters as tests/test_uv_scenes_cpu.py asserts them of the plan, read back from the begun scene -- and
    tex_pow2, which decides the branch of wrap_abs: 1 only where every side is a power of two"""
    sc = tiled(kind)
    rm = render.RenderingManager(render.RenderParameters(max_bounces=BOUNCES))
    rm.start_rendering(sc)
    try:
        dump = rm.debug_read_textures()
    finally:
        rm.close()
    plan = abi.debug_texture_plan(sc)
    uv_scenes.assert_plan(kind, plan)
    assert dump["tex_pow2"] == uv_scenes.KINDS[kind]["tex_pow2"] and dump["fused_any"] == 1
    assert dump["table"].tobytes() == plan["table"].tobytes() and dump["fused"].tobytes() == plan["fused"].tobytes()


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("kind", KINDS)
def test_paths_equal_the_oracles(oracle_mod, kind, schedule):
    sc = tiled(kind)
    o = oracle_frame(kind)
    g = gpu_render(sc, SPP, max_bounces=BOUNCES, flags=SCHEDULES[schedule])
    compare(g, o, what=f"{kind} / {schedule}")
    print({k: (g["counters"][k], o["counters"][k]) for k in ("paths", "bounce_samples", "shaded_hits", "hdri_samples")})
    assert g["counters"]["paths"] == o["counters"]["paths"] == sc.x_res * sc.y_res * SPP
    assert g["counters"]["bounce_samples"] == o["counters"]["bounce_samples"]
    assert g["counters"]["shaded_hits"] == o["counters"]["shaded_hits"] > 0
    assert g["counters"]["hdri_samples"] == o["counters"]["hdri_samples"] > 0


@pytest.mark.parametrize("kind", KINDS)
def test_schedules_count_the_same_events(kind):
    """the three schedules against each other, every bit and every counter; with ER_FLAG_COUNTERS the texel fetches too (wavefront and
    streaming, as tests/test_gpu_parity.py compares them).  Node visits and triangle tests are not held against each other here: on
    smooth normals -- a soup with these jittered normals and the default material is enough, whatever its uvs -- the two schedules
    count the resolution of lifted candidates differently (1.4 % apart on this frame, every plane and every other counter equal)."""
    sc = tiled(kind)
    for count in (0, abi.FLAG_COUNTERS):
        w = run_counted(sc, [SPP], abi.FLAG_WAVEFRONT | count, max_bounces=BOUNCES)
        s = run_counted(sc, [2, SPP - 2], abi.FLAG_STREAM | count, max_bounces=BOUNCES)
        assert_no_bit_differs(s, w, (kind, "stream", count))
        if count:
            print({k: (s["counters"][k], w["counters"][k]) for k in ("texel_fetches", "shaded_hits")}, "form", s["stream"]["form"])
            assert s["counters"]["texel_fetches"] == w["counters"]["texel_fetches"] > w["counters"]["shaded_hits"]
        else:
            m = run_counted(sc, [SPP], abi.FLAG_MEGAKERNEL, max_bounces=BOUNCES)
            assert_no_bit_differs(m, w, (kind, "megakernel"))


@pytest.mark.parametrize("knob", ["ER_TEX_COMPACT", "ER_TEX_FUSE", "ER_TEX_POW2"])
@pytest.mark.parametrize("kind", KINDS)
def test_plan_knobs_do_not_change_a_bit(kind, knob, monkeypatch):
    """every texture as it came (no compaction, no fused records), no fused records alone, and the wrap by division where the mask
    is the default: the same image"""
    sc = tiled(kind)
    ref = gpu_render(sc, SPP, max_bounces=BOUNCES, flags=abi.FLAG_STREAM)
    monkeypatch.setenv(knob, "0")
    rm = render.RenderingManager(render.RenderParameters(max_bounces=BOUNCES, flags=abi.FLAG_STREAM))
    rm.start_rendering(sc)
    try:
        dump = rm.debug_read_textures()
        rm.render(SPP)
        other = {p: rm.get_pass(p) for p in ("beauty", "normal", "tangent", "bitangent")}
        other["rng"], other["samples"], other["counters"] = rm.read_rng(), rm.read_samples(), rm.counters()
    finally:
        rm.close()
    monkeypatch.delenv(knob)
    if knob == "ER_TEX_POW2":
        assert dump["tex_pow2"] == 0 and dump["fused_any"] == 1
    else:      # the knob took effect
        assert dump["fused_any"] == 0 and dump["tex_pow2"] == uv_scenes.KINDS[kind]["tex_pow2"]
        assert (dump["table"]["channels"] == [t[3] for t in sc.textures]).all() == (knob == "ER_TEX_COMPACT")
    for p in ("beauty", "normal", "tangent", "bitangent"):
        assert (ref[p].view(np.uint32) == other[p].view(np.uint32)).all(), (knob, p)
    assert (ref["rng"] == other["rng"]).all() and (ref["samples"] == other["samples"]).all()
    for k in COUNTS:
        assert ref["counters"][k] == other["counters"][k], (knob, k)


def test_per_bounce_records_of_forty_pixels(oracle_mod):
    """er_debug_trace_pixel against oracle_trace_pixel on tiled-pow2, as tests/test_gpu_function_level.py::
    test_per_bounce_trace_of_pixel_samples: which bounce, which field"""
    sc = tiled("tiled-pow2")
    orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, max_bounces=BOUNCES, threads=1)
    rm = render.RenderingManager(render.RenderParameters(max_bounces=BOUNCES))
    rm.start_rendering(sc)
    try:
        rm.render(2)
        orc.render(2)
        pixels = np.random.default_rng(5).choice(sc.x_res * sc.y_res, 40, replace=False)
        n_rec = n_bad = n_shadow = n_hit = 0
        for idx in pixels:
            for rep in range(2):
                g = rm.debug_trace_pixel(int(idx), max_recs=32)
                o = orc.trace_pixel(int(idx), max_recs=32)
                assert len(g) == len(o), (idx, len(g), len(o))
                for a, b in zip(g, o):
                    n_rec += 1
                    n_hit += int(a.tri >= 0)
                    traced = a.shadow_occ >= 0      # (the kernels skip the HDRI shadow ray where the BRDF term is exactly zero)
                    n_shadow += int(traced)
                    if _rec_tuple(a, traced) != _rec_tuple(b, traced):
                        n_bad += 1
                        if n_bad <= 3:
                            print("pixel", idx, "bounce", a.bounce, _rec_tuple(a, traced), "!=", _rec_tuple(b, traced))
        print(f"{n_rec} bounce records ({n_hit} hits, {n_shadow} with a traced shadow query), {n_bad} differ")
        assert n_hit > 40 and n_shadow > 0.05 * n_rec
        assert n_bad == 0
        img, ref = rm.get_pass("beauty"), orc.read_pass(0)
        assert (img.view(np.uint32) == ref.view(np.uint32)).all(-1).mean() >= 0.999
    finally:
        rm.close()
        orc.close()


def test_paths_with_point_lights_and_mis(oracle_mod):
    sc = tiled("tiled-any", True)
    o = oracle_frame("tiled-any", LIGHTS)
    g = gpu_render(sc, SPP, max_bounces=BOUNCES, flags=LIGHTS)
    compare(g, o, what="tiled-any with point lights and MIS")
    assert g["counters"]["bounce_samples"] == o["counters"]["bounce_samples"]
    plain = oracle_frame("tiled-any")
    assert (plain["beauty"].view(np.uint32) != o["beauty"].view(np.uint32)).any()      # the lights do something


# ---- mesh lights ----

def emitter_scene(x_res=40, y_res=32):
    """test_gpu_mesh_lights.py's textured scene (the light under a 4 x 4 bilinear emission map) with the light's two triangles mapped
    over several periods, one of them mirrored, and the constant emitter and a wall under negative coordinates"""
    sc = textured_scene(x_res, y_res)
    sc.uvs[10] = [[-1.5, -2.25], [2.5, -2.0], [-1.25, 1.75]]
    sc.uvs[11] = [[3.0, 2.5], [2.75, -1.0], [-0.5, 2.25]]           # the other orientation: mirrored
    sc.uvs[12] = [[-0.3, -0.2], [-2.0, 0.1], [0.4, -1.7]]
    sc.tangent_sign[10:13] = [-1.0, 1.0, -1.0]
    sc._desc = None
    e = sc.uvs[10:12]
    d = (e[:, 1, 0] - e[:, 0, 0]) * (e[:, 2, 1] - e[:, 0, 1]) - (e[:, 1, 1] - e[:, 0, 1]) * (e[:, 2, 0] - e[:, 0, 0])
    assert d[0] * d[1] < 0 and np.ptp(e[..., 0]) > 2
    return sc


def test_mesh_lights_with_varied_emitter_uvs(oracle_mod):
    """The oracle does not mirror ER_FLAG_MESH_LIGHTS (tests/test_gpu_mesh_lights.py), so: the emitter table against numpy; the three
    schedules against each other with the flag, with and without MIS (the emission "at p's interpolated uv", csrc/er_shade.h, through
    er_bounce.inc and the streaming kernel's own copy); and WITHOUT the flag -- where a path that reaches the light fetches the same
    bilinear emission map at the same varied coordinates -- against the oracle."""
    sc = emitter_scene()
    ids, _ = numpy_table(sc)
    for mis in (0, abi.FLAG_MIS):
        outs = [run_lights(sc, 6, flags=MESH | mis | s) for s in (abi.FLAG_STREAM, abi.FLAG_WAVEFRONT, abi.FLAG_MEGAKERNEL)]
        assert outs[0]["lights"]["emitters"] == len(ids) == 3
        for o, s in zip(outs[1:], ("wavefront", "megakernel")):
            same_lights(outs[0], o, f"{s} against streaming, mis {mis}")
    unit = textured_scene(40, 32)
    assert not (run_lights(unit, 6, flags=MESH)["beauty"].view(np.uint32) == outs[0]["beauty"].view(np.uint32)).all()      # the uvs count
    g = gpu_render(sc, 6, max_bounces=5)
    o = oracle_render(oracle_mod, sc, 6, max_bounces=5)
    compare(g, o, what="textured emitter, varied uvs, no NEE")
    assert g["counters"]["bounce_samples"] == o["counters"]["bounce_samples"]


# ---- edits keep each triangle's uvs and sign ----

W, H = 64, 48


@functools.lru_cache(maxsize=None)
def varied_torture(n=6000, seed=6, uv_seed=23):
    """a varied 6 000-triangle textured scene (never edited in place: the edits below go through copies)"""
    return uv_scenes.varied(scenes.torture(n, W, H, seed=seed, n_materials=8, tex_size=16, hdri_size=(32, 16), n_lights=0), uv_seed)


def records_by_triangle(dump, n):
    """(uv [n][3][2], sign [n]) of a structure dump, by triangle id"""
    ids = dump["isect"]["tri_id"][:n]
    uv, sign = np.zeros((n, 3, 2), np.float32), np.zeros(n, np.float32)
    uv[ids], sign[ids] = dump["attr"]["uv"][:n], dump["isect"]["sign"][:n]
    return uv, sign


def assert_records_are_the_scenes(rm, sc, what):
    """accel_check's r_attr and r_sign in particular, stated once more in two lines"""
    d = rm.debug_read_accel()
    rep = accel_check.check(sc, d, accel_depth=rm.accel_info()["max_depth"])
    assert rep.ok, (what, rep.message())
    uv, sign = records_by_triangle(d, sc.tri_count)
    assert uv.tobytes() == sc.uvs.tobytes() and sign.tobytes() == sc.tangent_sign.tobytes(), what


@pytest.mark.parametrize("builder", ["default", "device"])
def test_remove_and_append_keep_every_triangles_own_uvs(builder):
    """tests/test_gpu_topology.py::test_edits_equal_fresh_scenes' remove-and-append on 6 000 varied triangles: removed ids spread over the
    range, appended triangles with uvs and signs of their own; through the host builder (path 0) and, twice, through the device builder:
    the first edit fills the geometry store (path 2), the second compacts and gathers on the device (path 1: k_topo_gather over the uvs)."""
    flags = abi.FLAG_GPU_BUILD if builder == "device" else 0
    sc = varied_torture()
    other = varied_torture(400, 5, 31)
    rm = manager(sc, flags)
    try:
        rm.render(2)
        steps = [dict(remove=np.arange(7, sc.tri_count, 37), append=tail_of(other, 150, 100)),
                 dict(remove=np.concatenate([np.arange(3, 5900, 101), np.arange(5950, 5988)]), append=tail_of(other, 61, 300))]
        for k, kw in enumerate(steps):
            sc = topology_edit(rm, sc, f"{builder}: edit {k}", flags, **kw)
            assert rm.topology_info()["path"] == (0 if builder == "default" else 2 if k == 0 else 1)
            assert_records_are_the_scenes(rm, sc, f"{builder}: edit {k}")
            tail = kw["append"]
            assert sc.uvs[-len(tail["uvs"]):].tobytes() == tail["uvs"].tobytes() and (sc.uvs[-1] != uv_scenes.UNIT).any()
    finally:
        rm.close()


def spread_ids(sc, k=40, seed=3):
    """k triangle ids spread over the range, none of which holds the scene's largest |coordinate|"""
    a = np.abs(tris(sc)).reshape(sc.tri_count, -1).max(1)
    ids = np.random.default_rng(seed).permutation(sc.tri_count)
    return ids[a[ids] < a.max()][:k]


def assert_outputs_equal_a_fresh_scenes(A, sc_new, what):
    fresh = manager(sc_new)
    try:
        assert_same_outputs(outputs(A), outputs(fresh), what + ": right after")
        for rm in (A, fresh):
            rm.render(3)
        assert_same_outputs(outputs(A), outputs(fresh), what + ": 3 spp later")
        assert A.counters() == fresh.counters(), what
    finally:
        fresh.close()


def test_a_sparse_update_leaves_uvs_and_signs_alone():
    sc = varied_torture()
    ids = spread_ids(sc)
    new = (tris(sc)[ids] * np.float32(0.97) + np.array([0.0, 0.0, 0.09], np.float32)).astype(np.float32)      # towards the scene's middle
    A, B = sparse_pair(sc)
    try:
        for rm in (A, B):
            rm.render(2)
        sc_new = sparse_both(A, B, sc, ids, new)
        assert A.sparse_info()["path"] in (1, 2) and A.sparse_info()["why_full"] == 0 and A.sparse_info()["moved"] == len(ids)
        assert_same_as_twin_structure(A, B, sc_new, "sparse")
        assert_records_are_the_scenes(A, sc_new, "sparse")
        assert_outputs_equal_a_fresh_scenes(A, sc_new, "sparse")
    finally:
        A.close()
        B.close()


def test_an_object_transform_leaves_uvs_and_signs_alone():
    sc = varied_torture()
    objects = soup_objects(sc, sizes=(65, 200), avoid_maximum=True)
    poses = {1: matrix(rotation((2, -1, 0.5), 0.9) @ np.diag([0.8, 0.6, 0.9]), about=centre_of(sc, objects[1])), 0: matrix(np.eye(3) * 0.9)}
    A, B, rp = transform_pair(sc, objects)
    try:
        for rm in (A, B):
            rm.render(2)
        sc_new = transform_both(A, B, rp, poses)
        assert A.transform_info()["moved"] == 265
        assert_same_as_twin_structure(A, B, sc_new, "transform")
        assert_records_are_the_scenes(A, sc_new, "transform")
        assert_outputs_equal_a_fresh_scenes(A, sc_new, "transform")
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("builder", ["host", "device"])
def test_a_rebuilding_update_packs_every_triangles_own_uvs(builder):
    """REBUILD_ALWAYS through either builder (k_records on the device): the four buffers of a fresh create + begin of the edited scene"""
    flags = abi.FLAG_GPU_BUILD if builder == "device" else abi.FLAG_HOST_BUILD
    sc = varied_torture()
    arrays = edit_J(sc)
    sc_new = with_arrays(sc, **arrays)
    rm, fresh = manager(sc, flags), manager(sc_new, flags)
    try:
        assert rm.accel_info()["builder"] == (1 if builder == "device" else 0)
        rm.set_update_policy(abi.REBUILD_ALWAYS)
        rm.update(**arrays)
        assert rm.rebuild_info()["rebuilds"] == 1
        assert_same_as_fresh_structure(rm, fresh, sc_new, f"always / {builder}")
        assert_records_are_the_scenes(rm, sc_new, f"always / {builder}")
        for m in (rm, fresh):
            m.render(3)
        assert_same_outputs(outputs(rm), outputs(fresh), f"always / {builder}: 3 spp later")
    finally:
        rm.close()
        fresh.close()
