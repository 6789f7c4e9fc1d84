"""er_render_update and er_render_edit are one function (csrc/er_api_edit.cpp): the same camera / geometry edit sent through either
entry point leaves twin scenes byte-equal -- planes, structure, texture stage, info structs -- under every rebuild policy and both
builders; which info struct a call's wall time goes to; whose name a refusal carries; and that a refused call has touched nothing of
the host copy, which the arrays of fixed size are now copied into in place.

Scenes: soup-6000 (host builder) and soup-20001 (device builder), the smallest pair on either side of ER_GPU_BUILD_MIN_TRIS, at
tests/test_gpu_update.py's frame.  Geometry: S5 of tests/test_gpu_rebuild.py (5 % of the triangles scattered), whose refitted tree
that file's control finds at >= 3 x the built tree's cost on both scenes.  So under ER_REBUILD_AUTO the ratio 2.0 (that file's)
rebuilds, and the largest finite float keeps the refit -- no finite cost exceeds it times a positive one; the test asserts either
decision."""
import ctypes as C

import numpy as np
import pytest

from elevenrender_amd import abi
from test_accel_cost_cpu import edit_S5
from test_gpu_accel_structure import raw_buffers, scene
from test_gpu_edit import TP, assert_same_dump, changed, edit_args
from test_gpu_update import assert_same_outputs, edit_J, manager, moved_camera, outputs

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
POLICIES = {"never": (abi.REBUILD_NEVER, 0.0, 0), "always": (abi.REBUILD_ALWAYS, 0.0, 3),      # mode, ratio, last_decision of a geometry edit
            "auto-keeps": (abi.REBUILD_AUTO, FLT_MAX, 1), "auto-rebuilds": (abi.REBUILD_AUTO, 2.0, 2)}
MS_FIELDS = ("build_ms", "upload_ms", "refit_ms", "update_ms", "cost_ms", "rebuild_ms")


def edit_of(sc, kind):
    out = {}
    if "camera" in kind:
        out["camera"] = moved_camera(sc)
    if "geometry" in kind:
        out.update(edit_S5(sc))
    if "normals" in kind:      # J's turned normals; the tangents of each triangle's vertices in another order
        out["normals"] = edit_J(sc)["normals"]
        out["tangents"] = np.ascontiguousarray(np.roll(sc.tangents.reshape(-1, 3, 3), 1, axis=1))
    return out


def without_ms(info):
    return {k: v for k, v in info.items() if k not in MS_FIELDS}


def everything(rm):
    return dict(outputs=outputs(rm), accel=raw_buffers(rm.debug_read_accel()), textures=rm.debug_read_textures(), accel_info=without_ms(rm.accel_info()),
                update_info=without_ms(rm.update_info()), rebuild_info=without_ms(rm.rebuild_info()), edits=rm.edit_info()["edits"])


def assert_twins(a, b, what):
    assert_same_outputs(a["outputs"], b["outputs"], what)
    for k in a["accel"]:
        assert a["accel"][k] == b["accel"][k], f"{what}: structure buffer {k} differs"
    assert_same_dump(a["textures"], b["textures"], what)
    for k in ("accel_info", "update_info", "rebuild_info"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert a["edits"] == 0 and b["edits"] == 0, what


@pytest.mark.parametrize("policy", list(POLICIES))
@pytest.mark.parametrize("kind", ["camera", "geometry", "camera+geometry", "geometry+normals+tangents"])
@pytest.mark.parametrize("case", ["soup-6000", "soup-20001"])
def test_the_same_edit_through_either_entry_point(case, kind, policy):
    sc = scene(case)
    args = edit_of(sc, kind)
    mode, ratio, decision = POLICIES[policy]
    a, b = manager(sc), manager(sc)
    try:
        for rm in (a, b):
            rm.set_update_policy(mode, ratio)
            rm.render(2)
        a.update(**args)
        b.edit(**args)
        for rm in (a, b):
            rm.render(2)
        ea, eb = everything(a), everything(b)
        r, u = ea["rebuild_info"], ea["update_info"]
        print(f"{case} / {kind} / {policy}: builder {ea['accel_info']['builder']}, decision {r['last_decision']}, cost built {r['cost_built']:.6g} refit {r['cost_refit']:.6g}, {u}")
        assert_twins(ea, eb, f"{case} / {kind} / {policy}")
        geometry = "geometry" in kind
        assert r["last_decision"] == (decision if geometry else 0)
        assert u["updates"] == 1 and u["refits"] == (1 if geometry and decision in (0, 1) else 0)
        assert ea["accel_info"]["builder"] == (2 if u["refits"] else (0 if case == "soup-6000" else 1))
    finally:
        a.close()
        b.close()


def test_which_info_struct_takes_the_wall_time():
    sc = TP()
    new = changed(sc, materials={0: dict(albedo=(0.2, 0.7, 0.4), roughness=0.35)})
    rm = manager(sc)
    try:
        rm.edit(**edit_args(sc, new))                   # materials alone: an edit
        u, e = rm.update_info(), rm.edit_info()
        assert u["update_ms"] == 0.0 and u["updates"] == 1 and e["edits"] == 1 and e["edit_ms"] > 0
        rm.edit(camera=moved_camera(sc))                # the camera alone through er_render_edit: an update
        u, e2 = rm.update_info(), rm.edit_info()
        assert u["update_ms"] > 0 and u["updates"] == 2 and e2 == e
    finally:
        rm.close()


def test_refusals_carry_the_name_of_the_entry_point():
    sc = scene("soup-6000")
    v = sc.vertices.copy()
    v.reshape(-1)[4321] = np.nan
    rm = manager(sc)
    try:
        for call, name in ((rm.update, "er_render_update"), (rm.edit, "er_render_edit")):
            with pytest.raises(abi.ErError) as err:
                call(vertices=v)
            msg = rm.lib.er_last_error().decode()
            assert err.value.code == abi.ER_ERR_INVALID_ARG and msg.startswith(name) and "finite" in msg, msg
        u = abi.ErSceneUpdate()
        u.what = abi.EDIT_MATERIALS                     # a bit er_render_edit knows and er_render_update does not
        assert rm.lib.er_render_update(rm.handle, C.byref(u)) == abi.ER_ERR_INVALID_ARG
        assert rm.lib.er_last_error().decode().startswith("er_render_update")
        assert rm.update_info()["updates"] == 0 and rm.edit_info()["edits"] == 0
    finally:
        rm.close()


def begin_again(rm):
    p = abi.ErRenderParams(rm.pars.sampleTarget, rm.pars.block_size, rm.pars.max_bounces, 0, rm.pars.rank, rm.pars.world, rm.pars.flags)
    abi.check(rm.lib.er_render_begin(rm.handle, C.byref(p)))


@pytest.mark.parametrize("case", ["soup-6000", "soup-20001"])
def test_a_refused_call_has_not_touched_the_host_copy(case):
    """geometry + materials, the vertices moved, the material list refused (material_count 0): er_render_begin again on the handle
    builds from the host copy -- which must still be the scene's own"""
    sc = scene(case)
    moved = edit_S5(sc)["vertices"]
    assert (moved != sc.vertices.reshape(moved.shape)).any()
    rm, twin = manager(sc), manager(sc)
    try:
        e = abi.ErSceneEdit()
        e.what = abi.EDIT_GEOMETRY | abi.EDIT_MATERIALS
        e.vertices = abi._fptr(moved)
        mats = (abi.ErMaterial * len(sc.materials))(*sc.materials)
        e.material_count, e.materials = 0, mats
        assert rm.lib.er_render_edit(rm.handle, C.byref(e)) == abi.ER_ERR_INVALID_ARG
        begin_again(rm)
        rm.render(2)
        twin.render(2)
        assert_same_outputs(outputs(rm), outputs(twin), case)
        got, want = raw_buffers(rm.debug_read_accel()), raw_buffers(twin.debug_read_accel())
        for k in got:
            assert got[k] == want[k], k
        assert rm.update_info()["updates"] == 0 and rm.edit_info()["edits"] == 0
    finally:
        rm.close()
        twin.close()
