"""er_render_update on the GPU: a begun scene edited in place -- a new camera, moved triangles by a device refit of the built structure
(csrc/er_refit.hip) -- against the contract of include/eleven_hip.h: every readable output equals a fresh er_scene_create +
er_render_begin of the edited description, bit for bit; the structure keeps its topology and checks clean under tests/accel_check.py.

The edits (seeded, float32):  T  every vertex + (40, -3, 7): the largest coordinate, the absolute padding and the node exponents change;
J  every vertex jittered by N(0, 0.3 x 2 / cbrt(n)) and every triangle's normals turned by a small seeded rotation: the lift changes;
M  (blobs) one instance moved across the grid into another: an object move, overlapping subtrees;  I  the unchanged arrays."""
import copy
import ctypes as C
import time

import numpy as np
import pytest

import accel_check
from elevenrender_amd import abi, client, render, scenes
from test_gpu_accel_structure import BARY, aimed_rays, oracle_hits, raw_buffers, scene

pytestmark = pytest.mark.gpu

PLANES = ("beauty", "denoise", "normal", "tangent", "bitangent")
SCHEDULES = {"stream": abi.FLAG_STREAM, "wavefront": abi.FLAG_WAVEFRONT, "megakernel": abi.FLAG_MEGAKERNEL}
BLOB_INSTANCES = 30          # test_gpu_accel_structure.scene("blobs")


def with_arrays(sc, vertices=None, normals=None, tangents=None, camera=None):
    """a copy of the scene description with those arrays or that camera replaced: what a fresh er_scene_create would be given"""
    out = copy.copy(sc)
    out._desc = None
    if vertices is not None:
        out.vertices = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(sc.vertices.shape))
    if normals is not None:
        out.normals = np.ascontiguousarray(np.asarray(normals, np.float32).reshape(sc.normals.shape))
    if tangents is not None:
        out.tangents = np.ascontiguousarray(np.asarray(tangents, np.float32).reshape(sc.tangents.shape))
    if camera is not None:
        out.camera = camera
    return out


def edit_T(sc):
    return dict(vertices=(sc.vertices.reshape(-1, 3, 3) + np.array([40.0, -3.0, 7.0], np.float32)).astype(np.float32))


def edit_J(sc, seed=7):
    rng = np.random.default_rng(seed)
    v = sc.vertices.reshape(-1, 3, 3)
    n = len(v)
    vj = (v + rng.normal(0.0, 0.3 * 2.0 / np.cbrt(n), size=v.shape)).astype(np.float32)
    # one small rotation per triangle, applied to its three normals (first order in the angle, the length restored)
    w = rng.normal(0.0, 0.05, size=(n, 1, 3))
    nn = sc.normals.reshape(-1, 3, 3).astype(np.float64)
    turned = nn + np.cross(np.broadcast_to(w, nn.shape), nn)
    turned *= np.linalg.norm(nn, axis=-1, keepdims=True) / np.maximum(np.linalg.norm(turned, axis=-1, keepdims=True), 1e-30)
    return dict(vertices=vj, normals=turned.astype(np.float32))


def edit_M(sc):
    """blobs: instance 0 translated onto the far corner instance of the grid"""
    v = sc.vertices.reshape(-1, 3, 3).copy()
    per = len(v) // BLOB_INSTANCES
    delta = v[(BLOB_INSTANCES - 1) * per:].reshape(-1, 3).mean(0) - v[:per].reshape(-1, 3).mean(0)
    v[:per] += delta.astype(np.float32)
    return dict(vertices=v)


def edit_I(sc):
    return dict(vertices=sc.vertices.copy(), normals=sc.normals.copy(), tangents=sc.tangents.copy())


EDITS = {"T": edit_T, "J": edit_J, "M": edit_M, "I": edit_I}


def moved_camera(sc):
    cam = abi.ErCamera.from_buffer_copy(sc.camera)
    cam.position = abi.ErVec3(sc.camera.position.x + 0.21, sc.camera.position.y - 0.13, sc.camera.position.z - 0.4)
    cam.rotation = abi.ErVec3(3.0, -7.0, 1.5)
    return cam


def manager(sc, flags=0, rank=0, world=1):
    rm = render.RenderingManager(render.RenderParameters(max_bounces=4, flags=flags, rank=rank, world=world))
    rm.start_rendering(sc)
    return rm


def outputs(rm):
    out = {p: rm.get_pass(p).view(np.uint32) for p in PLANES}
    out["samples"], out["rng"] = rm.read_samples(), rm.read_rng()
    out["state"] = rm.state_export()
    return out


def assert_same_outputs(a, b, what):
    for k in a:
        diff = int((a[k] != b[k]).sum())
        assert diff == 0, f"{what}: {k} differs in {diff} words"


# ---- structure ----

STRUCTURE_CASES = ["soup-3", "soup-257", "soup-6000", "soup-20001", "torture", "blobs", "same-centroid", "duplicates", "flat-grid"]
TOPOLOGY8 = ("imask", "child_base", "tri_base", "tri_present", "reserved")


def lift_by_triangle(dump, n):
    out = np.zeros(n, np.float32)
    out[dump["isect"]["tri_id"][:n]] = dump["isect"]["lift"][:n]
    return out


def check_refitted(sc_new, before, after, info, fresh_dump):
    n = sc_new.tri_count
    rep = accel_check.check(sc_new, after, accel_depth=info["max_depth"])
    assert rep.ok, rep.message()
    for f in TOPOLOGY8:
        assert before["nodes8"][f].tobytes() == after["nodes8"][f].tobytes(), f
    for f in ("c0", "c1"):
        assert before["nodes"][f].tobytes() == after["nodes"][f].tobytes(), f
    for f in ("tri_id", "sign"):
        assert before["isect"][f].tobytes() == after["isect"][f].tobytes(), f
    for f in ("uv", "material", "pad"):
        assert before["attr"][f].tobytes() == after["attr"][f].tobytes(), f
    assert info["builder"] == 2 and after["builder"] == 2
    assert after["lo"].tobytes() == fresh_dump["lo"].tobytes() and after["hi"].tobytes() == fresh_dump["hi"].tobytes(), (after["lo"], fresh_dump["lo"], after["hi"], fresh_dump["hi"])
    assert after["lift_bound"].tobytes() == fresh_dump["lift_bound"].tobytes() and after["max_lift"].tobytes() == fresh_dump["max_lift"].tobytes()
    assert np.float32(info["lift_bound"]) == after["lift_bound"]
    assert lift_by_triangle(after, n).tobytes() == lift_by_triangle(fresh_dump, n).tobytes()


@pytest.mark.parametrize("case,edit", [(c, e) for c in STRUCTURE_CASES for e in ("J", "T")] + [("blobs", "M")])
def test_refitted_structure_checks_clean_and_keeps_its_topology(case, edit):
    sc = scene(case)
    arrays = EDITS[edit](sc)
    sc_new = with_arrays(sc, **arrays)
    rm = manager(sc)
    before, info0 = rm.debug_read_accel(), rm.accel_info()
    rm.update(**arrays)
    after, info, upd = rm.debug_read_accel(), rm.accel_info(), rm.update_info()
    rm.close()
    fresh = manager(sc_new)
    fresh_dump = fresh.debug_read_accel()
    fresh.close()
    print(f"{case} / {edit}: builder {info0['builder']} built {before['node8_count']} wide nodes; refit {upd['refit_ms']:.3f} ms, update {upd['update_ms']:.3f} ms")
    assert upd["updates"] == 1 and upd["refits"] == 1 and info["build_ms"] == upd["refit_ms"]
    for f in ("node_count", "node_bytes", "leaf_count", "max_depth", "tri_record_bytes"):
        assert info[f] == info0[f], f
    check_refitted(sc_new, before, after, info, fresh_dump)


@pytest.mark.parametrize("case", ["soup-6000", "soup-20001"])
def test_refit_of_the_unchanged_arrays(case):
    sc = scene(case)
    rm = manager(sc)
    before = rm.debug_read_accel()
    rm.update(**edit_I(sc))
    after, info = rm.debug_read_accel(), rm.accel_info()
    rm.close()
    assert before["isect"].tobytes() == after["isect"].tobytes() and before["attr"].tobytes() == after["attr"].tobytes()
    rep = accel_check.check(sc, after, accel_depth=info["max_depth"])
    assert rep.ok, rep.message()
    same8 = (before["nodes8"].view(np.uint8).reshape(len(before["nodes8"]), -1) == after["nodes8"].view(np.uint8).reshape(len(after["nodes8"]), -1)).all(1).mean()
    same2 = (before["nodes"].view(np.uint8).reshape(len(before["nodes"]), -1) == after["nodes"].view(np.uint8).reshape(len(after["nodes"]), -1)).all(1).mean()
    print(f"{case}: byte-equal after a refit of the unchanged arrays: wide nodes {same8:.4f}, binary nodes {same2:.4f}")


def test_a_stale_structure_fails_the_checker():
    """negative control, the checker alone: the dump of the scene as built, judged against the J-edited scene"""
    sc = scene("soup-6000")
    rm = manager(sc)
    before = rm.debug_read_accel()
    rm.close()
    rep = accel_check.check(with_arrays(sc, **edit_J(sc)), before)
    assert rep.counts["w_box"] > 0 and rep.counts["r_vertices"] > 0, rep.message()


@pytest.mark.parametrize("case", ["soup-6000", "soup-20001"])
def test_two_updates_in_a_row(case):
    sc = scene(case)
    rm = manager(sc)
    before = rm.debug_read_accel()
    first = edit_J(sc)
    rm.update(**first)
    sc1 = with_arrays(sc, **first)
    second = edit_J(sc1, seed=8)
    rm.update(**second)
    sc2 = with_arrays(sc1, **second)
    after, info, upd = rm.debug_read_accel(), rm.accel_info(), rm.update_info()
    rm.close()
    fresh = manager(sc2)
    fresh_dump = fresh.debug_read_accel()
    fresh.close()
    assert upd["updates"] == 2 and upd["refits"] == 2
    check_refitted(sc2, before, after, info, fresh_dump)


# ---- rays ----

@pytest.mark.parametrize("case,edit", [("soup-6000", "J"), ("blobs", "M")])
def test_rays_through_a_refitted_structure(oracle_mod, case, edit):
    sc = scene(case)
    arrays = EDITS[edit](sc)
    sc_new = with_arrays(sc, **arrays)
    bary = BARY if case == "soup-6000" else BARY[:1]
    o, d, own, h = aimed_rays(sc_new, bary)
    limit = np.full(len(o), 2 * h, np.float32)
    got = {}
    for which in ("updated", "fresh"):
        rm = manager(sc if which == "updated" else sc_new)
        if which == "updated":
            rm.update(**arrays)
        tri, slot, pos, dist, _ = rm.debug_trace_rays(o, d)
        etri, epos, edist = rm.debug_closest_hit(o, d)
        occ, _ = rm.debug_trace_rays(o, d, self_slots=np.where(tri >= 0, slot, -1).astype(np.int32), limits=limit)      # first hit exempt, limit 2 h
        rm.close()
        got[which] = dict(tri=tri, pos=pos.view(np.uint32), dist=dist.view(np.uint32), etri=etri, epos=epos.view(np.uint32), edist=edist.view(np.uint32), occ=occ)
    for k in got["fresh"]:
        diff = int((got["updated"][k] != got["fresh"][k]).sum())
        print(f"{case} / {edit}: {k}: {diff} of {len(o)} rays differ between the refitted and the fresh structure")
        assert diff == 0, k
    if case == "soup-6000":
        orc = oracle_mod.Oracle(sc_new, math_mode=oracle_mod.MATH_ER, max_bounces=4, threads=16)
        otri, opos = oracle_hits(orc, o, d)
        orc.close()
        own_share = float((otri == own).mean())
        print(f"   oracle: own-triangle share {own_share:.4f}")
        assert own_share >= 0.98
        u = got["updated"]
        for what, t, p in (("production traversal", u["tri"], u["pos"]), ("exact routine", u["etri"], u["epos"])):
            bad = (t != otri) | (p != opos.view(np.uint32)).any(-1)
            assert not bad.any(), (what, int(bad.sum()))


# ---- images ----

def image_scene(name):
    return scene("soup-6000") if name == "soup-6000" else scenes.cornell(48, 48)


def update_args(sc, kind):
    out = {}
    if "camera" in kind:
        out["camera"] = moved_camera(sc)
    if "J" in kind:
        out.update(edit_J(sc))
    return out


def updated_and_fresh(sc, args, flags=0, rank=0, world=1, before=None):
    """(outputs, counters, manager) of: 4 spp, the update, 4 spp -- and of a fresh create + begin + 4 spp of the edited description"""
    rm = manager(sc, flags, rank, world)
    if before:
        before(rm)
    rm.render(4)
    rm.update(**args)
    fresh = manager(with_arrays(sc, **args), flags, rank, world)
    assert rm.get_render_info().samples == fresh.get_render_info().samples
    assert rm.adaptive_info() == fresh.adaptive_info()
    assert_same_outputs(outputs(rm), outputs(fresh), "right after the update")
    rm.render(4)
    fresh.render(4)
    return rm, fresh


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("kind", ["camera", "J", "camera+J"])
@pytest.mark.parametrize("name", ["soup-6000", "cornell"])
def test_render_after_an_update_equals_a_fresh_render(name, kind, schedule):
    sc = image_scene(name)
    rm, fresh = updated_and_fresh(sc, update_args(sc, kind), SCHEDULES[schedule])
    try:
        assert_same_outputs(outputs(rm), outputs(fresh), f"{name} / {kind} / {schedule}")
        assert rm.counters() == fresh.counters()
        assert rm.get_render_info().samples == fresh.get_render_info().samples == 5
        assert rm.light_info() == fresh.light_info() and rm.adaptive_info() == fresh.adaptive_info()
        assert rm.update_info()["refits"] == (1 if "J" in kind else 0)
    finally:
        rm.close()
        fresh.close()


@pytest.mark.parametrize("name", ["soup-6000", "cornell"])
def test_update_on_rank_1_of_3(name):
    sc = image_scene(name)
    rm, fresh = updated_and_fresh(sc, update_args(sc, "camera+J"), 0, rank=1, world=3)
    try:
        assert_same_outputs(outputs(rm), outputs(fresh), name)
        assert rm.counters() == fresh.counters()
    finally:
        rm.close()
        fresh.close()


def test_mesh_lights_follow_a_moved_emitter():
    sc = scenes.cornell(48, 48)
    v = sc.vertices.reshape(-1, 3, 3).copy()
    v[10:12] += np.array([0.3, -0.2, 0.25], np.float32)      # the light: lower and off centre
    args = dict(vertices=v)
    rm, fresh = updated_and_fresh(sc, args, abi.FLAG_MESH_LIGHTS)
    try:
        assert_same_outputs(outputs(rm), outputs(fresh), "mesh lights")
        assert rm.counters() == fresh.counters()
        assert rm.light_info() == fresh.light_info() and rm.light_info()["emitters"] == 2
        (tri_a, cdf_a), (tri_b, cdf_b) = rm.debug_light_table(), fresh.debug_light_table()
        assert tri_a.tolist() == tri_b.tolist() and sorted(tri_a.tolist()) == [10, 11]
        assert cdf_a.tobytes() == cdf_b.tobytes()
    finally:
        rm.close()
        fresh.close()


def test_camera_only_update_leaves_the_structure_alone():
    sc = scene("soup-6000")
    rm = manager(sc)
    rm.render(2)
    info0, buffers0 = rm.accel_info(), raw_buffers(rm.debug_read_accel())
    rm.update(camera=moved_camera(sc))
    info1, buffers1, upd = rm.accel_info(), raw_buffers(rm.debug_read_accel()), rm.update_info()
    rm.close()
    assert info0 == info1
    assert upd["updates"] == 1 and upd["refits"] == 0 and upd["refit_ms"] == 0.0
    for k in buffers0:
        assert buffers0[k] == buffers1[k], k


def test_update_turns_adaptive_sampling_off():
    sc = scenes.cornell(48, 48)
    args = dict(camera=moved_camera(sc))
    rm, fresh = updated_and_fresh(sc, args, before=lambda m: m.set_adaptive(1e-3, 3, 1))
    try:
        assert rm.adaptive_info()["enabled"] == 0
        assert_same_outputs(outputs(rm), outputs(fresh), "after an adaptive render")
    finally:
        rm.close()
        fresh.close()


# ---- errors ----

def test_refused_updates_leave_the_render_as_it_was():
    sc = scene("soup-6000")
    rm, plain = manager(sc), manager(sc)
    try:
        rm.render(2)
        plain.render(2)
        u = abi.ErSceneUpdate()
        assert rm.lib.er_render_update(rm.handle, C.byref(u)) == abi.ER_ERR_INVALID_ARG                 # what = 0
        u.what = 4
        assert rm.lib.er_render_update(rm.handle, C.byref(u)) == abi.ER_ERR_INVALID_ARG                 # an unknown bit
        u.what = abi.UPDATE_GEOMETRY
        assert rm.lib.er_render_update(rm.handle, C.byref(u)) == abi.ER_ERR_INVALID_ARG                 # no vertices
        v = sc.vertices.copy()
        v.reshape(-1)[12345] = np.nan
        with pytest.raises(abi.ErError) as e:
            rm.update(vertices=v)
        assert e.value.code == abi.ER_ERR_INVALID_ARG and "finite" in str(e.value)
        assert rm.update_info()["updates"] == 0
        rm.render(2)
        plain.render(2)
        assert_same_outputs(outputs(rm), outputs(plain), "after refused updates")
    finally:
        rm.close()
        plain.close()


# ---- host ----

def test_host_session_restarts_a_moved_camera_by_update():
    """start, get_pass, load_camera, start, get_pass through eleven_server: the second pass equals that of a session that loaded the
    second camera from the beginning, and the server took the update path (get_info: camera_updates)."""
    from test_host_server import Server

    def wait_for(c, samples):
        deadline = time.time() + 120
        while c.get_info()["samples"] < samples + 1:      # (every poll is a round trip to the server: no sleep between them)
            assert time.time() < deadline, "render did not reach the sample target"

    a = client.cornell_session_assets(48, 48)
    second = dict(position=(0.3, -0.2, -1.9), rotation=(2.0, -5.0, 0.0))
    s = Server()
    c = client.Client(port=s.port)
    first_img = client.play_cornell_session(c, a, sample_target=4)
    assert c.get_info()["camera_updates"] == 0
    c.load_camera(**second)
    c.start()
    wait_for(c, 4)
    moved = c.get_pass("beauty", 48, 48)
    info = c.get_info()
    c.close()
    assert s.finish() == 0
    assert info["camera_updates"] == 1 and info["samples"] == 5
    s = Server()
    c = client.Client(port=s.port)
    ref = client.play_cornell_session(c, dict(a, camera=second), sample_target=4)
    assert c.get_info()["camera_updates"] == 0
    c.close()
    assert s.finish() == 0
    assert (moved.view(np.uint32) == ref.view(np.uint32)).all()
    assert (moved.view(np.uint32) != first_img.view(np.uint32)).any()
