"""er_render_topology on the GPU: after a topology edit of a begun scene every readable output and the structure equal, bit for bit,
er_scene_create + er_render_begin of the edited description (elevenrender_amd/topology.py: apply) -- per schedule and builder, down to
the empty scene and back, through the device-resident geometry store (ErTopologyInfo.path 2, 1, 2 again after another edit), with an
object table, with materials and textures added in the same call, with mesh lights, on one rank of three, after refusals, after a
failed device build, and through the host server."""
import ctypes as C
import time

import numpy as np
import pytest

from elevenrender_amd import abi, client, render, scenes, topology
from test_gpu_edit import assert_same_dump
from test_gpu_rebuild import assert_same_structure
from test_gpu_transform import begin_again, matrix, rotation
from test_gpu_update import SCHEDULES, assert_same_outputs, manager, moved_camera, outputs

pytestmark = pytest.mark.gpu

W, H = 64, 48
GPU = abi.FLAG_GPU_BUILD


def soup(n, seed=13):
    return scenes.soup(n, W, H, seed=seed, hdri_size=(32, 16))


def tail_of(sc, k, start=0):
    """k triangles of another scene as the `append` of a topology edit"""
    return {name: getattr(sc, name)[start:start + k].copy() for name in topology.ARRAYS}      # (copies: a test may edit them)


def equals_fresh(rm, sc_new, what, flags=0, rank=0, world=1, structure=True, samples=2):
    """rm (just edited) against a fresh create + begin of sc_new: outputs right after, the structure byte for byte with the checker's
    23 checks, then `samples` samples on both: outputs, counters, samples done, light info, adaptive info.  Returns nothing: the
    fresh manager is closed."""
    fresh = manager(sc_new, flags, rank, world)
    try:
        assert rm.get_render_info().samples == fresh.get_render_info().samples, what
        assert_same_outputs(outputs(rm), outputs(fresh), what + ": right after the edit")
        if structure:
            assert_same_structure(rm, fresh, sc_new, what)
        rm.render(samples)
        fresh.render(samples)
        assert_same_outputs(outputs(rm), outputs(fresh), f"{what}: {samples} spp later")
        assert rm.counters() == fresh.counters(), what
        assert rm.get_render_info().samples == fresh.get_render_info().samples == samples + 1
        assert rm.light_info() == fresh.light_info(), what
        assert rm.adaptive_info() == fresh.adaptive_info() and rm.adaptive_info()["enabled"] == 0
    finally:
        fresh.close()


def edit(rm, sc, what, flags=0, rank=0, world=1, **kw):
    """one topology edit on rm (holding sc) checked against fresh; returns the edited SceneData"""
    new = topology.apply(sc, **{k: v for k, v in kw.items() if k != "as_object"})
    rm.topology(**kw)
    info = rm.topology_info()
    assert info["tri_count"] == new.tri_count and info["removed"] == (0 if kw.get("remove") is None else len(kw["remove"]))
    assert info["appended"] == (0 if kw.get("append") is None else len(kw["append"]["vertices"]))
    equals_fresh(rm, new, what, flags, rank, world)
    return new


# ---- equals fresh, per schedule ----

@pytest.mark.parametrize("size,builder", [(257, "default"), (257, "device"), (513, "device")])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_edits_equal_fresh_scenes(schedule, size, builder):
    """remove only (id 0, the last id, every other id, a run of 256 that starts on a multiple of 256), append only, and both with a
    camera in `rest`, one after the other on one begun scene: 257 triangles through the default (host) builder (path 0), 257 and 513
    through the device builder and the geometry store.  The first step removes as many as it appends, so it fills the store (path 2)
    and leaves the size as it was; every later step compacts on the device (path 1).  Every other id is then removed from exactly
    `size` triangles, and the run of 256 (ids 256..511 of 513) as well, so that the scan crosses block edges with a one-element
    tail.  Ids 0..255 of 257 would leave one triangle, which only the host builder takes (path 0, no compaction on the device):
    there the append before it leaves 262, and the run's survivors are the six-element tail."""
    flags = SCHEDULES[schedule] | (GPU if builder == "device" else 0)
    sc = soup(size)
    other = soup(300, seed=5)
    run_from = 256 * ((size - 1) // 256 - 1)      # 0 of 257, 256 of 513
    rm = manager(sc, flags)
    try:
        rm.render(2)
        steps = [("both, with a camera", dict(remove=[3, 1, 10], append=tail_of(other, 3, 9), camera=moved_camera(sc))),
                 ("every other id", dict(remove="even")),
                 ("append only", dict(append=tail_of(other, max(size, 262) - size // 2, 20))),
                 ("a run of 256 from a multiple of 256", dict(remove=np.arange(run_from, run_from + 256))),
                 ("id 0", dict(remove=[0])), ("the last id", dict(remove=[-1]))]
        sizes = []
        for k, (what, kw) in enumerate(steps):
            n = sc.tri_count
            sizes.append(n)
            if "remove" in kw:
                kw["remove"] = np.arange(0, n, 2) if isinstance(kw["remove"], str) else np.asarray(kw["remove"]) % n
            sc = edit(rm, sc, f"{schedule}, {size}: {what}", flags, **kw)
            info = rm.topology_info()
            assert info["path"] == (0 if builder == "default" else 2 if k == 0 else 1), what
            if info["path"] == 1 and "remove" in kw:
                assert info["store_ms"] > 0, what      # the mark, the scan and the gather ran
            elif info["path"] != 1:
                assert info["store_ms"] == 0, what
            assert rm.accel_info()["builder"] == (1 if builder == "device" else 0)
        assert sizes == [size, size, size // 2, max(size, 262), max(size, 262) - 256, max(size, 262) - 257]
        assert rm.topology_info()["calls"] == len(steps)
    finally:
        rm.close()


# ---- shrinking to the edges ----

def test_down_to_three_two_and_no_triangles_and_back():
    sc = soup(257)
    rm = manager(sc, GPU)
    try:
        rm.render(2)
        sc = edit(rm, sc, "all but 3", GPU, remove=np.arange(3, 257))
        assert rm.accel_info()["builder"] == 1 and rm.topology_info()["path"] == 2      # the device builder still accepts: ER_BVH_LEAF_MAX is 2
        sc = edit(rm, sc, "all but 2", GPU, remove=[1])
        assert rm.accel_info()["builder"] == 0 and rm.topology_info()["path"] == 0      # the host build
        sc = edit(rm, sc, "all", GPU, remove=[0, 1])
        assert sc.tri_count == 0 and rm.topology_info()["tri_count"] == 0
        c = rm.counters()
        assert c["shaded_hits"] == 0                                                      # every ray sees the HDRI
        sc = edit(rm, sc, "onto the empty scene", GPU, append=tail_of(soup(40, seed=5), 9))
        assert rm.accel_info()["builder"] == 1 and rm.topology_info()["path"] == 2
        sc = edit(rm, sc, "and again", GPU, remove=[8], append=tail_of(soup(40, seed=5), 4, 20))
        assert rm.topology_info()["path"] == 1
    finally:
        rm.close()


# ---- the store ----

def test_the_store_is_resident_until_another_edit_writes_geometry():
    """edit (path 2), edit (path 1), er_render_update of the same arrays, edit (path 2 again); each equals fresh, and on path 1
    bytes_uploaded is the same for 257 and 6000 triangles given the same lists"""
    other = soup(40, seed=5)
    uploaded = {}
    for size in (257, 6000):
        sc = soup(size)
        rm = manager(sc, GPU)
        try:
            rm.render(2)
            sc = edit(rm, sc, f"{size}: first edit", GPU, remove=[5, 0, 200], append=tail_of(other, 3))
            info = rm.topology_info()
            assert info["path"] == 2 and info["bytes_uploaded"] == 140 * sc.tri_count and info["store_ms"] == 0
            sc = edit(rm, sc, f"{size}: second edit", GPU, remove=np.arange(100, 164), append=tail_of(other, 6, 3))
            info = rm.topology_info()
            assert info["path"] == 1 and info["bytes_uploaded"] == topology.bytes_uploaded(64, 6) and info["build_ms"] > 0
            uploaded[size] = info["bytes_uploaded"]
            rm.update(vertices=sc.vertices)      # the same arrays: the scene does not change, the store is released all the same
            sc = edit(rm, sc, f"{size}: after an update", GPU, remove=[7], append=tail_of(other, 2, 30))
            assert rm.topology_info()["path"] == 2
            sc = edit(rm, sc, f"{size}: remove only on the store", GPU, remove=[0, sc.tri_count - 1])
            assert rm.topology_info()["path"] == 1 and rm.topology_info()["bytes_uploaded"] == 8
            rm.edit(materials=sc.materials, material_id=sc.material_id)      # material ids written by another call
            sc = edit(rm, sc, f"{size}: after new material ids", GPU, append=tail_of(other, 1))
            assert rm.topology_info()["path"] == 2
        finally:
            rm.close()
    assert uploaded[257] == uploaded[6000]


# ---- objects ----

def test_the_object_table_survives_renumbered():
    sc = soup(257)
    objects = [np.arange(0, 40), np.arange(40, 100), np.array([120]), np.arange(150, 200)[::-1]]
    front = soup(2, seed=3)      # two triangles in front of everything: what a pick finds
    front.vertices[:] = np.array([[[-0.4, -0.3, 1.5], [0.4, -0.3, 1.5], [0.0, 0.4, 1.5]], [[-0.4, 0.35, 1.5], [0.4, 0.35, 1.5], [0.0, 0.5, 1.5]]], np.float32)
    front.normals[:] = np.array([0, 0, -1], np.float32)
    front.tangents[:] = np.array([1, 0, 0], np.float32)
    tail = tail_of(front, 2)
    m0 = matrix(rotation((0, 1, 0), 0.3), (0.1, 0, 0.2), about=(0, 0, 3))
    m1 = matrix(np.eye(3) * 1.2, (0, 0.1, 0))
    m1b = matrix(rotation((1, 0, 0), -0.2), (-0.1, 0, 0), about=(0, 0, 3))
    m4 = matrix(np.eye(3), (0.05, -0.02, 0.1))
    remove = np.concatenate([np.arange(40, 70), [120], [250]])      # half of object 1, all of object 2, a triangle in no object
    A = manager(sc)
    try:
        A.set_objects(objects)
        A.render(2)
        A.transform({0: m0, 1: m1})
        before = [A.update_info(), A.transform_info()["calls"]]
        A.topology(remove=remove, append=tail, as_object=True)
        assert [A.update_info(), A.transform_info()["calls"]] == before
        A.transform({1: m1b, 4: m4})
        # the same absolute poses on a fresh scene made from the edited REST arrays with the renumbered table
        rest = topology.apply(sc, remove=remove, append=tail)
        table = topology.remap_objects(objects, remove, sc.tri_count, append_count=2, as_object=True)
        assert [len(o) for o in table] == [40, 30, 0, 50, 2] and table[4].tolist() == [rest.tri_count - 2, rest.tri_count - 1]
        B = manager(rest)
        try:
            B.set_objects(table)
            B.transform({0: m0, 1: m1b, 4: m4})
            assert_same_outputs(outputs(A), outputs(B), "right after the transforms")
            for rm in (A, B):
                rm.render(2)
            assert_same_outputs(outputs(A), outputs(B), "2 spp later")
            # the id planes report the renumbered ids; a pick on an appended triangle returns the new object
            for rm in (A, B):
                rm.render_ids(1)
            for kind in ("triangle", "object", "material"):
                a, b = A.get_ids(kind), B.get_ids(kind)
                assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), kind
            tri, obj = A.get_ids("triangle")[0][..., 0], A.get_ids("object")[0][..., 0]
            hit = tri != abi.ID_NONE
            appended = hit & (tri >= rest.tri_count - 2)
            assert appended.any() and (tri[hit] < rest.tri_count).all()
            assert (obj[appended] == 4).all()
            seen = np.unique(obj[hit & ~appended])
            assert set(seen.tolist()) <= {0, 1, 3, abi.ID_NONE} and len(seen) > 1
            y, x = np.argwhere(appended)[0]
            p = A.pick(int(x), int(y))
            assert p["hit"] == 1 and p["object"] == 4 and p["triangle"] == tri[y, x]
        finally:
            B.close()
    finally:
        A.close()


# ---- rest ----

def test_appended_triangles_use_a_material_and_a_texture_of_the_same_call():
    sc = scenes.cornell_textured(W, H)
    rng = np.random.default_rng(4)
    tex = (rng.random((8, 8, 3)).astype(np.float32), 8, 8, 3, 0)
    mats = list(sc.materials) + [abi.default_material(albedo=(0.9, 0.9, 0.9), albedo_tex=len(sc.textures), roughness=0.6)]
    tail = tail_of(sc, 2)      # the floor again, a little higher
    tail["vertices"] = tail["vertices"] + np.array([0, 0.3, 0], np.float32)
    tail["material_id"][:] = len(sc.materials)
    kw = dict(append=tail, materials=mats, textures=[None] * len(sc.textures) + [tex])
    for flags in (0, GPU):
        rm = manager(sc, flags)
        try:
            rm.render(2)
            before = rm.edit_info()
            new = topology.apply(sc, **kw)
            rm.topology(**kw)
            info = rm.topology_info()
            assert info["texture_stage"] == 2 and info["texture_stage_ms"] > 0 and rm.edit_info() == before
            fresh = manager(new, flags)
            try:
                assert_same_dump(rm.debug_read_textures(), fresh.debug_read_textures(), "a texture added with the triangles")
            finally:
                fresh.close()
            equals_fresh(rm, new, "a material and a texture added with the triangles", flags)
            # a refused material id of an appended triangle: beyond the list the same call gives
            bad = dict(kw, append=dict(tail, material_id=tail["material_id"] + 1))
            with pytest.raises(abi.ErError) as e:
                rm.topology(**bad)
            assert e.value.code == abi.ER_ERR_INVALID_ARG and "material_id" in str(e.value)
        finally:
            rm.close()


# ---- mesh lights ----

def test_mesh_lights_follow_the_emitters_removal_and_return():
    flags = abi.FLAG_MESH_LIGHTS
    sc = scenes.cornell(W, H)
    emissive = [i for i, m in enumerate(sc.materials) if m.emission.x > 0]
    lit = np.flatnonzero(np.isin(sc.material_id, emissive))
    assert len(lit) == 2 and lit[1] == lit[0] + 1
    rm = manager(sc, flags)
    try:
        rm.render(2)
        assert rm.light_info()["emitters"] == 2
        dark = edit(rm, sc, "the only emitter removed", flags, remove=lit)
        assert rm.light_info()["emitters"] == 0
        back = edit(rm, dark, "an emitter appended onto a scene without one", flags, append=tail_of(sc, 2, int(lit[0])))
        assert rm.light_info()["emitters"] == 2 and back.tri_count == sc.tri_count
    finally:
        rm.close()


# ---- sharding ----

def test_rank_1_of_3():
    sc = soup(257)
    rm = manager(sc, GPU, rank=1, world=3)
    try:
        rm.render(2)
        edit(rm, sc, "rank 1 of 3", GPU, 1, 3, remove=np.arange(0, 257, 3), append=tail_of(soup(40, seed=5), 11), camera=moved_camera(sc))
    finally:
        rm.close()


# ---- state handling ----

INFOS = ("update_info", "edit_info", "sparse_info", "transform_info", "rebuild_info")


def test_state_after_an_edit():
    """adaptive sampling is off again, feature and id planes are invalid, the counts of the other edit paths do not move"""
    sc = soup(257)
    rm = manager(sc)
    try:
        rm.set_update_policy(abi.REBUILD_AUTO, 1.5)
        rm.set_adaptive(1e-3, 3, 1)
        rm.render(2)
        rm.update(vertices=sc.vertices)      # (a refit: the rebuild baseline and the sparse refit's level lists exist)
        rm.render_features(2)
        rm.render_ids(2)
        assert rm.feature_info()["valid"] == 1 and rm.id_info()["valid"] == 1
        before = {k: getattr(rm, k)() for k in INFOS}
        new = topology.apply(sc, remove=[1, 2], append=tail_of(soup(40, seed=5), 3))
        rm.topology(remove=[1, 2], append=tail_of(soup(40, seed=5), 3))
        assert {k: getattr(rm, k)() for k in INFOS} == before
        assert rm.adaptive_info()["enabled"] == 0 and rm.feature_info()["valid"] == 0 and rm.id_info()["valid"] == 0
        assert rm.accel_info()["builder"] in (0, 1)
        with pytest.raises(abi.ErError) as e:
            rm.get_feature("albedo")
        assert e.value.code == abi.ER_ERR_STATE
        fresh = manager(new)
        try:
            fresh.set_update_policy(abi.REBUILD_AUTO, 1.5)
            assert_same_structure(rm, fresh, new, "after a refit and an edit")
            # the rebuild baseline is forgotten, as after any build: the next update under AUTO decides as on the fresh scene
            v = new.vertices + np.float32(0.01)
            for m in (rm, fresh):
                m.update(vertices=v)
            a, b = rm.rebuild_info(), fresh.rebuild_info()
            assert a["last_decision"] == b["last_decision"] and a["cost_built"] == b["cost_built"] and a["cost_refit"] == b["cost_refit"]
            for m in (rm, fresh):
                m.render(2)
            assert_same_outputs(outputs(rm), outputs(fresh), "an update after the edit")
        finally:
            fresh.close()
    finally:
        rm.close()


def test_refused_edits_leave_everything_as_it_was():
    sc = soup(257)
    n = sc.tri_count
    rm, twin = manager(sc, GPU), manager(sc, GPU)
    try:
        rm.render(2)
        twin.render(2)
        good = tail_of(soup(40, seed=5), 2)
        bad_v = dict(good, vertices=good["vertices"].copy())
        bad_v["vertices"][1, 2, 0] = np.nan
        for kw, word in ((dict(remove=[n]), "not below tri_count"), (dict(remove=[4, 9, 4]), "removed twice"), (dict(append=bad_v), "not finite"),
                         (dict(append=dict(good, material_id=np.array([0, 1], np.int32))), "material_id"),
                         (dict(remove=[0], materials=sc.materials, material_id=np.full(n - 1, 1, np.int32)), "material_id"),
                         (dict(camera=moved_camera(sc)), "neither")):
            with pytest.raises(abi.ErError) as e:
                rm.topology(**kw)
            assert e.value.code == abi.ER_ERR_INVALID_ARG and word in str(e.value), (list(kw), str(e.value))
        ids = np.array([1, 2], np.uint32)

        def raw(**fields):
            t = abi.ErTopologyEdit()
            t.what, t.remove_count, t.remove_ids = abi.TOPO_REMOVE, 2, ids.ctypes.data_as(C.POINTER(C.c_uint32))
            for k, v in fields.items():
                if k == "rest_what":
                    t.rest.what = v
                else:
                    setattr(t, k, v)
            rc = rm.lib.er_render_topology(rm.handle, C.byref(t))
            assert rc == abi.ER_ERR_INVALID_ARG, (fields, rc, rm.lib.er_last_error())

        raw(what=0)
        raw(what=abi.TOPO_REMOVE | 4)
        raw(remove_count=0)
        raw(remove_ids=None)
        raw(what=abi.TOPO_REMOVE | abi.TOPO_APPEND, append_count=0)
        raw(what=abi.TOPO_REMOVE | abi.TOPO_APPEND, append_count=2)      # without its arrays
        raw(rest_what=abi.EDIT_GEOMETRY)
        raw(rest_what=abi.EDIT_CAMERA | 32)
        raw(rest_what=abi.EDIT_MATERIALS)                                # what er_render_edit refuses: the bit without its list
        assert rm.topology_info() == twin.topology_info() and rm.topology_info()["calls"] == 0
        assert_same_structure(rm, twin, sc, "after refused edits")
        for m in (rm, twin):
            m.render(2)
        assert_same_outputs(outputs(rm), outputs(twin), "after refused edits")
        assert rm.counters() == twin.counters()
    finally:
        rm.close()
        twin.close()


# ---- builder failure (er_debug_set_gpu_build_failure simulates a return code; nothing faults) ----

def test_a_failed_device_build_unforced_falls_to_the_host_builder(monkeypatch):
    monkeypatch.setenv("ER_GPU_BUILD_MIN_TRIS", "1000")
    sc = soup(6000)
    kw = dict(remove=np.arange(10, 50), append=tail_of(soup(40, seed=5), 4))
    new = topology.apply(sc, **kw)
    rm = manager(sc)
    try:
        assert rm.accel_info()["builder"] == 1
        rm.render(2)
        rm.lib.er_debug_set_gpu_build_failure(1)
        try:
            rm.topology(**kw)
        finally:
            rm.lib.er_debug_set_gpu_build_failure(0)
        assert rm.accel_info()["builder"] == 0 and rm.topology_info()["path"] == 0 and rm.topology_info()["bytes_uploaded"] == 0
        equals_fresh(rm, new, "the host builder took over", abi.FLAG_HOST_BUILD)
        sc2 = edit(rm, new, "the next edit builds on the device again", remove=[0])
        assert rm.accel_info()["builder"] == 1 and rm.topology_info()["path"] == 2 and sc2.tri_count == new.tri_count - 1
    finally:
        rm.close()


def test_a_failed_device_build_forced_fails_the_call_and_a_begin_renders_the_edited_scene():
    sc = soup(257)
    kw = dict(remove=[0, 100, 256], append=tail_of(soup(40, seed=5), 4))
    new = topology.apply(sc, **kw)
    rm = manager(sc, GPU)
    try:
        rm.render(2)
        rm.lib.er_debug_set_gpu_build_failure(1)
        try:
            with pytest.raises(abi.ErError) as e:
                rm.topology(**kw)
        finally:
            rm.lib.er_debug_set_gpu_build_failure(0)
        assert e.value.code == abi.ER_ERR_HIP and "simulated failure" in str(e.value)
        assert rm.topology_info()["calls"] == 0
        for call in (lambda: rm.render(1), lambda: rm.topology(remove=[0]), lambda: rm.update(camera=moved_camera(sc))):
            with pytest.raises(abi.ErError) as e:
                call()
            assert e.value.code == abi.ER_ERR_STATE
        begin_again(rm)      # builds from the edited host copy
        equals_fresh(rm, new, "er_render_begin after the failed edit", GPU)
        edit(rm, new, "and an edit after that", GPU, remove=[1])
        assert rm.topology_info()["path"] == 2 and rm.topology_info()["calls"] == 1
    finally:
        rm.close()


# ---- host ----

def extra_object():
    """a small quad in the box as OBJ text (the loader flips z)"""
    pts = [(-0.5, -0.6, 2.6), (0.5, -0.6, 2.6), (0.5, -0.6, 3.4), (-0.5, -0.6, 3.4)]
    lines = ["o shelf"]
    for p in pts:
        lines.append("v %.9g %.9g %.9g" % (p[0], p[1], -p[2]))
    lines += ["vn 0 1 0", "vt 0 0", "vt 1 0", "vt 1 1", "vt 0 1", "usemtl red", "f 1/1/1 3/3/1 2/2/1", "f 1/1/1 4/4/1 3/3/1"]
    return "\n".join(lines) + "\n", "newmtl red\nKd 0.5 0.5 0.5\n"


def test_host_session_answers_an_object_load_by_a_topology_edit(tmp_path):
    """start, --load_object, start through eleven_server: the server takes the topology path (get_info: topology_edits) and the image
    equals a direct ABI render (er_scene_create + er_render_begin) of the combined scene, made here from the two OBJ texts"""
    from test_host_server import Server, session_scene

    a = client.cornell_session_assets(48, 48)
    obj, mtl = extra_object()
    s = Server()
    c = client.Client(port=s.port)
    first_img = client.play_cornell_session(c, a, sample_target=4)
    assert c.get_info()["topology_edits"] == 0
    c.load_object(obj, mtl)
    c.start()
    deadline = time.time() + 120
    while c.get_info()["samples"] < 5:      # (every poll is a round trip to the server: no sleep between them)
        assert time.time() < deadline, "render did not reach the sample target"
    edited = c.get_pass("beauty", 48, 48)
    info = c.get_info()
    c.close()
    assert s.finish() == 0
    assert info["topology_edits"] == 1 and info["scene_edits"] == 0 and info["camera_updates"] == 0 and info["samples"] == 5
    shelf = session_scene(dict(a, obj=obj), tmp_path)
    assert shelf.tri_count == 2
    combined = topology.apply(session_scene(a, tmp_path), append=tail_of(shelf, 2))
    rm = render.RenderingManager(render.RenderParameters())      # the server's defaults, as in test_host_server
    rm.start_rendering(combined)
    try:
        rm.render(4)
        ref = rm.get_pass("beauty")
    finally:
        rm.close()
    assert (edited.view(np.uint32) == ref.view(np.uint32)).all()
    assert (edited.view(np.uint32) != first_img.view(np.uint32)).any()
