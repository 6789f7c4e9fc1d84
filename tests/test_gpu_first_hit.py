"""The first-hit camera pass (csrc/er_first_hit.h) where its four consumers -- er_render_features, er_render_ids, er_pick and the key pass
of er_history_* -- share code that no other test reaches.

(1) THE STRIDE FRAME.  The pass launches 4 workgroups per CU and walks the owned tiles with a grid stride; every other feature, id or
history test uses a frame of at most 54 tiles, so the walk's second trip runs under no assertion.  Here the frame is the smallest one
whose whole-frame share needs a second trip and has a partial last tile column and row: 261 pixels across (33 tiles, the last 5 wide) and
ceil((4 CUs + 1) / 33) tile rows, the last 3 pixels high.  Features and ids of one rank (two trips) against three ranks on the one GPU,
gathered (a third of the tiles each: one trip); er_pick in the last tile row against a one-ray id pass; the history of a moved camera
against the replay of tests/test_gpu_history.py; and, by the oracle alone, that the tiles only the second trip reaches show neither only
sky nor only hits -- a skipped trip could otherwise hide behind a cleared buffer.

(2) THE TRIG KNOB.  ER_CAM_TRIG_ON_DEVICE at er_render_begin makes the pass evaluate the camera's six sines and cosines on the device
instead of taking the host's: all four consumers must give the same bits either way."""
import ctypes as C
import functools

import numpy as np
import pytest

from elevenrender_amd import abi, history, render, scenes
from test_gpu_history import assert_words, key_plane, resolve
from test_gpu_ids import KINDS, all_planes, assert_same_planes, ids_manager, table
from test_gpu_update import moved_camera, with_arrays

pytestmark = pytest.mark.gpu
f32 = np.float32
bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)
X_RES, TILES_X, N = 261, 33, 2
# Chosen on the CPU with the oracle alone, for the 256 CUs of an MI355X (test_the_tiles_of_the_second_trip_show_geometry_and_sky: 0.358).
# The frame follows the device's CU count, the scene does not: which tiles come last, and what the camera sees there, changes with the
# count (the same scene gives 0.30 at 104 CUs, 0.18 at 64 and 0.01 at 304, where the last tiles are the sky of the bottom right corner),
# so on another device that test fails and says that the two have to be chosen again -- it must not pass on an input that proves nothing.
TRIS, SEED = 3000, 7


def blocks():
    """the workgroups the pass launches on device 0: 4 per CU"""
    return 4 * render.list_devices()[0]["max_compute_units"]


@functools.lru_cache(maxsize=None)
def stride_scene():
    rows = -(-(blocks() + 1) // TILES_X)
    return scenes.torture(TRIS, X_RES, 8 * rows - 5, seed=SEED, n_materials=8, tex_size=32, hdri_size=(64, 32), n_lights=4)


def second_trip(sc):
    """(H, W) bool: the pixels of the tiles with list index >= the workgroup count (one rank: the list is the frame's tiles, row-major)"""
    ys, xs = np.mgrid[0:sc.y_res, 0:sc.x_res]
    return (ys // 8) * TILES_X + xs // 8 >= blocks()


@functools.lru_cache(maxsize=None)
def snapshots():
    """the replay's states before and after the camera move (test_gpu_history.State.snapshot, without poses), computed once and shared"""
    sc, cam = stride_scene(), moved_camera(stride_scene())
    objects = table(sc)
    identity = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(f32).reshape(12)
    poses = np.tile(identity, (len(objects), 1))
    old = dict(key=key_plane(sc, objects), cam=abi.debug_history_camera(sc.camera), poses=poses)
    new = dict(key=key_plane(with_arrays(sc, camera=cam), objects), cam=abi.debug_history_camera(cam), poses=poses)
    return old, new, cam


def test_the_frame_needs_a_second_trip_and_a_third_of_it_does_not():
    sc = stride_scene()
    tiles_y = (sc.y_res + 7) // 8
    assert sc.x_res % 8 == 5 and sc.y_res % 8 == 3 and TILES_X == (sc.x_res + 7) // 8
    assert TILES_X * tiles_y > blocks() >= TILES_X * (tiles_y - 1)                  # the smallest such frame
    ty, tx = np.mgrid[0:tiles_y, 0:TILES_X]
    assert max(int(((tx + ty) % 3 == r).sum()) for r in range(3)) <= blocks()       # a rank of three takes a single trip
    late = second_trip(sc)
    assert late[-1, -1] and late.sum() > 0


def test_the_tiles_of_the_second_trip_show_geometry_and_sky():
    """the oracle alone, on this input: the closest hits of the pinhole rays"""
    sc = stride_scene()
    late = second_trip(sc).reshape(-1)
    for what, state in zip(("scene camera", "moved camera"), snapshots()[:2]):
        share = float((state["key"]["hit"][late] != 0).mean())
        print(f"{sc.x_res} x {sc.y_res}, {blocks()} workgroups: {int(late.sum())} pixels in second-trip tiles, {share:.3f} of their pinhole rays hit ({what})")
        if what == "scene camera":
            assert 0.2 <= share <= 0.8, f"{share:.3f}: TRIS and SEED were chosen for 1 024 workgroups, choose them again for {blocks()}"


def test_features_and_ids_of_two_trips_equal_three_ranks_of_one_trip():
    lib = abi.load()
    sc = stride_scene()
    one = ids_manager(sc)
    try:
        one.render_features(N)
        one.render_ids(N)
        assert one.feature_info()["rays"] == one.id_info()["rays"] == N * sc.x_res * sc.y_res
        want = {n: one.get_feature(n) for n in ("albedo", "depth")}
        want_ids = all_planes(one)
    finally:
        one.close()
    late = second_trip(sc)
    cov = want["albedo"][..., 3]
    print(f"coverage of the second trip's pixels: mean {cov[late].mean():.3f}, of the others {cov[~late].mean():.3f}")
    world, root = 3, 0
    comms = (C.c_void_p * world)()
    abi.check(lib.er_comm_create_local(world, comms))
    rms = [ids_manager(sc, rank=r, world=world) for r in range(world)]
    try:
        for rm in rms:
            rm.render_features(N)
            rm.render_ids(N)
        for info in ([rm.feature_info() for rm in rms], [rm.id_info() for rm in rms]):
            assert sum(i["rays"] for i in info) == N * sc.x_res * sc.y_res and all(i["rays"] > 0 for i in info)
        order = [r for r in range(world) if r != root] + [root]
        for f in (abi.FEATURE_ALBEDO, abi.FEATURE_DEPTH):
            for r in order:
                abi.check(lib.er_gather_feature(rms[r].handle, f, comms[r], root))
        for kind in range(abi.ID_KIND_COUNT):
            for r in order:
                abi.check(lib.er_gather_ids(rms[r].handle, kind, comms[r], root))
        for n in ("albedo", "depth"):
            got = rms[root].get_feature(n)
            bad = (bits(got) != bits(want[n])).any(-1)
            assert not bad.any(), f"{n}: {int(bad.sum())} pixels differ, {int((bad & late).sum())} of them in second-trip tiles"
        assert_same_planes(all_planes(rms[root]), want_ids, "three ranks gathered against one rank")
    finally:
        for rm in rms:
            rm.close()
        for c in comms:
            lib.er_comm_destroy(c)


def test_pick_in_the_last_tile_row_equals_slot_0_of_a_one_ray_id_pass():
    sc = stride_scene()
    late = second_trip(sc)
    rm = ids_manager(sc)
    try:
        rm.render_ids(1)
        rm.render_features(1)
        planes, depth = all_planes(rm), rm.get_feature("depth")
        cols = np.nonzero(late[-1])[0]                                               # the last tile row's columns that only the second trip reaches
        xs = [int(cols[min(1, len(cols) - 1)]), int(cols[len(cols) // 3]), int(cols[2 * len(cols) // 3]), sc.x_res - 1]
        for x, y in zip(xs, (sc.y_res - 3, sc.y_res - 2, sc.y_res - 1, sc.y_res - 1)):   # the last: the partial corner tile
            assert late[y, x]
            p = rm.pick(x, y)
            assert p["hit"] == int(planes["triangle"][1][y, x, 0]), (x, y)
            for k in KINDS:
                assert p[k] == int(planes[k][0][y, x, 0]), (x, y, k)
            assert bits(p["distance"]) == bits(depth[y, x, 0]), (x, y)
    finally:
        rm.close()


def test_history_over_two_trips_equals_the_replay():
    sc = stride_scene()
    npx = sc.x_res * sc.y_res
    old, new, cam = snapshots()
    rm = render.RenderingManager(render.RenderParameters(max_bounces=2))
    rm.start_rendering(sc)
    try:
        rm.set_objects(table(sc))
        rm.render(2)
        beauty, samples = rm.get_pass("beauty"), rm.read_samples()
        rm.history_capture()
        rm.update(camera=cam)
        rm.history_resolve()
        got_hist = rm.get_history()
        rm.render(2)
        got_blend = rm.get_blended()
        want_hist, _, cls, moved = resolve(old, new, history.capture(beauty, samples, None, 32.0), sc.x_res, sc.y_res)
        assert_words(got_hist, want_hist, "stride frame, camera: history")
        assert_words(got_blend, history.blend(rm.get_pass("beauty"), rm.read_samples(), want_hist), "stride frame, camera: blend")
        info, c = rm.history_info(), history.class_counts(cls)
        print("classes", c)
        assert {k: info["pixels_" + k] for k in history.CLASS_NAMES} == c and sum(c.values()) == npx, (info, c)
        assert (info["captured"], info["resolved"], info["moved_objects"]) == (1, 1, moved) and moved == 0
    finally:
        rm.close()


# ---- (2) ----

def knob_outputs(sc):
    rm = ids_manager(sc, max_bounces=2)
    try:
        rm.render_features(4)
        rm.render_ids(4)
        out = {n: bits(rm.get_feature(n)) for n in ("albedo", "depth")}
        for k, (i, c) in all_planes(rm).items():
            out[k + " ids"], out[k + " counts"] = i, c
        y, x = np.argwhere(out["albedo"].view(f32)[..., 3] == 1)[0]                   # a pixel all of whose rays hit
        p = rm.pick(int(x), int(y))
        out["pick"] = np.concatenate([np.array([p["hit"], p["triangle"], p["object"], p["material"]], np.uint32), bits(p["distance"]).reshape(1),
                                      bits(p["position"]), bits(p["uv"])])
        rm.render(2)
        rm.history_capture()
        rm.update(camera=moved_camera(sc))
        rm.history_resolve()
        out["history"] = bits(rm.get_history())
        info = rm.history_info()
        out["classes"] = np.array([info["pixels_" + k] for k in history.CLASS_NAMES], np.uint64)
        return out
    finally:
        rm.close()


def test_the_cameras_trig_from_the_host_or_on_the_device_gives_the_same_bits(monkeypatch):
    sc = scenes.torture(4000, 70, 45, seed=7, n_materials=8, tex_size=32, hdri_size=(64, 32), n_lights=4)
    sc.camera.bokeh = 1                                                              # a rotated thin-lens camera: the trig turns the lens sample too
    sc.camera.focus_distance = 3.0
    sc.camera.rotation = abi.ErVec3(3.0, -5.0, 2.0)
    sc._desc = None
    # (Both sides are bit-equal by design, so the test cannot see a knob that took no effect: it runs the device branch only because
    # er_render_begin reads the environment at EVERY begin (er_api.cpp, where cam_trig_valid is set).  If that getenv is ever cached,
    # this test and the ER_CAM_TRIG_ON_DEVICE block of test_gpu_parity.py need another way to set the knob.)
    monkeypatch.delenv("ER_CAM_TRIG_ON_DEVICE", raising=False)
    host = knob_outputs(sc)
    monkeypatch.setenv("ER_CAM_TRIG_ON_DEVICE", "1")
    device = knob_outputs(sc)
    assert host["pick"][0] == 1 and 0 < host["albedo"].size and host["classes"].sum() == sc.x_res * sc.y_res
    cov = host["albedo"].view(f32)[..., 3]
    assert ((cov > 0) & (cov < 1)).any() and (cov == 0).any()                        # hits, misses and lens-blurred edges
    for k in host:
        assert (host[k] == device[k]).all(), f"{k}: {int((host[k] != device[k]).sum())} words differ with ER_CAM_TRIG_ON_DEVICE=1"
