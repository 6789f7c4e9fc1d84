"""Temporal reprojection on the GPU (er_history_capture / er_history_resolve / er_read_history / er_read_blended: csrc/er_history.hip and
csrc/er_reproject.h).

(1) history and blend word for word against a numpy replay composed from the oracle's entry points (oracle_camera_ray, Oracle.closest_hit,
oracle_tri_hit) and elevenrender_amd/history.py, fed the BEAUTY read before the capture, for a moved camera, posed objects, both, and the
same camera again; (2) accumulation over three edits and the weight cap; (3) a render with all of it in between equals the render
without; (4) what drops a capture and what keeps it; (5) the blend after a small camera move is nearer the converged frame than the
plain render."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as orc
from elevenrender_amd import abi, history, ids, render, scenes
from test_gpu_ids import BUILDERS
from test_gpu_transform import Replay, matrix, rotation
from test_gpu_update import SCHEDULES, assert_same_outputs, outputs, with_arrays

pytestmark = pytest.mark.gpu
f32 = np.float32
NONE = abi.ID_NONE
INV, STATE = abi.ER_ERR_INVALID_ARG, abi.ER_ERR_STATE
bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)
NAMES = ("large", "small")      # 70 x 45 over 4 050 triangles (partial tiles on both edges), 32 x 24 over 588
SHAPES = {"large": (70, 45, 9, 15), "small": (32, 24, 6, 7)}      # frame, panels, quads per panel side


@functools.lru_cache(maxsize=None)
def scene(name):
    """Tessellated, tilted, slightly buckled panels at depths 2.2 .. 3.8 in front of the sky, with the torture scene's materials,
    textures, HDRI and camera: surfaces wide enough for the four taps of a pixel to lie on one of them, edges, overlaps and gaps enough
    for every way a tap can fail."""
    x_res, y_res, panels, g = SHAPES[name]
    base = scenes.torture(panels * g * g * 2, x_res, y_res, seed=7, n_materials=8, tex_size=32, hdri_size=(64, 32), n_lights=4)
    rng = np.random.default_rng(21 if name == "large" else 23)
    depth = (2.5, 3.5, 3.0, 2.2, 3.8, 2.8, 3.2, 2.6, 3.6)
    tris = []
    for p in range(panels):
        centre = np.array([rng.uniform(-1.3, 1.3), rng.uniform(-0.8, 0.8), depth[p]])
        if p % 3 == 2:                                   # the panels in no object overlap one another: one "object" at several depths
            centre[:2] = (0.25 * (p // 3) - 0.3, 0.2 * (p // 3) - 0.2)
        if p == 1:                                       # behind panel 0 and half beside it: the two are ONE object, which hides part of itself
            centre[:2] = first[:2] + (0.35, 0.2)
        first = centre if p == 0 else first
        half = rng.uniform(0.55, 0.9, 2)
        R = rotation(rng.uniform(-1, 1, 3), rng.uniform(-0.5, 0.5))
        u, v = np.meshgrid(np.linspace(-1, 1, g + 1), np.linspace(-1, 1, g + 1), indexing="ij")
        local = np.stack([u * half[0], v * half[1], rng.uniform(-0.012, 0.012, u.shape)], -1)
        pts = local @ R.T + centre
        a, b, c, d = pts[:-1, :-1], pts[1:, :-1], pts[1:, 1:], pts[:-1, 1:]
        tris.append(np.concatenate([np.stack([a, b, c], 2).reshape(-1, 3, 3), np.stack([a, c, d], 2).reshape(-1, 3, 3)]))
    v = np.concatenate(tris).astype(f32)
    n, t = scenes.face_frame(v)
    return with_arrays(base, vertices=v, normals=n, tangents=t)


def table(sc):
    """panels 0 and 1 are object 0, every other panel an object of its own, but every third panel is in no object (a third of the
    triangles), and a last object is empty"""
    name = "large" if sc.x_res == 70 else "small"
    panels, g = SHAPES[name][2:]
    per = g * g * 2
    listed = [p for p in range(2, panels) if p % 3 != 2]
    return [np.arange(0, 2 * per, dtype=np.uint32)] + [np.arange(p * per, (p + 1) * per, dtype=np.uint32) for p in listed] + [np.zeros(0, np.uint32)]


# per frame: the camera's translation and rotation (degrees), and the angle object 0 turns by in units of 0.25 rad (the small frame's
# pixels are twice as wide: more parallax for strips as many pixels wide)
PARAMS = {"large": ((0.5, -0.2, -0.3), (3.0, -8.0, 1.0), 1.0), "small": ((1.3, 0.6, -0.7), (7.0, -14.0, 2.0), 2.5)}


def camera_of(sc, dpos=(0, 0, 0), rot=None):
    cam = abi.ErCamera.from_buffer_copy(sc.camera)
    cam.position = abi.ErVec3(sc.camera.position.x + dpos[0], sc.camera.position.y + dpos[1], sc.camera.position.z + dpos[2])
    if rot is not None:
        cam.rotation = abi.ErVec3(*rot)
    return cam


def object_centre(sc, objects, o):
    return sc.vertices.reshape(-1, 3, 3)[objects[o]].reshape(-1, 3).mean(0)


def moves(name, case):
    """(camera or None, {object: pose}) of a case -- chosen on the CPU with the replay alone (test_the_moves_exercise_every_class)"""
    sc = scene(name)
    objects = table(sc)
    dpos, rot, k = PARAMS[name]
    cam = camera_of(sc, dpos, rot)
    # object 0 turned about its own centre (its front panel slides over its back one); the object farthest from the view axis pulled
    # towards it and to depth 2, in front of the other
    centres = [object_centre(sc, objects, o) for o in range(1, len(objects) - 1)]
    far = 1 + int(np.argmax([np.hypot(c[0], c[1]) for c in centres]))
    c = centres[far - 1]
    poses = {0: matrix(rotation((0.1, 1.0, 0.0), 0.25 * k), t=(0.02, 0.0, 0.05), about=object_centre(sc, objects, 0)),
             far: matrix(rotation((0.0, 0.2, 1.0), 0.1), t=(-0.7 * c[0], -0.7 * c[1], 2.0 - c[2]), about=c)}
    return {"camera": (cam, {}), "objects": (None, poses), "both": (cam, poses), "same": (camera_of(sc), {})}[case]


# ---- the replay ----

def key_plane(sc, objects):
    """the key plane of a scene description: one pinhole ray per pixel (r1 = r2 = 0.5, bokeh 0) -> hit, object, dist, P, flat"""
    L = orc.lib()
    npx = sc.x_res * sc.y_res
    cam = abi.ErCamera.from_buffer_copy(sc.camera)
    cam.bokeh = 0
    origins, dirs = np.zeros((npx, 3), f32), np.zeros((npx, 3), f32)
    r = (C.c_float * 5)(0.5, 0.5, 0.0, 0.0, 0.0)
    for idx in range(npx):
        o, d = (C.c_float * 3)(), (C.c_float * 3)()
        L.oracle_camera_ray(C.byref(cam), sc.x_res, sc.y_res, idx % sc.x_res, idx // sc.x_res, r, orc.MATH_ER, o, d)
        origins[idx], dirs[idx] = o[:], d[:]
    o = orc.Oracle(sc, math_mode=orc.MATH_ER, max_bounces=1)
    tri, _ = o.closest_hit(origins, dirs)
    o.close()
    tri = np.asarray(tri, np.int64)
    V, N, T, UV = sc.vertices.reshape(-1, 9), sc.normals.reshape(-1, 9), sc.tangents.reshape(-1, 9), sc.uvs.reshape(-1, 6)
    fp = lambda a: np.ascontiguousarray(a, f32).ctypes.data_as(C.POINTER(C.c_float))
    P = dirs.copy()
    for idx in np.nonzero(tri >= 0)[0]:
        t = int(tri[idx])
        rec = np.zeros(17, f32)
        assert L.oracle_tri_hit(fp(V[t]), fp(N[t]), fp(T[t]), fp(UV[t]), float(sc.tangent_sign[t]), fp(origins[idx]), fp(dirs[idx]), fp(rec))
        P[idx] = rec[0:3]
    e = P - origins
    dist = np.where(tri >= 0, np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]), f32(0)).astype(f32)
    of = ids.object_of(sc.tri_count, objects) if objects is not None else np.full(sc.tri_count, NONE, np.uint32)
    obj = np.where(tri >= 0, of[np.maximum(tri, 0)], NONE).astype(np.uint32)
    return dict(hit=(tri >= 0).astype(np.uint32), obj=obj, dist=dist, P=P.astype(f32))


class State:
    """what the scene is after a sequence of cameras and poses: the description, its absolute poses and its key plane"""

    def __init__(self, name):
        self.sc, self.objects = scene(name), table(scene(name))
        self.rp = Replay(self.sc, self.objects)
        identity = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(f32).reshape(12)
        self.poses = np.tile(identity, (len(self.objects), 1))
        self.camera = abi.ErCamera.from_buffer_copy(self.sc.camera)

    def apply(self, camera, poses):
        if camera is not None:
            self.camera = abi.ErCamera.from_buffer_copy(camera)
        if poses:
            self.rp.transform(poses)
            for o, m in poses.items():
                self.poses[o] = np.asarray(m, f32).reshape(12)

    def snapshot(self):
        self.rp.camera = self.camera
        return dict(key=key_plane(self.rp.scene(), self.objects), cam=abi.debug_history_camera(self.camera), poses=self.poses.copy())


def resolve(old, new, cw, x_res, y_res, tol=0.02):
    """the history plane, the tap states and the classes of a resolve of `new` against the capture `old` with its (C, W) plane"""
    back, moved = history.back_table(old["poses"], new["poses"])
    k = new["key"]
    listed = (k["hit"] != 0) & (k["obj"] < len(back))
    o = np.where(listed, k["obj"], 0)
    px_back = np.where(listed[:, None], back[o], f32(0)).astype(f32)
    px_moved = np.where(listed, moved[o], 0).astype(np.uint32)
    ko = old["key"]
    return history.resolve(old["cam"], x_res, y_res, f32(tol), k["hit"], k["obj"], k["P"], px_moved, px_back, ko["hit"], ko["obj"], ko["dist"], cw) + (int(moved.sum()),)


def census(state, cls):
    """the pixel classes by name, the rejected ones split by why"""
    c = history.class_counts(cls)
    rej = cls == history.REJECTED
    c["rejected_object"] = int((rej & (state == history.TAP_OBJECT).any(1)).sum())
    c["rejected_depth"] = int((rej & (state == history.TAP_DEPTH).any(1)).sum())
    return c


@functools.lru_cache(maxsize=None)
def case_states(name, case):
    st = State(name)
    old = st.snapshot()
    st.apply(*moves(name, case))
    return old, st.snapshot()


def test_the_moves_exercise_every_class():
    """the oracle alone, on these inputs: a degenerate move cannot hide a failure"""
    for name in NAMES:
        sc = scene(name)
        npx = sc.x_res * sc.y_res
        for case in ("camera", "objects", "both"):
            old, new = case_states(name, case)
            _, state, cls, moved = resolve(old, new, np.ones((npx, 4), f32), sc.x_res, sc.y_res)
            c = census(state, cls)
            print(name, case, c, "moved objects", moved)
            assert c["valid"] >= 0.05 * npx, (name, case, c)
            for k in ("partial", "offscreen", "rejected_object", "rejected_depth", "sky"):
                assert c[k] >= 20, (name, case, k, c)
    for name in NAMES:
        objs = table(scene(name))
        assert len(objs[-1]) == 0 and sum(len(o) for o in objs) * 3 == scene(name).tri_count * 2      # an empty object; a third of the triangles in none


# ---- (1) ----

def history_manager(sc, flags=0, max_bounces=2, objects=True):
    rm = render.RenderingManager(render.RenderParameters(max_bounces=max_bounces, flags=flags))
    rm.start_rendering(sc)
    if objects:
        rm.set_objects(table(sc))
    return rm


def edit(rm, camera, poses):
    if poses:
        rm.transform(poses, camera=camera)
    else:
        rm.update(camera=camera)


def assert_words(got, want, what):
    bad = int((bits(got).reshape(-1, 4) != bits(want).reshape(-1, 4)).any(1).sum())
    assert bad == 0, f"{what}: {bad} pixels differ from the replay"


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", NAMES)
def test_history_and_blend_equal_the_replay(name, builder):
    sc = scene(name)
    npx = sc.x_res * sc.y_res
    for case in ("camera", "objects", "both", "same"):
        old, new = case_states(name, case)
        rm = history_manager(sc, BUILDERS[builder])
        try:
            assert rm.history_info() == dict(captured=0, resolved=0, moved_objects=0, pixels_valid=0, pixels_partial=0, pixels_offscreen=0, pixels_rejected=0,
                                             pixels_sky=0, capture_ms=0.0, resolve_ms=0.0)
            rm.render(8)
            beauty, samples = rm.get_pass("beauty"), rm.read_samples()
            rm.history_capture()
            info = rm.history_info()
            assert (info["captured"], info["resolved"]) == (1, 0) and info["capture_ms"] > 0
            edit(rm, *moves(name, case))
            rm.history_resolve()
            got_hist = rm.get_history()                                      # before the new samples: the history does not depend on them
            rm.render(2)
            beauty2, samples2 = rm.get_pass("beauty"), rm.read_samples()
            got_blend = rm.get_blended()
            cw = history.capture(beauty, samples, None, 32.0)
            want_hist, state, cls, moved = resolve(old, new, cw, sc.x_res, sc.y_res)
            assert_words(got_hist, want_hist, f"{name} {builder} {case} history")
            assert_words(rm.get_history(), want_hist, f"{name} {builder} {case} history after two samples")
            assert_words(got_blend, history.blend(beauty2, samples2, want_hist), f"{name} {builder} {case} blend")
            info = rm.history_info()
            c = history.class_counts(cls)
            assert {k: info["pixels_" + k] for k in history.CLASS_NAMES} == c and sum(c.values()) == npx, (case, info, c)
            assert (info["captured"], info["resolved"], info["moved_objects"]) == (1, 1, moved) and info["resolve_ms"] > 0
            assert moved == {"camera": 0, "objects": 2, "both": 2, "same": 0}[case]
            if case == "same":                                               # nothing moved: every hit pixel finds itself, weight n
                assert c["offscreen"] == c["rejected"] == 0 and c["valid"] > 0.5 * (npx - c["sky"])
            w = got_hist[..., 3]                                            # 8 samples after the setup one: n = 8 carried (a mean of equal weights, to rounding)
            assert (w <= 8 * (1 + 1e-6)).all() and w.max() >= 8 * (1 - 1e-6) and ((w == 0) | (w >= 8 * (1 - 1e-6))).all()
        finally:
            rm.close()


# ---- (2) ----

def test_history_accumulates_over_three_edits_up_to_the_cap():
    """Three edits in a row with 2 samples between them, max_weight 4.  The captured (C, W) is not handed out; the history a resolve makes
    of it is, so every capture is checked through the resolve that follows it, the replay chaining its own history into the next C."""
    name = "large"
    sc = scene(name)
    st = State(name)
    objects = table(sc)
    steps = [(camera_of(sc, (0.03, 0.0, -0.05), (0.5, -1.0, 0.0)), {}),
             (None, {2: matrix(t=(0.02, 0.01, 0.0))}),
             (camera_of(sc, (0.05, -0.02, -0.08), (1.0, -1.5, 0.2)), {2: matrix(rotation((0, 1, 0), 0.02), t=(0.03, 0.01, 0.0), about=object_centre(sc, objects, 2))})]
    rm = history_manager(sc)
    try:
        rm.render(2)
        want_hist, top, cap = None, [], []
        for camera, poses in steps:
            beauty, samples = rm.get_pass("beauty"), rm.read_samples()
            old = st.snapshot()
            rm.history_capture(max_weight=4.0)
            edit(rm, camera, poses)
            st.apply(camera, poses)
            rm.history_resolve()
            cw = history.capture(beauty, samples, want_hist, 4.0)
            cap.append(float(cw[:, 3].max()))
            want_hist = resolve(old, st.snapshot(), cw, sc.x_res, sc.y_res)[0]
            got = rm.get_history()
            assert_words(got, want_hist, f"edit {len(top)}")
            top.append(float(got[..., 3].max()))
            rm.render(2)
            assert_words(rm.get_blended(), history.blend(rm.get_pass("beauty"), rm.read_samples(), want_hist), f"blend {len(top)}")
        # n = 2 per round: W is 2, then min(2 + 2, 4), then min(4 + 2, 4) -- it reaches the cap and does not pass it
        assert cap == [2.0, 4.0, 4.0] and all(t <= 4 * (1 + 1e-6) for t in top) and top[1] >= 4 * (1 - 1e-6), (cap, top)
        # two more rounds under the same camera: the weight reaches the cap and does not pass it
        for _ in range(2):
            rm.history_capture(max_weight=4.0)
            rm.update(camera=st.camera)
            rm.history_resolve()
            rm.render(2)
        assert 4 * (1 - 1e-6) <= float(rm.get_history()[..., 3].max()) <= 4 * (1 + 1e-6)
    finally:
        rm.close()


# ---- (3) ----

@pytest.mark.parametrize("sched", ["stream", "wavefront"])
def test_history_leaves_the_render_alone(sched):
    sc = scene("large")
    camera, poses = moves("large", "both")
    got = []
    for with_history in (True, False):
        rm = history_manager(sc, SCHEDULES[sched], max_bounces=4)
        rm.render(3)
        if with_history:
            rm.history_capture()
        edit(rm, camera, poses)
        if with_history:
            rm.history_resolve()
            rm.get_history()
            rm.get_blended()
        rm.render(2)
        if with_history:
            rm.get_blended()
        got.append((outputs(rm), rm.counters(), rm.get_render_info().samples))
        rm.close()
    assert_same_outputs(got[0][0], got[1][0], sched)
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2]


# ---- (4) ----

def refused(rm, sc):
    lib = abi.load()
    plane = np.zeros(sc.y_res * sc.x_res * 4, f32)
    fp = plane.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.er_history_resolve(rm.handle) == STATE
    assert b"capture" in lib.er_last_error()
    assert lib.er_read_history(rm.handle, fp) == STATE and lib.er_read_blended(rm.handle, fp) == STATE
    info = rm.history_info()
    assert (info["captured"], info["resolved"]) == (0, 0)


def test_what_drops_a_capture_and_what_keeps_it():
    sc = scene("small")
    objects = table(sc)
    lib = abi.load()
    cam = camera_of(sc, (0.02, 0.0, -0.03))
    V = sc.vertices.reshape(-1, 3, 3)
    mats = [abi.ErMaterial.from_buffer_copy(m) for m in sc.materials]
    rm = history_manager(sc)
    try:
        refused(rm, sc)                                                                      # begun, no capture yet

        def armed():
            rm.render(1)
            rm.history_capture()
            rm.update(camera=cam)
            rm.history_resolve()
            rm.history_capture()
            assert rm.history_info()["captured"] == 1

        # what keeps it: a camera through each of the three edit entry points, a pose, samples
        armed()
        rm.update(camera=cam)
        rm.history_resolve()
        rm.history_capture()
        u = abi.ErSparseUpdate()
        u.what, u.camera = abi.UPDATE_CAMERA, cam
        abi.check(lib.er_render_update_sparse(rm.handle, C.byref(u)))
        rm.history_resolve()
        rm.history_capture()
        rm.edit(camera=cam)
        rm.history_resolve()
        rm.history_capture()
        rm.transform({1: matrix(t=(0.01, 0, 0))})
        rm.render(1)
        rm.history_resolve()
        assert rm.history_info()["moved_objects"] == 1
        rm.get_history(), rm.get_blended()
        # keep_history: capture and resolve around the call, refused where the call would drop the capture
        rm.update(camera=cam, keep_history=True)
        rm.edit(camera=cam, keep_history=True)
        rm.transform({1: matrix(t=(0.02, 0, 0))}, camera=cam, keep_history=True)
        assert rm.history_info()["resolved"] == 1
        with pytest.raises(ValueError):
            rm.update(vertices=V, keep_history=True)
        with pytest.raises(ValueError):
            rm.edit(materials=mats, keep_history=True)
        # what drops it
        drops = {
            "update": lambda: rm.update(vertices=V),
            "update_sparse": lambda: rm.update(tri_ids=np.array([3, 4], np.uint32), vertices=V[[3, 4]]),
            "edit geometry": lambda: rm.edit(vertices=V),
            "edit materials": lambda: rm.edit(materials=mats),
            "edit textures": lambda: rm.edit(textures=[None] * len(sc.textures)),
            "edit hdri": lambda: rm.edit(hdri=sc.hdri),
            "objects_set": lambda: rm.set_objects(objects),
            "topology": lambda: rm.topology(remove=np.array([sc.tri_count - 1], np.uint32)),
            "state_import": lambda: rm.state_import(rm.state_export()),
        }
        for what, call in drops.items():
            armed()
            call()
            refused(rm, sc)
            if what == "topology":                                                           # (back to the scene the other calls know)
                rm.start_rendering(sc)
                rm.set_objects(objects)
        armed()
        rm.start_rendering(sc)                                                               # er_render_begin
        refused(rm, sc)
    finally:
        rm.close()


def test_a_sharded_frame_is_refused():
    sc = scene("small")
    rm = render.RenderingManager(render.RenderParameters(max_bounces=1, rank=0, world=2))
    rm.start_rendering(sc)
    try:
        lib = abi.load()
        assert lib.er_history_capture(rm.handle, C.byref(abi.ErHistoryParams(0.0, 0.0))) == STATE
        assert b"sharded" in lib.er_last_error()
        assert lib.er_history_resolve(rm.handle) == STATE
    finally:
        rm.close()


# ---- (5) ----

def test_the_blend_after_a_small_camera_move_is_nearer_the_converged_frame():
    """cornell_textured 96 x 96: 64 spp, a small camera move, 4 spp.  The mean absolute error of the blend against 1 024 spp of the new
    frame is below that of the plain render (the parent's behaviour), both scaled by samples / n.  No margin is claimed."""
    sc = scenes.cornell_textured(96, 96)
    cam = camera_of(sc, (0.02, 0.01, 0.0), (0.0, 1.0, 0.0))
    rm = render.RenderingManager(render.RenderParameters())
    rm.start_rendering(sc)
    try:
        rm.render(64)
        rm.update(camera=cam, keep_history=True)
        rm.render(4)
        blended = rm.get_blended()[..., :3].astype(np.float64)
        plain = history.blend(rm.get_pass("beauty"), rm.read_samples(), np.zeros((96 * 96, 4), f32)).reshape(96, 96, 4)[..., :3].astype(np.float64)
        info = rm.history_info()
        rm.update(camera=cam)
        rm.render(1024)
        truth = history.blend(rm.get_pass("beauty"), rm.read_samples(), np.zeros((96 * 96, 4), f32)).reshape(96, 96, 4)[..., :3].astype(np.float64)
    finally:
        rm.close()
    e_blend, e_plain = np.abs(blended - truth).mean(), np.abs(plain - truth).mean()
    print(f"mean absolute error against 1024 spp: blend {e_blend:.5f}, plain 4 spp {e_plain:.5f}, ratio {e_blend / e_plain:.3f}; classes {info}")
    assert e_blend < e_plain
