"""The id pass (er_render_ids: the first-hit ids of n camera rays per pixel through the production traversal, csrc/er_ids.hip) and its
consumers -- er_id_matte, er_pick_rect, er_pick, er_gather_ids -- on the GPU.

(a) the planes of all three kinds against a replay composed from the oracle's entry points (oracle_rng_stream, oracle_camera_ray,
Oracle.closest_hit) and elevenrender_amd/ids.py, every word equal; (b) consistency with the feature planes, and er_pick against slot 0
of the planes and the oracle's hit record; (c) a render with all of it in between equals the render without; (d) what invalidates the
planes, and that er_pick is always current; (e) mattes; (f) box selections; (g) two ranks on one GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as orc
from elevenrender_amd import abi, ids, render, scenes, transform
from test_gpu_transform import Replay, matrix, rotation
from test_gpu_update import SCHEDULES, assert_same_outputs, manager, moved_camera, outputs

pytestmark = pytest.mark.gpu
f32 = np.float32
NONE = abi.ID_NONE
KINDS = ("triangle", "object", "material")
BUILDERS = {"host": abi.FLAG_HOST_BUILD, "device": abi.FLAG_GPU_BUILD}
INV, STATE = abi.ER_ERR_INVALID_ARG, abi.ER_ERR_STATE
N_MAX = {"small": 64, "large": 16}


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "small":
        return scenes.torture(600, 32, 24, seed=7, n_materials=8, tex_size=32, hdri_size=(64, 32), n_lights=4)
    if name == "large":          # 70 x 45: partial tiles on both edges
        return scenes.torture(4000, 70, 45, seed=7, n_materials=8, tex_size=32, hdri_size=(64, 32), n_lights=4)
    raise KeyError(name)


def table(sc):
    """triangle t is in object t % 7 unless t % 3 == 0 or t % 7 == 5: a third of the triangles are in no object, object 5 is empty"""
    t = np.arange(sc.tri_count)
    free = (t % 3 == 0) | (t % 7 == 5)
    return [t[(t % 7 == o) & ~free].astype(np.uint32) for o in range(7)]


def rays_of(sc, n):
    """origins, dirs [npx, n, 3]: ray k of pixel idx from oracle_rng_stream (five draws per ray) and oracle_camera_ray"""
    L = orc.lib()
    npx = sc.x_res * sc.y_res
    origins, dirs = np.zeros((npx, n, 3), f32), np.zeros((npx, n, 3), f32)
    for idx in range(npx):
        st, va = (C.c_uint32 * (5 * n))(), (C.c_float * (5 * n))()
        L.oracle_rng_stream(idx, 5 * n, st, va)
        for k in range(n):
            o, d = (C.c_float * 3)(), (C.c_float * 3)()
            L.oracle_camera_ray(C.byref(sc.camera), sc.x_res, sc.y_res, idx % sc.x_res, idx // sc.x_res, (C.c_float * 5)(*va[5 * k:5 * k + 5]), orc.MATH_ER, o, d)
            origins[idx, k], dirs[idx, k] = o[:], d[:]
    return origins, dirs


def traced(sc, n):
    origins, dirs = rays_of(sc, n)
    o = orc.Oracle(sc, math_mode=orc.MATH_ER, max_bounces=1)
    tri, _ = o.closest_hit(origins.reshape(-1, 3), dirs.reshape(-1, 3))
    o.close()
    return np.asarray(tri, np.int64).reshape(-1, n), origins, dirs


@functools.lru_cache(maxsize=None)
def replay(name):
    """the triangle every ray hits (-1: none), [npx, N_MAX]; its origins and directions.  Computed once per scene and shared."""
    return traced(scene(name), N_MAX[name])


def kind_ids(sc, tri, kind, objects, material_id=None):
    t = np.maximum(tri, 0)
    if kind == "triangle":
        return t.astype(np.uint32)
    if kind == "object":
        return (ids.object_of(sc.tri_count, objects) if objects is not None else np.full(sc.tri_count, NONE, np.uint32))[t]
    return np.asarray(sc.material_id if material_id is None else material_id).astype(np.uint32)[t]


@functools.lru_cache(maxsize=None)
def expected(name, n, kind, with_table=True):
    """(ids, counts) as (H, W, 4) uint32 and the overflow pixels, from the replay's first n rays and ids.py"""
    sc = scene(name)
    tri = replay(name)[0][:, :n]
    i, c, over = ids.planes(kind_ids(sc, tri, kind, table(sc) if with_table else None), tri >= 0)
    return i.reshape(sc.y_res, sc.x_res, 4), c.reshape(sc.y_res, sc.x_res, 4), over


def cut_ties(name, n, kind):
    sc = scene(name)
    tri = replay(name)[0][:, :n]
    k = kind_ids(sc, tri, kind, table(sc))
    return sum(bool(ids.tie_at_the_cut(k[p][tri[p] >= 0])) for p in range(len(tri)))


def assert_planes(rm, name, n, with_table=True, what=""):
    for kind in KINDS:
        gi, gc = rm.get_ids(kind)
        wi, wc, _ = expected(name, n, kind, with_table)
        assert gi.dtype == gc.dtype == np.uint32 and gi.shape == wi.shape
        bad = int(((gi != wi) | (gc != wc)).any(-1).sum())
        assert bad == 0, f"{what} {name} n={n} {kind}: {bad} pixels differ from the replay"


def ids_manager(sc, flags=0, rank=0, world=1, objects=True, max_bounces=1):
    rm = render.RenderingManager(render.RenderParameters(max_bounces=max_bounces, flags=flags, rank=rank, world=world))
    rm.start_rendering(sc)
    if objects:
        rm.set_objects(table(sc))
    return rm


# ---- what the replay alone says about the inputs: a degenerate scene cannot hide a failure ----

def test_the_scenes_exercise_what_the_cases_are_about():
    for name, n in (("small", 64), ("large", 16), ("large", 4)):
        tri = replay(name)[0][:, :n]
        hits = (tri >= 0).sum(1)
        over = [expected(name, n, k)[2] for k in KINDS]
        ties = [cut_ties(name, n, k) for k in KINDS]
        print(name, n, "no hit", int((hits == 0).sum()), "of", len(hits), "partly", int(((hits > 0) & (hits < n)).sum()), "overflow", over, "cut ties", ties)
        assert 0 < (hits == 0).sum() < len(hits) and ((hits > 0) & (hits < n)).any() and (hits == n).any()
        if n == 4:
            assert over == [0, 0, 0]
            c = expected(name, 4, "triangle")[1]
            tied = sum(((c[..., s] == c[..., s + 1]) & (c[..., s + 1] > 0)) for s in range(3)) > 0
            assert tied.sum() == 915                                               # tied counts: the id order decides
            assert (c[..., 1] > 0).sum() == 1470                                   # more than one triangle in a pixel
        else:
            assert all(o > 0 for o in over) and all(t > 0 for t in ties)
            # (the oracle alone, on these inputs)
            assert (int((hits == 0).sum()), over, ties) == {"small": (232, [190, 50, 78], [42, 18, 19]), "large": (905, [620, 93, 241], [416, 58, 144])}[name]
            assert name != "small" or int(((hits > 0) & (hits < n)).sum()) == 476
    objs = table(scene("large"))
    assert len(objs[5]) == 0 and sum(len(o) for o in objs) < scene("large").tri_count * 0.7
    oi = expected("large", 4, "object")[0]
    assert (oi[expected("large", 4, "object")[1] > 0] == NONE).any()               # hits on geometry in no object


# ---- (a) ----

@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name,ns", [("large", (1, 4, 16)), ("small", (64,))])
def test_planes_equal_the_replay(name, ns, builder):
    sc = scene(name)
    npx = sc.x_res * sc.y_res
    rm = ids_manager(sc, BUILDERS[builder], objects=False)
    try:
        assert rm.accel_info()["builder"] == (1 if builder == "device" else 0)
        assert rm.id_info() == dict(valid=0, samples=0, rays=0, ms=0.0, objects=0, overflow_pixels=(0, 0, 0))
        # without a table: every OBJECT id is ER_ID_NONE, its count the pixel's hits
        n0 = ns[-1]
        rm.render_ids(n0)
        assert rm.id_info()["objects"] == 0
        hits = (replay(name)[0][:, :n0] >= 0).sum(1).reshape(sc.y_res, sc.x_res)
        oi, oc = rm.get_ids("object")
        assert (oi == NONE).all() and (oc[..., 0] == hits).all() and (oc[..., 1:] == 0).all()
        assert_planes(rm, name, n0, with_table=False, what="no table")
        if name == "large":
            rm.render_ids(4)                                                        # (no overflow at n = 4)
            assert (rm.get_ids("object")[1][..., 0] == rm.get_ids("triangle")[1].sum(-1)).all()
        rm.set_objects(table(sc))
        for n in ns:
            rm.render_ids(n)
            assert_planes(rm, name, n, what=builder)
            info = rm.id_info()
            assert (info["valid"], info["samples"], info["rays"], info["objects"]) == (1, n, n * npx, 7) and info["ms"] > 0
            assert info["overflow_pixels"] == tuple(expected(name, n, k)[2] for k in KINDS), (n, info)
        if name == "large":
            rm.render_ids(0)                                                        # 0 means 4
            assert rm.id_info()["samples"] == 4
            assert_planes(rm, name, 4, what="n = 0")
    finally:
        rm.close()


# ---- (b) ----

def test_triangle_counts_are_the_feature_planes_coverage():
    sc = scene("large")
    rm = ids_manager(sc)
    try:
        rm.render_ids(4)
        rm.render_features(4)
        cov = rm.get_feature("albedo")[..., 3]
        assert (rm.get_ids("triangle")[1].sum(-1) == np.round(cov * 4).astype(np.uint32)).all()
        assert_planes(rm, "large", 4, what="after a feature pass")                 # the passes share a spill area, not planes
    finally:
        rm.close()


def test_pick_equals_slot_0_at_one_ray_and_the_oracles_hit_record():
    sc = scene("small")
    L = orc.lib()
    fp = lambda a: np.ascontiguousarray(a, f32).ctypes.data_as(C.POINTER(C.c_float))
    tri, origins, dirs = replay("small")
    V, N, T, UV = sc.vertices.reshape(-1, 9), sc.normals.reshape(-1, 9), sc.tangents.reshape(-1, 9), sc.uvs.reshape(-1, 6)
    rm = ids_manager(sc)
    try:
        rm.render_ids(1)
        rm.render_features(1)
        planes = {k: rm.get_ids(k) for k in KINDS}
        depth = rm.get_feature("depth")
        before = {k: (planes[k][0].copy(), planes[k][1].copy()) for k in KINDS}
        bits = lambda x: np.ascontiguousarray(x, f32).view(np.uint32)
        seen = set()
        for y in range(sc.y_res):
            for x in range(sc.x_res):
                p = rm.pick(x, y)
                idx = y * sc.x_res + x
                hit = int(planes["triangle"][1][y, x, 0])
                assert p["hit"] == hit == int(tri[idx, 0] >= 0)
                for k in KINDS:
                    assert p[k] == int(planes[k][0][y, x, 0]), (x, y, k)
                assert bits(p["distance"]) == bits(depth[y, x, 0]), (x, y)
                if not hit:
                    assert (p["triangle"], p["object"], p["material"]) == (NONE, NONE, NONE)
                    assert p["distance"] == 0 and (p["position"] == 0).all() and (p["uv"] == 0).all()
                    continue
                t = int(tri[idx, 0])
                rec = np.zeros(17, f32)
                assert L.oracle_tri_hit(fp(V[t]), fp(N[t]), fp(T[t]), fp(UV[t]), float(sc.tangent_sign[t]), fp(origins[idx, 0]), fp(dirs[idx, 0]), fp(rec))
                assert (bits(p["position"]) == bits(rec[0:3])).all() and (bits(p["uv"]) == bits(rec[15:17])).all(), (x, y)
                assert p["triangle"] == t and p["material"] == int(sc.material_id[t])
                seen.add(p["object"])
        assert NONE in seen and len(seen) > 3
        for k in KINDS:                                                             # the picks left the planes alone
            gi, gc = rm.get_ids(k)
            assert (gi == before[k][0]).all() and (gc == before[k][1]).all()
    finally:
        rm.close()


# ---- (c) ----

@pytest.mark.parametrize("sched", ["stream", "wavefront"])
def test_ids_mattes_selections_and_picks_leave_the_render_alone(sched):
    sc = scene("large")
    got = []
    for with_ids in (True, False):
        rm = ids_manager(sc, SCHEDULES[sched], max_bounces=4)
        if with_ids:
            rm.render_ids(4)
            rm.pick(11, 9)
        rm.render(3)
        if with_ids:
            rm.render_ids(2)                                                        # ... nor does any of it after the samples
            rm.id_matte("object", [1, 2])
            rm.pick_rect(3, 2, 40, 30, "triangle")
            rm.pick(40, 20)
        rm.render(1)
        got.append((outputs(rm), rm.counters(), rm.get_render_info().samples))
        rm.close()
    assert_same_outputs(got[0][0], got[1][0], sched)
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2] == 5


# ---- (d) ----

def refused(rm, sc):
    lib = abi.load()
    comm = (C.c_void_p * 1)()
    abi.check(lib.er_comm_create_local(1, comm))
    words, plane, n = np.zeros(sc.y_res * sc.x_res * 4, np.uint32), np.zeros(sc.y_res * sc.x_res, f32), C.c_uint32()
    up, fp = words.ctypes.data_as(C.POINTER(C.c_uint32)), plane.ctypes.data_as(C.POINTER(C.c_float))
    try:
        assert rm.id_info()["valid"] == 0
        for kind in range(abi.ID_KIND_COUNT):
            assert lib.er_read_ids(rm.handle, kind, up, up) == STATE
            assert b"er_render_ids" in lib.er_last_error()
            assert lib.er_gather_ids(rm.handle, kind, comm[0], 0) == STATE
            assert lib.er_id_matte(rm.handle, kind, up, 1, fp) == STATE
            assert lib.er_pick_rect(rm.handle, 0, 0, 1, 1, kind, up, 4, C.byref(n)) == STATE
    finally:
        lib.er_comm_destroy(comm[0])


def all_planes(rm):
    return {k: rm.get_ids(k) for k in KINDS}


def assert_same_planes(a, b, what):
    for k in KINDS:
        assert (a[k][0] == b[k][0]).all() and (a[k][1] == b[k][1]).all(), (what, k)


def test_a_transform_invalidates_the_planes_and_pick_stays_current():
    sc = scene("small")
    objects = table(sc)
    obj = 2
    rp = Replay(sc, objects)
    centre = sc.vertices.reshape(-1, 3, 3)[objects[obj]].reshape(-1, 3).mean(0)
    m = matrix(rotation((0.2, 1.0, 0.1), 0.05), t=(0.01, -0.02, 0.01), about=centre)
    rp.transform({obj: m})
    posed = rp.scene()
    # a pixel whose ray 0 hits the object before AND after the pose, from the replays of both scenes
    tri0 = replay("small")[0][:, 0]
    tri1 = traced(posed, 1)[0][:, 0]
    of = ids.object_of(sc.tri_count, objects)
    shows = lambda tri: (tri >= 0) & (of[np.maximum(tri, 0)] == obj)
    assert (tri0 != tri1).any()                                                     # the pose changes what some pixel sees
    both = np.nonzero(shows(tri0) & shows(tri1))[0]
    assert len(both) > 0
    px, py = int(both[0]) % sc.x_res, int(both[0]) // sc.x_res
    rm = ids_manager(sc)
    try:
        refused(rm, sc)                                                             # begun, no pass yet
        assert rm.pick(px, py)["object"] == obj                                     # ... which er_pick does not need
        rm.render_ids(4)
        assert_planes(rm, "small", 4, what="before")
        rm.transform({obj: m})
        refused(rm, sc)
        after = rm.pick(px, py)
        assert after["object"] == obj and after["triangle"] == int(tri1[both[0]])
        changed = np.nonzero(tri0 != tri1)[0]
        for idx in changed[:8]:                                                     # and it sees the posed scene everywhere
            p = rm.pick(int(idx) % sc.x_res, int(idx) // sc.x_res)
            assert p["triangle"] == (int(tri1[idx]) if tri1[idx] >= 0 else NONE)
        refused(rm, sc)                                                             # a pick is not a pass
        rm.render_ids(4)
        fresh = ids_manager(posed)
        try:
            fresh.render_ids(4)
            assert_same_planes(all_planes(rm), all_planes(fresh), "after the transform")
        finally:
            fresh.close()
        # er_objects_set invalidates, and the new table shows: one object of everything
        rm.set_objects([np.arange(sc.tri_count, dtype=np.uint32)])
        refused(rm, sc)
        rm.render_ids(4)
        oi, oc = rm.get_ids("object")
        assert (oi[oc > 0] == 0).all() and rm.id_info()["objects"] == 1 and rm.pick(px, py)["object"] == 0
        rm.set_objects([])                                                          # ... and none
        refused(rm, sc)
        assert rm.pick(px, py)["object"] == NONE
        # a camera update invalidates
        rm.render_ids(4)
        rm.update(camera=moved_camera(sc))
        refused(rm, sc)
    finally:
        rm.close()


def test_the_material_plane_follows_an_edit_of_material_id():
    sc = scene("large")
    new_ids = ((sc.material_id.astype(np.int64) * 3 + np.arange(sc.tri_count)) % len(sc.materials)).astype(np.int32)
    assert (new_ids != sc.material_id).any()
    rm = ids_manager(sc)
    try:
        rm.render_ids(4)
        assert_planes(rm, "large", 4, what="before")
        rm.edit(materials=sc.materials, material_id=new_ids)
        refused(rm, sc)
        rm.render_ids(4)
        tri = replay("large")[0][:, :4]
        wi, wc, _ = ids.planes(kind_ids(sc, tri, "material", None, new_ids), tri >= 0)
        gi, gc = rm.get_ids("material")
        assert (gi.reshape(-1, 4) == wi).all() and (gc.reshape(-1, 4) == wc).all()
        assert not (gi == expected("large", 4, "material")[0]).all()
        for kind in ("triangle", "object"):
            gi, gc = rm.get_ids(kind)
            assert (gi == expected("large", 4, kind)[0]).all() and (gc == expected("large", 4, kind)[1]).all()
        x, y = np.argwhere(gc[..., 0] > 0)[0][::-1]
        p = rm.pick(int(x), int(y))
        assert p["material"] == int(new_ids[p["triangle"]])
    finally:
        rm.close()


# ---- (e) ----

def test_mattes_equal_numpy_bit_for_bit():
    sc = scene("large")
    rm = ids_manager(sc)
    try:
        for n in (4, 16):
            rm.render_ids(n)
            for kind, members in (("object", [2]), ("object", [1, 3, 3, 6]), ("object", [NONE]), ("object", [NONE, 0, NONE]), ("object", [5]), ("material", [3]),
                                  ("material", [0, 7]), ("triangle", list(range(0, 4000, 2)))):
                wi, wc, _ = expected("large", n, kind)
                want = ids.matte(wi, wc, members, n)
                got = rm.id_matte(kind, members)
                assert got.dtype == f32 and (got.view(np.uint32) == want.view(np.uint32)).all(), (n, kind, members[:4])
                if members != [5]:
                    assert 0 < (got > 0).sum() < got.size and ((got > 0) & (got < 1)).any()
                else:
                    assert (got == 0).all()                                        # the empty object covers nothing
        rm.render_ids(4)                                                            # no overflow: the objects and "none" partition the coverage
        rm.render_features(4)
        total = sum(rm.id_matte("object", [o]) for o in (0, 1, 2, 3, 4, 5, 6, NONE))
        assert (total.view(np.uint32) == rm.get_feature("albedo")[..., 3].view(np.uint32)).all()
    finally:
        rm.close()


# ---- (f) ----

def misses_only_rect(name, n):
    """a rectangle of the frame in which no ray of the replay hits"""
    sc = scene(name)
    miss = ((replay(name)[0][:, :n] >= 0).sum(1) == 0).reshape(sc.y_res, sc.x_res)
    for h, w in ((3, 3), (2, 2), (1, 2), (1, 1)):
        for y in range(sc.y_res - h + 1):
            for x in range(sc.x_res - w + 1):
                if miss[y:y + h, x:x + w].all():
                    return x, y, x + w, y + h
    raise AssertionError("no pixel without a hit")


def test_box_selections_equal_numpy_unique_of_the_replay():
    sc = scene("large")
    lib = abi.load()
    rm = ids_manager(sc)
    try:
        rm.render_ids(4)
        hit_px = np.argwhere(expected("large", 4, "triangle")[1][..., 0] > 0)[0]
        rects = {"frame": (0, 0, 70, 45), "pixel": (int(hit_px[1]), int(hit_px[0]), int(hit_px[1]) + 1, int(hit_px[0]) + 1), "partial tiles": (61, 38, 70, 45),
                 "corner pixel": (69, 44, 70, 45), "across tiles": (5, 3, 29, 20), "misses": misses_only_rect("large", 4)}
        for kind in KINDS:
            wi, wc, _ = expected("large", 4, kind)
            for what, r in rects.items():
                want = ids.rect(wi, wc, *r)
                got = rm.pick_rect(*r, kind)
                assert got.dtype == np.uint32 and len(got) == len(want) and (got == want).all(), (kind, what, got[:8], want[:8])
                if what == "misses":
                    assert len(got) == 0
                if what in ("frame", "across tiles"):
                    assert len(got) > 3 and (np.diff(got.astype(np.int64)) > 0).all()
            assert rm.pick_rect(0, 0, 70, 45, "object")[-1] == NONE                 # "in no object" is selected like any other id, last
        # the sizing call, and a capacity below the count: the prefix is written, the whole count returned
        want = ids.rect(*expected("large", 4, "triangle")[:2], 0, 0, 70, 45)
        n = C.c_uint32()
        abi.check(lib.er_pick_rect(rm.handle, 0, 0, 70, 45, abi.ID_TRIANGLE, None, 0, C.byref(n)))
        assert n.value == len(want) > 20
        buf = np.full(16, 0xABCDABCD, np.uint32)
        abi.check(lib.er_pick_rect(rm.handle, 0, 0, 70, 45, abi.ID_TRIANGLE, buf.ctypes.data_as(C.POINTER(C.c_uint32)), 10, C.byref(n)))
        assert n.value == len(want) and (buf[:10] == want[:10]).all() and (buf[10:] == 0xABCDABCD).all()
        big = np.full(len(want) + 8, 0xABCDABCD, np.uint32)
        abi.check(lib.er_pick_rect(rm.handle, 0, 0, 70, 45, abi.ID_TRIANGLE, big.ctypes.data_as(C.POINTER(C.c_uint32)), len(big), C.byref(n)))
        assert n.value == len(want) and (big[:len(want)] == want).all() and (big[len(want):] == 0xABCDABCD).all()
        # refusals, on a begun scene with valid planes
        up = buf.ctypes.data_as(C.POINTER(C.c_uint32))
        for r in ((4, 0, 4, 1), (5, 0, 4, 1), (0, 4, 1, 4), (0, 0, 71, 1), (0, 0, 1, 46), (70, 0, 71, 1)):
            assert lib.er_pick_rect(rm.handle, *r, 0, up, 4, C.byref(n)) == INV, r
        assert lib.er_pick_rect(rm.handle, 0, 0, 1, 1, 3, up, 4, C.byref(n)) == INV and lib.er_pick_rect(rm.handle, 0, 0, 1, 1, 0, None, 4, C.byref(n)) == INV
        assert lib.er_id_matte(rm.handle, 0, up, 0, buf.view(f32).ctypes.data_as(C.POINTER(C.c_float))) == INV
        assert lib.er_pick(rm.handle, 70, 0, C.byref(abi.ErPick())) == INV and lib.er_pick(rm.handle, 0, 45, C.byref(abi.ErPick())) == INV
        assert lib.er_render_ids(rm.handle, 65) == INV
        assert_planes(rm, "large", 4, what="after the refusals")
    finally:
        rm.close()


# ---- (g) ----

def test_two_ranks_on_one_gpu():
    lib = abi.load()
    sc = scene("large")
    world, root = 2, 0
    comms = (C.c_void_p * world)()
    abi.check(lib.er_comm_create_local(world, comms))
    rms = [ids_manager(sc, rank=r, world=world) for r in range(world)]
    try:
        for rm in rms:
            rm.render_ids(4)
        info = [rm.id_info() for rm in rms]
        assert sum(i["rays"] for i in info) == 4 * sc.x_res * sc.y_res and all(i["rays"] > 0 for i in info)
        assert tuple(sum(i["overflow_pixels"][k] for i in info) for k in range(3)) == (0, 0, 0)
        ys, xs = np.mgrid[0:sc.y_res, 0:sc.x_res]
        for r, rm in enumerate(rms):                                                # before the gather: this rank's pixels, empty slots elsewhere
            mine = (xs // 8 + ys // 8) % world == r
            for kind in KINDS:
                gi, gc = rm.get_ids(kind)
                wi, wc, _ = expected("large", 4, kind)
                assert (gi[mine] == wi[mine]).all() and (gc[mine] == wc[mine]).all() and (gi[~mine] == NONE).all() and (gc[~mine] == 0).all()
            assert (rm.id_matte("material", [1, 2, 3])[~mine] == 0).all()          # mattes work on the planes as they lie
        for kind in range(abi.ID_KIND_COUNT):
            for r in (1, 0):
                abi.check(lib.er_gather_ids(rms[r].handle, kind, comms[r], root))
        assert_planes(rms[root], "large", 4, what="gathered")
        one = ids_manager(sc)
        try:
            one.render_ids(4)
            assert_same_planes(all_planes(rms[root]), all_planes(one), "gathered against one rank")
        finally:
            one.close()
        assert lib.er_gather_ids(rms[0].handle, 0, comms[1], root) == INV           # another rank's communicator
        # er_pick answers for any pixel, whoever owns it: rank 1 for a pixel of rank 0's first tile, and the other way round
        tri = replay("large")[0][:, 0]
        for r, rm in enumerate(rms):
            other = np.nonzero(((xs // 8 + ys // 8) % world != r).reshape(-1) & (tri >= 0))[0]
            for idx in other[:4]:
                p = rm.pick(int(idx) % sc.x_res, int(idx) // sc.x_res)
                assert p["hit"] == 1 and p["triangle"] == int(tri[idx])
    finally:
        for rm in rms:
            rm.close()
        for c in comms:
            lib.er_comm_destroy(c)
