"""er_objects_set / er_render_transform on the GPU: registered objects posed on the device from their rest copy (k_xform_scatter,
csrc/er_refit.hip; the arithmetic is csrc/er_xform.h), against the contract of include/eleven_hip.h: whatever the transform leaves
equals, byte for byte, what er_render_update_sparse leaves when given the listed objects' ids with pose(rest, m) -- elevenrender_amd/
transform.py, the numpy restatement -- as vertices, normals and tangents.

Every case begins two managers on the same scene: A gets transform(), B update(tri_ids=...) of the posed arrays.  The oracle is the
sparse path, which tests/test_gpu_update_sparse.py holds against the full update and tests/test_gpu_update.py against a fresh build.
The cases that read the LAZY host copy (a rebuild, a second er_render_begin, a sparse patch) hold A against a fresh create + begin of the
replayed arrays, where the structure too is equal byte for byte."""
import ctypes as C

import numpy as np
import pytest

from elevenrender_amd import abi, scenes, transform
from test_gpu_accel_structure import BARY, aimed_rays, raw_buffers, scene
from test_gpu_update import BLOB_INSTANCES, SCHEDULES, assert_same_outputs, manager, moved_camera, outputs, with_arrays
from test_gpu_update_sparse import assert_same_structure, tris, vmax_bits, warm

pytestmark = pytest.mark.gpu

ENTRY_BYTES, GLOBALS_BYTES = 128, 64      # csrc/er_xform.h ErXformEntry; the refit's sixteen counter words


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def matrix(L=np.eye(3), t=(0, 0, 0), about=None):
    """[L | t] as float32; with `about`, x' = L (x - about) + about + t"""
    L, t = np.asarray(L, np.float64), np.asarray(t, np.float64)
    if about is not None:
        t = t + np.asarray(about, np.float64) - L @ np.asarray(about, np.float64)
    return np.concatenate([L, t[:, None]], 1).astype(np.float32)


IDENTITY = matrix()


class Replay:
    """what the scene's arrays are after a sequence of calls, in numpy: the rest copy as set_objects saw it, and the current arrays"""

    def __init__(self, sc, objects):
        self.objects = [np.asarray(o, np.int64) for o in objects]
        self.rest = [a.reshape(-1, 3, 3).copy() for a in (sc.vertices, sc.normals, sc.tangents)]
        self.cur = [a.copy() for a in self.rest]
        self.sc = sc
        self.camera = None

    def listed(self, poses):
        """the sparse form of a transform: ids in listed order, and pose(rest, m) of each"""
        ids = np.concatenate([self.objects[o] for o in poses])
        parts = [transform.pose(m, *(r[self.objects[o]] for r in self.rest)) for o, m in poses.items()]
        return ids, [np.concatenate([p[k] for p in parts]) for k in range(3)]

    def transform(self, poses):
        ids, arrays = self.listed(poses)
        self.patch(ids, *arrays)

    def patch(self, ids, vertices, normals=None, tangents=None):
        for cur, new in zip(self.cur, (vertices, normals, tangents)):
            if new is not None:
                cur[np.asarray(ids)] = new

    def replace(self, vertices, normals=None, tangents=None):
        for k, new in enumerate((vertices, normals, tangents)):
            if new is not None:
                self.cur[k] = np.asarray(new, np.float32).reshape(-1, 3, 3).copy()

    def scene(self):
        v, n, t = (a.copy() for a in self.cur)      # (a description that later calls do not change)
        return with_arrays(self.sc, vertices=v, normals=n, tangents=t, camera=self.camera)


def pair(sc, objects, flags=0, rank=0, world=1, warm_up=True):
    A, B = manager(sc, flags, rank, world), manager(sc, flags, rank, world)
    if warm_up:
        warm(A, B, sc)
    A.set_objects(objects)
    return A, B, Replay(sc, objects)


def both(A, B, rp, poses, camera=None):
    """transform() on A, the sparse update of the posed arrays on B; the infos agree; returns the replayed description"""
    ids, (v, n, t) = rp.listed(poses)
    A.transform(poses, camera=camera)
    B.update(camera=camera, tri_ids=ids, vertices=v, normals=n, tangents=t)
    rp.transform(poses)
    if camera is not None:
        rp.camera = camera
    ta, sb = A.transform_info(), B.sparse_info()
    for k in ("path", "why_full", "dirty_nodes2", "dirty_nodes8", "moved"):
        assert ta[k] == sb[k], (k, ta, sb)
    assert ta["objects"] == len(poses) and ta["moved"] == len(ids)
    if ta["path"] != 3:
        assert ta["bytes_uploaded"] == ENTRY_BYTES * len(poses) + GLOBALS_BYTES * (2 if ta["path"] == 2 else 1), ta
        assert ta["refit_ms"] == A.update_info()["refit_ms"] > 0
    return rp.scene()


def begin_again(rm):
    """a second er_render_begin of the same scene handle, with the manager's own parameters"""
    p = rm.pars
    params = abi.ErRenderParams(p.sampleTarget, p.block_size, p.max_bounces, 0, p.rank, p.world, p.flags)
    abi.check(rm.lib.er_render_begin(rm.handle, C.byref(params)))


def assert_equals_fresh(A, sc_new, what, flags=0, samples=2):
    """A's structure and outputs against a fresh create + begin of the replayed arrays, byte for byte (A's structure is a BUILT one)"""
    fresh = manager(sc_new, flags)
    try:
        assert A.accel_info()["builder"] != 2, what
        ra, rf = raw_buffers(A.debug_read_accel()), raw_buffers(fresh.debug_read_accel())
        for k in ra:
            assert ra[k] == rf[k], f"{what}: {k} differs from a fresh begin's"
        assert_same_outputs(outputs(A), outputs(fresh), f"{what}: right after")
        for rm in (A, fresh):
            rm.render(samples)
        assert_same_outputs(outputs(A), outputs(fresh), f"{what}: after {samples} spp")
    finally:
        fresh.close()


def blob_objects(sc):
    per = sc.tri_count // BLOB_INSTANCES
    return [np.arange(i * per, (i + 1) * per) for i in range(BLOB_INSTANCES)]


def blob_onto_the_far_one(sc):
    v = tris(sc)
    per = len(v) // BLOB_INSTANCES
    delta = v[(BLOB_INSTANCES - 1) * per:].reshape(-1, 3).mean(0) - v[:per].reshape(-1, 3).mean(0)
    return {0: matrix(t=delta)}


def soup_objects(sc, sizes=(1, 63, 64, 65), seed=31, avoid_maximum=False):
    """objects of those sizes drawn as a seeded permutation of the ids: non-contiguous, and the rest of the triangles in no object"""
    perm = np.random.default_rng(seed).permutation(sc.tri_count)
    if avoid_maximum:      # (a pose of these objects can then not change the scene's largest |coordinate| by shrinking)
        a = np.abs(tris(sc)).reshape(sc.tri_count, -1).max(1)
        perm = perm[a[perm] < a.max()]
    cuts = np.cumsum((0,) + tuple(sizes))
    assert cuts[-1] <= len(perm)
    return [perm[cuts[i]:cuts[i + 1]] for i in range(len(sizes))]


def centre_of(sc, ids):
    return tris(sc)[ids].reshape(-1, 3).mean(0)


def four_poses(sc, objects, k=0):
    """a different rotation x non-uniform scale x translation for each of four objects, about its own centre"""
    axes = [(1, 2, 3), (-0.3, 0.11, 5), (7, -1, 0.01), (0, 1, 1)]
    out = {}
    for o in range(4):
        L = rotation(axes[o], 0.4 + 0.9 * o + 1.7 * k) @ np.diag([1.0 + 0.2 * o, 0.7, 1.3 - 0.1 * k])
        out[o] = matrix(L, (0.05 * o, -0.02 * (k + 1), 0.03), about=centre_of(sc, objects[o]))
    return out


# ---- 1: an object ----

def test_an_instance_translated_onto_another():
    sc = scene("blobs")
    A, B, rp = pair(sc, blob_objects(sc))
    try:
        sc_new = both(A, B, rp, blob_onto_the_far_one(sc))
        info = A.transform_info()
        print(f"blobs, instance 0 onto instance {BLOB_INSTANCES - 1}: {info}")
        assert_same_structure(A, B, sc_new, "blobs")
        assert info["calls"] == 1 and info["objects"] == 1 and info["moved"] == sc.tri_count // BLOB_INSTANCES and info["path"] in (1, 2)
        if info["path"] == 1:
            assert info["dirty_nodes8"] < A.accel_info()["node_count"]
    finally:
        A.close()
        B.close()


# ---- 2: sizes around a wave, non-contiguous ids, absolute poses ----

def test_four_objects_posed_then_two_posed_again_from_the_rest_copy():
    sc = scene("soup-257")
    objects = soup_objects(sc)
    assert [len(o) for o in objects] == [1, 63, 64, 65] and sc.tri_count - sum(len(o) for o in objects) == 64
    A, B, rp = pair(sc, objects)
    fresh = None
    try:
        sc1 = both(A, B, rp, four_poses(sc, objects))
        assert_same_structure(A, B, sc1, "four objects")
        assert A.transform_info()["moved"] == 193
        second = {k: m for k, m in four_poses(sc, objects, k=1).items() if k in (3, 1)}
        sc2 = both(A, B, rp, dict(sorted(second.items(), reverse=True)))      # (listed 3, then 1)
        assert_same_structure(A, B, sc2, "two again")
        # absolute: objects 1 and 3 are pose(rest, M2), not M2 of the first pose; 0 and 2 stay where the first call put them
        for o, m in second.items():
            want = transform.pose(m, tris(sc)[objects[o]], sc.normals.reshape(-1, 3, 3)[objects[o]], sc.tangents.reshape(-1, 3, 3)[objects[o]])
            assert tris(sc2)[objects[o]].tobytes() == want[0].tobytes()
        for o in (0, 2):
            assert tris(sc2)[objects[o]].tobytes() == tris(sc1)[objects[o]].tobytes()
        loose = np.setdiff1d(np.arange(sc.tri_count), np.concatenate(objects))
        assert tris(sc2)[loose].tobytes() == tris(sc)[loose].tobytes()
        # ... and against a fresh create + begin of the replayed arrays: bounds, lift bound and outputs (the refit keeps its topology)
        fresh = manager(sc2)
        da, df = A.debug_read_accel(), fresh.debug_read_accel()
        for k in ("lo", "hi", "lift_bound", "max_lift"):
            assert da[k].tobytes() == df[k].tobytes(), k
        assert_same_outputs(outputs(A), outputs(fresh), "right after, against a fresh begin")
        for rm in (A, B, fresh):
            rm.render(2)
        oa = outputs(A)
        assert_same_outputs(oa, outputs(B), "after 2 spp, against the sparse update")
        assert_same_outputs(oa, outputs(fresh), "after 2 spp, against a fresh begin")
    finally:
        for rm in (A, B, fresh):
            if rm is not None:
                rm.close()


# ---- 3: the largest |coordinate| ----

def test_the_object_with_the_largest_coordinate_scaled_out_and_back():
    sc = scene("soup-257")
    a = np.abs(tris(sc)).reshape(sc.tri_count, -1).max(1)
    top = int(a.argmax())
    others = np.setdiff1d(np.arange(sc.tri_count), [top])[:40]
    objects = [others[:20], np.concatenate([[top], others[20:]])]
    A, B, rp = pair(sc, objects)
    try:
        sc1 = both(A, B, rp, {1: matrix(np.eye(3) * 1.5)})
        assert vmax_bits(sc1.vertices) > vmax_bits(sc.vertices)
        info = A.transform_info()
        assert_same_structure(A, B, sc1, "outward")
        assert info["path"] == 2 and info["why_full"] == 2, info
        sc2 = both(A, B, rp, {1: IDENTITY})
        assert vmax_bits(sc2.vertices) == vmax_bits(sc.vertices) < vmax_bits(sc1.vertices)
        info = A.transform_info()
        assert_same_structure(A, B, sc2, "back inward")
        assert info["path"] == 2 and info["why_full"] == 2 and info["calls"] == 2, info
        assert tris(sc2).tobytes() == tris(sc).tobytes()      # pose(rest, identity) reproduces the vertices
    finally:
        A.close()
        B.close()


# ---- 4: no kept boxes yet ----

@pytest.mark.parametrize("case", ["soup-257", "soup-6000"])
def test_first_call_after_begin_then_the_dirty_path(case):
    sc = scene(case)
    objects = soup_objects(sc, sizes=(20, 30), avoid_maximum=True)
    A, B, rp = pair(sc, objects, warm_up=False)
    try:
        sc1 = both(A, B, rp, {0: matrix(np.eye(3) * 0.99)})
        info = A.transform_info()
        assert_same_structure(A, B, sc1, f"{case} first")
        assert info["path"] == 2 and info["why_full"] == 1 and info["calls"] == 1, info
        sc2 = both(A, B, rp, {1: matrix(np.eye(3) * 0.98), 0: matrix(np.eye(3) * 0.97)})
        assert vmax_bits(sc2.vertices) == vmax_bits(sc1.vertices)
        info = A.transform_info()
        assert_same_structure(A, B, sc2, f"{case} second")
        assert info["path"] == 1 and info["why_full"] == 0 and info["calls"] == 2 and info["moved"] == 50, info
        assert 1 <= info["dirty_nodes8"] <= A.accel_info()["node_count"]
    finally:
        A.close()
        B.close()


# ---- 5: the whole scene ----

def test_every_triangle_in_one_object_and_the_scene_rotated():
    sc = scene("soup-6000")
    ids = np.random.default_rng(5).permutation(sc.tri_count)
    A, B, rp = pair(sc, [ids])
    try:
        sc_new = both(A, B, rp, {0: matrix(rotation((1, -2, 0.5), 0.83), (0.3, 0.0, -0.1))})
        info = A.transform_info()
        print(f"soup-6000, every triangle: {info}")
        assert_same_structure(A, B, sc_new, "whole scene")
        assert info["moved"] == sc.tri_count
        if info["path"] == 1:
            assert info["dirty_nodes8"] == A.accel_info()["node_count"]
    finally:
        A.close()
        B.close()


# ---- 6: the readers of the lazy host copy ----

def tenth_apart(sc, step):
    """a tenth of the soup as one object, moved apart: the refitted tree degrades (tests/test_gpu_update_sparse.py)"""
    return {0: matrix(t=(0.4 * (step + 1),) * 3)}


def test_under_always_the_rebuild_reads_the_posed_arrays():
    sc = scene("soup-6000")
    A, B, rp = pair(sc, [np.arange(0, 600), np.arange(900, 1000)])
    try:
        for rm in (A, B):
            rm.set_update_policy(abi.REBUILD_ALWAYS)
        sc1 = both(A, B, rp, {0: tenth_apart(sc, 0)[0], 1: matrix(rotation((0, 0, 1), 0.5), about=centre_of(sc, np.arange(900, 1000)))})
        assert_same_structure(A, B, sc1, "always")
        ra, rb = A.rebuild_info(), B.rebuild_info()
        assert (ra["rebuilds"], ra["last_decision"]) == (rb["rebuilds"], rb["last_decision"]) == (1, 3)
        assert A.transform_info()["path"] == 3 and A.transform_info()["calls"] == 1
        assert_equals_fresh(A, sc1, "always")
    finally:
        A.close()
        B.close()


def test_under_auto_with_a_ratio_that_triggers():
    sc = scene("soup-6000")
    A, B, rp = pair(sc, [np.arange(0, 600)], warm_up=False)
    try:
        for rm in (A, B):
            rm.set_update_policy(abi.REBUILD_AUTO, 1.0)
        cur = None
        for step in range(2):
            cur = both(A, B, rp, tenth_apart(sc, step))
            assert_same_structure(A, B, cur, f"auto step {step}")
            ra, rb = A.rebuild_info(), B.rebuild_info()
            print(f"auto step {step}: {ra}  transform {A.transform_info()}")
            for k in ("mode", "max_cost_ratio", "rebuilds", "last_decision"):
                assert ra[k] == rb[k], (k, ra, rb)
            for k in ("cost_built", "cost_refit", "cost_after"):
                assert np.float64(ra[k]).view(np.uint64) == np.float64(rb[k]).view(np.uint64), (k, ra, rb)
        assert A.rebuild_info()["last_decision"] == 2 and A.transform_info()["path"] == 3
        assert_equals_fresh(A, cur, "auto")
    finally:
        A.close()
        B.close()


def test_a_second_begin_after_two_transforms_and_the_table_survives():
    sc = scene("soup-6000")
    objects = soup_objects(sc, sizes=(300, 65), avoid_maximum=True)
    A, B, rp = pair(sc, objects)
    try:
        both(A, B, rp, {0: matrix(rotation((1, 1, 0), 1.1) @ np.diag([0.5, 0.6, 0.4]), about=centre_of(sc, objects[0]))})
        sc2 = both(A, B, rp, {1: matrix(np.eye(3) * 0.9), 0: matrix(rotation((0, 1, 0), 0.3) * 0.8, about=centre_of(sc, objects[0]))})
        assert_same_structure(A, B, sc2, "two transforms")
        begin_again(A)
        assert_equals_fresh(A, sc2, "second begin")
        # the table belongs to the scene: the next transform poses from the same rest copy (B begins again too: its host copy is the same)
        begin_again(B)
        sc3 = both(A, B, rp, {1: matrix(np.eye(3) * 0.8)})
        assert_same_structure(A, B, sc3, "after the second begin")
        assert A.transform_info()["path"] == 2 and A.transform_info()["why_full"] == 1
    finally:
        A.close()
        B.close()


def test_a_sparse_patch_after_a_transform_then_a_second_begin():
    sc = scene("soup-6000")
    objects = soup_objects(sc, sizes=(65, 64), avoid_maximum=True)
    A, B, rp = pair(sc, objects)
    try:
        both(A, B, rp, {0: matrix(rotation((3, 1, 2), 0.7), about=centre_of(sc, objects[0]))})
        outside = int(np.setdiff1d(np.arange(sc.tri_count), np.concatenate(objects))[7])
        ids = np.concatenate([objects[0][[3, 40, 64]], [outside]])
        new = (rp.cur[0][ids] * np.float32(0.995)).astype(np.float32)
        for rm in (A, B):
            rm.update(tri_ids=ids, vertices=new)
        rp.patch(ids, new)
        assert_same_structure(A, B, rp.scene(), "sparse patch")
        begin_again(A)
        assert_equals_fresh(A, rp.scene(), "second begin after the patch")
    finally:
        A.close()
        B.close()


# ---- 7: sequences ----

@pytest.mark.parametrize("full", ["vertices only", "all three arrays"])
def test_transform_sparse_transform_full_transform(full):
    sc = scene("soup-6000")
    objects = soup_objects(sc, sizes=(65, 129), avoid_maximum=True)
    A, B, rp = pair(sc, objects)
    try:
        pose_a = matrix(rotation((1, 2, 3), 0.6) @ np.diag([0.9, 0.5, 0.7]), about=centre_of(sc, objects[0]))
        assert_same_structure(A, B, both(A, B, rp, {0: pose_a}), "transform a")
        outside = int(np.setdiff1d(np.arange(sc.tri_count), np.concatenate(objects))[11])
        ids = np.concatenate([objects[0][[0, 17, 64]], [outside]])
        new = (rp.cur[0][ids] * np.float32(0.99)).astype(np.float32)
        for rm in (A, B):
            rm.update(tri_ids=ids, vertices=new)
        rp.patch(ids, new)
        assert_same_structure(A, B, rp.scene(), "sparse update")
        assert_same_structure(A, B, both(A, B, rp, {1: matrix(np.eye(3) * 0.95, (0.01, 0.0, 0.0))}), "transform b")
        shrunk = (rp.cur[0] * np.float32(0.97)).astype(np.float32)
        arrays = dict(vertices=shrunk) if full == "vertices only" else dict(vertices=shrunk, normals=rp.cur[1][:, ::-1].copy(), tangents=rp.cur[2][:, ::-1].copy())
        for rm in (A, B):
            rm.update(**arrays)
        rp.replace(**arrays)
        assert_same_structure(A, B, rp.scene(), "full update")
        sc5 = both(A, B, rp, {0: IDENTITY})
        assert_same_structure(A, B, sc5, "transform a again")
        assert tris(sc5)[objects[0]].tobytes() == tris(sc)[objects[0]].tobytes()      # from the REST copy: the direct edits moved the pose only
        begin_again(A)
        assert_equals_fresh(A, sc5, "second begin at the end")
    finally:
        A.close()
        B.close()


# ---- 8: outputs ----

def rendered_three_ways(sc, objects, poses, flags=0, rank=0, world=1, camera=None):
    """4 spp, the call, 4 spp on A (transform) and B (sparse); 4 spp on a fresh create + begin of the replayed description"""
    A, B, rp = pair(sc, objects, flags, rank, world)
    fresh = None
    try:
        for rm in (A, B):
            rm.render(4)
        sc_new = both(A, B, rp, poses, camera=camera)
        fresh = manager(sc_new, flags, rank, world)
        oa = outputs(A)
        assert_same_outputs(oa, outputs(B), "right after, against the sparse update")
        assert_same_outputs(oa, outputs(fresh), "right after, against a fresh begin")
        for rm in (A, B, fresh):
            rm.render(4)
        oa = outputs(A)
        assert_same_outputs(oa, outputs(B), "after 4 spp, against the sparse update")
        assert_same_outputs(oa, outputs(fresh), "after 4 spp, against a fresh begin")
        assert A.counters() == B.counters() == fresh.counters()
        assert A.get_render_info().samples == B.get_render_info().samples == fresh.get_render_info().samples == 5
        assert A.light_info() == B.light_info() == fresh.light_info()
        assert A.adaptive_info() == B.adaptive_info() == fresh.adaptive_info()
        return A.transform_info(), A.light_info()
    finally:
        for rm in (A, B, fresh):
            if rm is not None:
                rm.close()


def soup_case():
    sc = scene("soup-6000")
    objects = soup_objects(sc, sizes=(65, 200), avoid_maximum=True)
    poses = {1: matrix(rotation((2, -1, 0.5), 0.9) @ np.diag([0.8, 0.6, 0.9]), about=centre_of(sc, objects[1])), 0: matrix(np.eye(3) * 0.9)}
    return sc, objects, poses


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_render_after_a_transform(schedule):
    info, _ = rendered_three_ways(*soup_case(), SCHEDULES[schedule])
    assert info["moved"] == 265


def test_render_on_rank_1_of_3_with_a_camera_in_the_same_call():
    sc, objects, poses = soup_case()
    rendered_three_ways(sc, objects, poses, rank=1, world=3, camera=moved_camera(sc))


def test_render_with_mesh_lights_and_the_emitter_inside_a_moved_object():
    sc = scenes.cornell(48, 48)
    light = np.array([11, 10])      # the light: lower and off centre, turned a little
    pose = matrix(rotation((0, 1, 0), 0.3) @ np.diag([0.8, 1.0, 0.7]), (0.3, -0.2, 0.25), about=centre_of(sc, light))
    _, lights = rendered_three_ways(sc, [light, np.array([0, 1])], {0: pose}, abi.FLAG_MESH_LIGHTS)
    assert lights["emitters"] == 2


def test_aimed_rays_at_the_moved_object():
    sc = scene("blobs")
    A, B, rp = pair(sc, blob_objects(sc))
    try:
        sc_new = both(A, B, rp, blob_onto_the_far_one(sc))
        per = sc.tri_count // BLOB_INSTANCES
        o, d, _, _ = aimed_rays(sc_new, BARY)
        o, d = o[: per * len(BARY)], d[: per * len(BARY)]      # (triangle-major: the rays aimed at instance 0, where it lies now)
        got = []
        for rm in (A, B):
            tri, _, pos, dist, _ = rm.debug_trace_rays(o, d)
            got.append((tri, pos.view(np.uint32), dist.view(np.uint32)))
        assert (got[0][0] >= 0).mean() > 0.9
        for what, a, b in zip(("triangle", "position", "distance"), got[0], got[1]):
            assert (a != b).sum() == 0, what
    finally:
        A.close()
        B.close()


# ---- 9: the upload ----

def test_bytes_uploaded_follow_the_objects_listed_not_their_size():
    sc = scene("soup-257")
    objects = soup_objects(sc, avoid_maximum=True)
    A, B, rp = pair(sc, objects)
    try:
        shrink = matrix(np.eye(3) * 0.99)
        got = {}
        for o in (0, 3):
            both(A, B, rp, {o: shrink})
            info = A.transform_info()
            assert info["moved"] == len(objects[o]) and info["path"] == 1, info
            got[o] = info["bytes_uploaded"]
        assert len(objects[0]) == 1 and len(objects[3]) == 65
        assert got[0] == got[3] == ENTRY_BYTES + GLOBALS_BYTES
        both(A, B, rp, {1: shrink, 2: shrink, 0: IDENTITY})
        assert A.transform_info()["bytes_uploaded"] == 3 * ENTRY_BYTES + GLOBALS_BYTES
    finally:
        A.close()
        B.close()


# ---- 10: refusals ----

def test_refused_transforms_leave_everything_as_it_was():
    sc = scene("soup-6000")
    objects = soup_objects(sc, sizes=(65, 64, 0))
    rm, plain, bare = manager(sc), manager(sc), manager(sc)
    try:
        for m in (rm, plain):
            m.update(vertices=sc.vertices)
        rm.set_objects(objects)
        shrink = matrix(np.eye(3) * 0.99)
        rm.transform({0: shrink})
        v, n, t = transform.pose(shrink, *(a.reshape(-1, 3, 3)[objects[0]] for a in (sc.vertices, sc.normals, sc.tangents)))
        plain.update(tri_ids=objects[0], vertices=v, normals=n, tangents=t)
        for m in (rm, plain):
            m.render(2)
        assert_same_outputs(outputs(rm), outputs(plain), "before the refusals")
        before = raw_buffers(rm.debug_read_accel()), rm.update_info(), rm.transform_info(), rm.sparse_info(), rm.accel_info(), rm.rebuild_info()

        def call(what=abi.UPDATE_GEOMETRY, poses=((0, IDENTITY),), count=None, null=False, handle=rm.handle):
            x = (abi.ErObjectTransform * max(1, len(poses)))()
            for i, (o, m) in enumerate(poses):
                x[i].object = o
                x[i].m[:] = np.asarray(m, np.float32).reshape(12).tolist()
            u = abi.ErTransformUpdate()
            u.what, u.count = what, len(poses) if count is None else count
            if not null:
                u.transforms = x
            return rm.lib.er_render_transform(handle, C.byref(u))

        nan, inf = IDENTITY.copy(), IDENTITY.copy()
        nan[2, 1], inf[0, 3] = np.nan, -np.inf
        B = np.abs(tris(sc)[objects[1]]).reshape(-1, 3).max(0).astype(np.float64)
        beyond = matrix(np.eye(3), (1e37 * (1 + 1e-6), 0, 0))
        assert not transform.bound_ok(beyond, B) and transform.bound_ok(matrix(np.eye(3), (1e37 * (1 - 1e-6), 0, 0)), np.zeros(3))
        refused = {"what 0": call(what=0), "an unknown bit": call(what=abi.UPDATE_GEOMETRY | 4), "count 0": call(count=0), "NULL transforms": call(null=True),
                   "an object index equal to the object count": call(poses=((len(objects), IDENTITY),)), "an object listed twice": call(poses=((1, IDENTITY), (0, IDENTITY), (1, IDENTITY))),
                   "a NaN": call(poses=((1, nan),)), "an infinity": call(poses=((0, IDENTITY), (1, inf))), "a mirror": call(poses=((1, matrix(np.diag([1.0, 1.0, -1.0]))),)),
                   "a singular matrix": call(poses=((1, matrix(np.diag([1.0, 0.0, 1.0]))),)), "a zero matrix": call(poses=((1, matrix(np.zeros((3, 3)))),)),
                   "beyond the overflow bound": call(poses=((1, beyond),)), "an empty object alone": call(poses=((2, IDENTITY),)),
                   "a NULL update": rm.lib.er_render_transform(rm.handle, None), "a NULL scene": call(handle=None)}
        for what, rc in refused.items():
            assert rc == abi.ER_ERR_INVALID_ARG, what
        assert call(handle=bare.handle) == abi.ER_ERR_STATE                      # begun, but no object table
        assert b"er_objects_set" in rm.lib.er_last_error()
        assert rm.lib.er_objects_set(rm.handle, 1, None, None) == abi.ER_ERR_INVALID_ARG      # a refused table leaves the old one
        after = raw_buffers(rm.debug_read_accel()), rm.update_info(), rm.transform_info(), rm.sparse_info(), rm.accel_info(), rm.rebuild_info()
        assert before == after
        assert_same_outputs(outputs(rm), outputs(plain), "right after refused transforms")
        rm.render(2)
        plain.render(2)
        assert_same_outputs(outputs(rm), outputs(plain), "a render continued after refused transforms")
        # (the table is still the old one)
        assert call(poses=((1, shrink),)) == abi.ER_OK
        assert rm.transform_info()["calls"] == 2 and rm.transform_info()["moved"] == 64
    finally:
        for m in (rm, plain, bare):
            m.close()
