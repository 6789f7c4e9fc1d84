"""er_skin_set / er_render_skin on the GPU: registered objects deformed on the device by linear-blend skinning from their rest copy
(k_skin_scatter, csrc/er_refit.hip; the arithmetic is csrc/er_skin.h), against the contract of include/eleven_hip.h: whatever the call
leaves equals, byte for byte, what er_render_update_sparse leaves when given the listed objects' ids with pose(palette, ...) --
elevenrender_amd/skin.py, the numpy restatement -- as vertices, normals and tangents.

The method is tests/test_gpu_transform.py's.  Every case begins two managers on the same scene: A gets skin(), B update(tri_ids=...) of
the posed arrays.  The cases that read the LAZY host copy (a rebuild, a second er_render_begin, a topology edit) hold A against a fresh
create + begin of the replayed arrays, where the structure too is equal byte for byte.

So that no case passes vacuously, each one asserts in numpy, BEFORE any device call (relevant(), below), that at least half of the listed
corners change a coordinate's bits under the palettes it uses, that corners with 2, 3 and 4 non-zero weights are all present, and that a
palette has a non-uniform scale (the cofactor path then differs from the linear one)."""
import ctypes as C

import numpy as np
import pytest

from elevenrender_amd import abi, scenes, skin, topology
from test_gpu_accel_structure import BARY, aimed_rays, oracle_hits, raw_buffers, scene
from test_gpu_transform import Replay, assert_equals_fresh, begin_again, centre_of, matrix, rotation, soup_objects
from test_gpu_update import SCHEDULES, assert_same_outputs, manager, moved_camera, outputs
from test_gpu_update_sparse import assert_same_structure, tris, vmax_bits, warm

pytestmark = pytest.mark.gpu

GLOBALS_BYTES = 64      # the refit's sixteen counter words


def upload_bytes(objects, bones, path):
    """include/eleven_hip.h: ErSkinInfo.bytes_uploaded = 32 x objects + 48 x bones + 64 (+ 64 on path 2)"""
    return skin.ENTRY_BYTES * objects + skin.BONE_BYTES * bones + GLOBALS_BYTES * (2 if path == 2 else 1)


def influences(size, bones, seed):
    """[size][3][4] seeded bones below `bones` and float32 weights that sum to 1 per corner, with 1, 2, 3, 4 non-zero ones in turn"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, bones, size=(size, 3, 4)).astype(np.uint16)
    w = rng.uniform(0.1, 1.0, size=(size, 3, 4))
    nonzero = (np.arange(size * 3).reshape(size, 3) % 4) + 1
    w[np.arange(4)[None, None, :] >= nonzero[:, :, None]] = 0
    w = (w / w.sum(-1, keepdims=True)).astype(np.float32)
    return b, np.minimum(w, np.float32(1))


def palette(bones, about, seed, turn=0.5, shrink_only=False):
    """[bones][3][4]: per bone a rotation x non-uniform scale about `about` and a small shift; shrink_only: scales in (0.9, 1) about the
    origin and nothing else, so that no |coordinate| grows"""
    rng = np.random.default_rng(seed)
    P = np.empty((bones, 3, 4), np.float32)
    for k in range(bones):
        if shrink_only:
            P[k] = matrix(np.diag(rng.uniform(0.9, 0.99, size=3)))
        else:
            L = rotation(rng.normal(size=3), rng.uniform(0.2, 1.0) * turn) @ np.diag(rng.uniform(0.6, 1.3, size=3))
            P[k] = matrix(L, rng.normal(size=3) * 0.03, about=about)
    return P


class SkinReplay(Replay):
    """test_gpu_transform.Replay with skins: what the scene's arrays are after a sequence of calls, in numpy"""

    def __init__(self, sc, objects, skins):
        super().__init__(sc, objects)
        self.skins = skins      # {object: (bones, weights)}

    def listed_skin(self, palettes):
        """the sparse form of a skin call: ids in listed order, and pose(palette, ...) of each object's rest rows"""
        ids = np.concatenate([self.objects[o] for o in palettes])
        parts = [skin.pose(P, *self.skins[o], *(r[self.objects[o]] for r in self.rest)) for o, P in palettes.items()]
        return ids, [np.concatenate([p[k] for p in parts]) for k in range(3)]

    def skin(self, palettes):
        ids, arrays = self.listed_skin(palettes)
        self.patch(ids, *arrays)


def relevant(sc, objects, skins, calls):
    """the three conditions of the module's docstring, for every call (a {object: palette}) of a case; numpy only"""
    rest = [a.reshape(-1, 3, 3) for a in (sc.vertices, sc.normals, sc.tangents)]
    for palettes in calls:
        moved, counts, scales = [], set(), False
        for o, P in palettes.items():
            b, w = skins[o]
            ids = np.asarray(objects[o], np.int64)
            assert skin.palette_ok(P, np.abs(rest[0][ids]).reshape(-1, 3).max(0))
            pv = skin.pose(P, b, w, *(r[ids] for r in rest))[0]
            moved.append((pv.view(np.uint32) != rest[0][ids].view(np.uint32)).any(-1).reshape(-1))
            counts |= set((w != 0).sum(-1).reshape(-1).tolist())
            s = np.linalg.svd(np.asarray(P, np.float64).reshape(-1, 3, 4)[:, :, :3], compute_uv=False)
            scales = scales or bool((s[:, 0] / s[:, 2] > 1.01).any())
        assert np.concatenate(moved).mean() >= 0.5, "fewer than half of the listed corners move"
        assert {2, 3, 4} <= counts, counts
        assert scales, "no palette with a non-uniform scale"


def pair(sc, objects, skins, flags=0, rank=0, world=1, warm_up=True):
    A, B = manager(sc, flags, rank, world), manager(sc, flags, rank, world)
    if warm_up:
        warm(A, B, sc)
    A.set_objects(objects)
    for o, (b, w) in skins.items():
        A.set_skin(o, b, w)
    assert A.skin_info()["skinned"] == len(skins)
    return A, B, SkinReplay(sc, objects, skins)


def both(A, B, rp, palettes, camera=None):
    """skin() on A, the sparse update of the posed arrays on B; the infos agree; returns the replayed description"""
    ids, (v, n, t) = rp.listed_skin(palettes)
    A.skin(palettes, camera=camera)
    B.update(camera=camera, tri_ids=ids, vertices=v, normals=n, tangents=t)
    rp.skin(palettes)
    if camera is not None:
        rp.camera = camera
    ka, sb = A.skin_info(), B.sparse_info()
    for k in ("path", "why_full", "dirty_nodes2", "dirty_nodes8", "moved"):
        assert ka[k] == sb[k], (k, ka, sb)
    bones = sum(len(P) for P in palettes.values())
    assert ka["objects"] == len(palettes) and ka["bones"] == bones and ka["moved"] == len(ids) and ka["skinned"] == len(rp.skins)
    assert ka["influence_bytes"] in (0, skin.INFLUENCE_BYTES * sum(len(rp.objects[o]) for o in rp.skins)), ka
    if ka["path"] != 3:
        assert ka["bytes_uploaded"] == upload_bytes(len(palettes), bones, ka["path"]), ka
        assert ka["refit_ms"] == A.update_info()["refit_ms"] > 0
    return rp.scene()


def close(*managers):
    for rm in managers:
        if rm is not None:
            rm.close()


def soup_case(case, sizes, bones, seed, avoid_maximum=False):
    sc = scene(case)
    objects = soup_objects(sc, sizes=sizes, seed=seed, avoid_maximum=avoid_maximum)
    skins = {o: influences(len(objects[o]), bones[o], seed + o) for o in range(len(sizes)) if bones[o]}
    return sc, objects, skins


# ---- 1: sizes around a wave, non-contiguous ids, absolute poses ----

def test_four_objects_skinned_then_two_skinned_again_from_the_rest_copy():
    bones = (1, 2, 5, 5)
    sc, objects, skins = soup_case("soup-257", (1, 63, 64, 65), bones, seed=31)
    assert [len(o) for o in objects] == [1, 63, 64, 65]
    first = {o: palette(bones[o], centre_of(sc, objects[o]), 40 + o) for o in range(4)}
    second = {o: palette(bones[o], centre_of(sc, objects[o]), 50 + o, turn=1.5) for o in (3, 1)}      # (listed 3, then 1)
    relevant(sc, objects, skins, [first, second])
    A, B, rp = pair(sc, objects, skins)
    fresh = None
    try:
        sc1 = both(A, B, rp, first)
        assert_same_structure(A, B, sc1, "four objects")
        assert A.skin_info()["moved"] == 193 and A.skin_info()["bones"] == 13
        sc2 = both(A, B, rp, second)
        assert_same_structure(A, B, sc2, "two again")
        # absolute: objects 1 and 3 are pose(second palette) of the REST rows, not of the first pose; 0 and 2 stay where the first call put them
        rest = [a.reshape(-1, 3, 3) for a in (sc.vertices, sc.normals, sc.tangents)]
        for o, P in second.items():
            want = skin.pose(P, *skins[o], *(r[objects[o]] for r in rest))
            assert tris(sc2)[objects[o]].tobytes() == want[0].tobytes()
            composed = skin.pose(P, *skins[o], tris(sc1)[objects[o]], rest[1][objects[o]], rest[2][objects[o]])[0]
            assert tris(sc2)[objects[o]].tobytes() != composed.tobytes()
        for o in (0, 2):
            assert tris(sc2)[objects[o]].tobytes() == tris(sc1)[objects[o]].tobytes()
        loose = np.setdiff1d(np.arange(sc.tri_count), np.concatenate(objects))
        assert tris(sc2)[loose].tobytes() == tris(sc)[loose].tobytes()
        fresh = manager(sc2)
        da, df = A.debug_read_accel(), fresh.debug_read_accel()
        for k in ("lo", "hi", "lift_bound", "max_lift"):
            assert da[k].tobytes() == df[k].tobytes(), k
        for rm in (A, B, fresh):
            rm.render(2)
        oa = outputs(A)
        assert_same_outputs(oa, outputs(B), "after 2 spp, against the sparse update")
        assert_same_outputs(oa, outputs(fresh), "after 2 spp, against a fresh begin")
    finally:
        close(A, B, fresh)


# ---- 2: more than one block ----

def test_every_triangle_of_soup_257_in_one_skinned_object():
    sc = scene("soup-257")
    objects = [np.random.default_rng(5).permutation(sc.tri_count)]
    skins = {0: influences(257, 7, 3)}
    P = {0: palette(7, centre_of(sc, objects[0]), 8)}
    relevant(sc, objects, skins, [P])
    A, B, rp = pair(sc, objects, skins)
    try:
        sc1 = both(A, B, rp, P)
        assert_same_structure(A, B, sc1, "soup-257 whole")
        assert A.skin_info()["moved"] == 257 > 256
    finally:
        close(A, B)


# ---- 3: the paths ----

def test_first_call_after_begin_then_the_dirty_path_then_the_maximum_shrinks():
    sc = scene("soup-6000")
    top = int(np.abs(tris(sc)).reshape(sc.tri_count, -1).max(1).argmax())
    objects = soup_objects(sc, sizes=(20, 30, 40), avoid_maximum=True)
    objects[2] = np.concatenate([[top], objects[2][1:]])      # the third object holds the scene's largest |coordinate|
    bones = (3, 4, 3)
    skins = {o: influences(len(objects[o]), bones[o], 60 + o) for o in range(3)}
    calls = [{0: palette(3, None, 1, shrink_only=True)}, {1: palette(4, None, 2, shrink_only=True), 0: palette(3, None, 3, shrink_only=True)},
             {2: palette(3, None, 4, shrink_only=True)}]
    relevant(sc, objects, skins, calls)
    A, B, rp = pair(sc, objects, skins, warm_up=False)
    try:
        sc1 = both(A, B, rp, calls[0])
        info = A.skin_info()
        assert_same_structure(A, B, sc1, "first")
        assert info["path"] == 2 and info["why_full"] == 1 and info["calls"] == 1, info
        assert info["influence_bytes"] == skin.INFLUENCE_BYTES * 90, info      # the first call after er_skin_set uploads them
        assert vmax_bits(sc1.vertices) == vmax_bits(sc.vertices)
        sc2 = both(A, B, rp, calls[1])
        assert vmax_bits(sc2.vertices) == vmax_bits(sc.vertices)
        info = A.skin_info()
        assert_same_structure(A, B, sc2, "second")
        assert info["path"] == 1 and info["why_full"] == 0 and info["calls"] == 2 and info["moved"] == 50 and info["influence_bytes"] == 0, info
        assert 1 <= info["dirty_nodes8"] <= A.accel_info()["node_count"]
        sc3 = both(A, B, rp, calls[2])
        assert vmax_bits(sc3.vertices) < vmax_bits(sc.vertices)
        info = A.skin_info()
        assert_same_structure(A, B, sc3, "the maximum shrinks")
        assert info["path"] == 2 and info["why_full"] == 2 and info["calls"] == 3, info
    finally:
        close(A, B)


# ---- 4: matrix and palette poses of one object, and a sparse patch between them ----

def test_transform_skin_transform_on_one_object_with_a_sparse_patch_between():
    sc, objects, skins = soup_case("soup-6000", (65, 129), (4, 6), seed=31, avoid_maximum=True)
    P = {0: palette(4, centre_of(sc, objects[0]), 11)}
    relevant(sc, objects, skins, [P])
    A, B, rp = pair(sc, objects, skins)
    try:
        def by_matrix(m, what):
            ids, (v, n, t) = rp.listed({0: m})
            A.transform({0: m})
            B.update(tri_ids=ids, vertices=v, normals=n, tangents=t)
            rp.transform({0: m})
            assert_same_structure(A, B, rp.scene(), what)

        by_matrix(matrix(rotation((1, 2, 3), 0.6) @ np.diag([0.9, 0.5, 0.7]), about=centre_of(sc, objects[0])), "transform a")
        assert_same_structure(A, B, both(A, B, rp, P), "skin")
        outside = int(np.setdiff1d(np.arange(sc.tri_count), np.concatenate(objects))[11])
        ids = np.concatenate([objects[0][[0, 17, 64]], [outside]])      # the lazy copy is read: the patch lands on the SKINNED pose
        new = (rp.cur[0][ids] * np.float32(0.99)).astype(np.float32)
        for rm in (A, B):
            rm.update(tri_ids=ids, vertices=new)
        rp.patch(ids, new)
        assert_same_structure(A, B, rp.scene(), "sparse patch")
        by_matrix(matrix(np.eye(3) * 0.95, (0.01, 0.0, 0.0)), "transform b")
        sc5 = both(A, B, rp, P)
        assert_same_structure(A, B, sc5, "skin again")
        assert tris(sc5)[objects[0]].tobytes() == skin.pose(P[0], *skins[0], *(a.reshape(-1, 3, 3)[objects[0]] for a in (sc.vertices, sc.normals, sc.tangents)))[0].tobytes()
        begin_again(A)
        assert_equals_fresh(A, sc5, "second begin at the end")
    finally:
        close(A, B)


# ---- 5: the readers of the lazy host copy ----

def lazy_case():
    sc = scene("soup-6000")
    objects = [np.arange(0, 600), np.arange(900, 1000)]
    skins = {0: influences(600, 6, 21), 1: influences(100, 3, 22)}
    return sc, objects, skins


def apart(sc, objects, step):
    """object 0 deformed and moved apart, further with every step: the refitted tree degrades"""
    P = palette(6, centre_of(sc, objects[0]), 30 + step)
    P[:, :, 3] += np.float32(0.4 * (step + 1))
    return {0: P}


def test_under_always_the_rebuild_reads_the_skinned_arrays():
    sc, objects, skins = lazy_case()
    P = {**apart(sc, objects, 0), 1: palette(3, centre_of(sc, objects[1]), 9)}
    relevant(sc, objects, skins, [P])
    A, B, rp = pair(sc, objects, skins)
    try:
        for rm in (A, B):
            rm.set_update_policy(abi.REBUILD_ALWAYS)
        sc1 = both(A, B, rp, P)
        assert_same_structure(A, B, sc1, "always")
        ra, rb = A.rebuild_info(), B.rebuild_info()
        assert (ra["rebuilds"], ra["last_decision"]) == (rb["rebuilds"], rb["last_decision"]) == (1, 3)
        assert A.skin_info()["path"] == 3 and A.skin_info()["calls"] == 1
        assert_equals_fresh(A, sc1, "always")
    finally:
        close(A, B)


def test_under_auto_with_a_ratio_that_triggers():
    sc, objects, skins = lazy_case()
    calls = [apart(sc, objects, step) for step in range(2)]
    relevant(sc, objects, skins, calls)
    A, B, rp = pair(sc, objects, skins, warm_up=False)
    try:
        for rm in (A, B):
            rm.set_update_policy(abi.REBUILD_AUTO, 1.0)
        cur = None
        for step, P in enumerate(calls):
            cur = both(A, B, rp, P)
            assert_same_structure(A, B, cur, f"auto step {step}")
            ra, rb = A.rebuild_info(), B.rebuild_info()
            print(f"auto step {step}: {ra}  skin {A.skin_info()}")
            for k in ("mode", "max_cost_ratio", "rebuilds", "last_decision"):
                assert ra[k] == rb[k], (k, ra, rb)
            for k in ("cost_built", "cost_refit", "cost_after"):
                assert np.float64(ra[k]).view(np.uint64) == np.float64(rb[k]).view(np.uint64), (k, ra, rb)
        assert A.rebuild_info()["last_decision"] == 2 and A.skin_info()["path"] == 3
        assert_equals_fresh(A, cur, "auto")
    finally:
        close(A, B)


def test_a_second_begin_after_two_skins_and_the_skins_survive():
    sc, objects, skins = soup_case("soup-6000", (300, 65), (5, 2), seed=31, avoid_maximum=True)
    calls = [{0: palette(5, centre_of(sc, objects[0]), 1)}, {1: palette(2, centre_of(sc, objects[1]), 2), 0: palette(5, centre_of(sc, objects[0]), 3)},
             {1: palette(2, centre_of(sc, objects[1]), 4)}]
    relevant(sc, objects, skins, calls)
    A, B, rp = pair(sc, objects, skins)
    try:
        both(A, B, rp, calls[0])
        sc2 = both(A, B, rp, calls[1])
        assert_same_structure(A, B, sc2, "two skins")
        begin_again(A)
        assert_equals_fresh(A, sc2, "second begin")
        # table and skins belong to the scene: the next call poses from the same rest copy with the same influences, uploaded again
        begin_again(B)
        sc3 = both(A, B, rp, calls[2])
        assert_same_structure(A, B, sc3, "after the second begin")
        info = A.skin_info()
        assert info["path"] == 2 and info["why_full"] == 1 and info["skinned"] == 2 and info["influence_bytes"] == skin.INFLUENCE_BYTES * 365, info
    finally:
        close(A, B)


def test_a_topology_edit_reads_the_skinned_arrays_and_drops_the_skins():
    sc, objects, skins = soup_case("soup-257", (1, 63, 64, 65), (1, 2, 5, 5), seed=31)
    P = {o: palette((1, 2, 5, 5)[o], centre_of(sc, objects[o]), 70 + o) for o in (3, 2, 0)}
    relevant(sc, objects, skins, [P])
    A, B, rp = pair(sc, objects, skins)
    try:
        sc1 = both(A, B, rp, P)
        gone = np.concatenate([objects[3][:5], objects[1][:2]])
        A.topology(remove=gone)
        assert A.skin_info()["skinned"] == 0 and A.skin_info()["calls"] == 1
        assert_equals_fresh(A, topology.apply(sc1, remove=gone), "topology")
        one = (abi.ErSkinPose * 1)()
        keep = np.ascontiguousarray(P[3].reshape(-1, 12))
        one[0].object, one[0].bone_count, one[0].palette = 3, 5, keep.ctypes.data_as(C.POINTER(C.c_float))
        u = abi.ErSkinUpdate()
        u.what, u.count, u.poses = abi.UPDATE_GEOMETRY, 1, one
        assert A.lib.er_render_skin(A.handle, C.byref(u)) == abi.ER_ERR_STATE      # the table survived renumbered, the skins did not
        assert b"no skin" in A.lib.er_last_error()
    finally:
        close(A, B)


# ---- 6: outputs ----

def rendered_three_ways(sc, objects, skins, P, flags=0, rank=0, world=1, camera=None):
    """4 spp, the call, 4 spp on A (skin) and B (sparse); 4 spp on a fresh create + begin of the replayed description"""
    relevant(sc, objects, skins, [P])
    A, B, rp = pair(sc, objects, skins, flags, rank, world)
    fresh = None
    try:
        for rm in (A, B):
            rm.render(4)
        sc_new = both(A, B, rp, P, camera=camera)
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
        return A.skin_info(), A.light_info()
    finally:
        close(A, B, fresh)


def render_case():
    sc, objects, skins = soup_case("soup-6000", (65, 200), (3, 8), seed=31, avoid_maximum=True)
    P = {1: palette(8, centre_of(sc, objects[1]), 5), 0: palette(3, centre_of(sc, objects[0]), 6)}
    return sc, objects, skins, P


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_render_after_a_skin(schedule):
    info, _ = rendered_three_ways(*render_case(), SCHEDULES[schedule])
    assert info["moved"] == 265 and info["bones"] == 11


def test_render_on_rank_1_of_3_with_a_camera_in_the_same_call():
    sc, objects, skins, P = render_case()
    rendered_three_ways(sc, objects, skins, P, rank=1, world=3, camera=moved_camera(sc))


def test_render_with_mesh_lights_and_the_emitter_inside_the_skinned_object():
    sc = scenes.cornell(48, 48)
    objects = [np.array([11, 10]), np.array([0, 1])]      # the light, and a wall
    skins = {0: influences(2, 3, 17)}
    P = palette(3, centre_of(sc, objects[0]), 18, turn=0.4)
    P[:, :, 3] += np.array([0.3, -0.2, 0.25], np.float32)      # lower and off centre
    _, lights = rendered_three_ways(sc, objects, skins, {0: P}, abi.FLAG_MESH_LIGHTS)
    assert lights["emitters"] == 2


def test_aimed_rays_at_the_skinned_object_return_the_oracles_answers(oracle_mod):
    sc, objects, skins, P = render_case()
    relevant(sc, objects, skins, [P])
    rp = SkinReplay(sc, objects, skins)
    rp.skin(P)
    sc_new = rp.scene()
    o, d, own, _ = aimed_rays(sc_new, BARY)
    at = np.isin(own, np.concatenate(objects))      # the rays aimed at the skinned objects, where they lie now
    o, d, own = np.ascontiguousarray(o[at]), np.ascontiguousarray(d[at]), own[at]
    orc = oracle_mod.Oracle(sc_new, math_mode=oracle_mod.MATH_ER, max_bounces=4, threads=16)
    otri, opos = oracle_hits(orc, o, d)
    orc.close()
    assert (otri == own).mean() > 0.9
    A = manager(sc)
    try:
        A.set_objects(objects)
        for k, (b, w) in skins.items():
            A.set_skin(k, b, w)
        A.skin(P)
        tri, _, pos, _, _ = A.debug_trace_rays(o, d)
        assert (tri != otri).sum() == 0
        assert (pos.view(np.uint32) != opos.view(np.uint32)).sum() == 0
    finally:
        close(A)


# ---- 7: the upload ----

def test_bytes_uploaded_follow_the_objects_and_bones_listed_not_their_size():
    sc, objects, skins = soup_case("soup-257", (1, 63, 64, 65), (5, 2, 5, 5), seed=31, avoid_maximum=True)
    assert len(objects[0]) == 1 and len(objects[2]) == 64      # the same bone count drives an object 64 x larger
    shrink = {o: palette(b, None, 90 + o, shrink_only=True) for o, b in enumerate((5, 2, 5, 5))}
    calls = [{2: shrink[2]}, {0: shrink[0], 2: shrink[2]}, {1: shrink[1], 2: shrink[2], 3: shrink[3]}]
    relevant(sc, objects, skins, calls)
    A, B, rp = pair(sc, objects, skins)
    try:
        got = {}
        both(A, B, rp, calls[0])
        assert A.skin_info()["influence_bytes"] == skin.INFLUENCE_BYTES * 193
        for o in (0, 2):
            ids, (v, n, t) = rp.listed_skin({o: shrink[o]})
            A.skin({o: shrink[o]})
            B.update(tri_ids=ids, vertices=v, normals=n, tangents=t)
            rp.skin({o: shrink[o]})
            info = A.skin_info()
            assert info["moved"] == len(objects[o]) and info["path"] == 1 and info["influence_bytes"] == 0, info
            got[o] = info["bytes_uploaded"]
        assert got[0] == got[2] == 32 + 48 * 5 + 64
        both(A, B, rp, calls[2])
        info = A.skin_info()
        assert info["bytes_uploaded"] == 3 * 32 + 48 * 12 + 64 == upload_bytes(3, 12, 1) and info["path"] == 1, info
        assert_same_structure(A, B, rp.scene(), "after the accounting")
    finally:
        close(A, B)


# ---- 8: refusals ----

def test_refused_skins_leave_everything_as_it_was():
    sc = scene("soup-6000")
    objects = soup_objects(sc, sizes=(65, 64, 30, 0))
    skins = {0: influences(65, 4, 1), 1: influences(64, 3, 2)}      # object 2 has no skin, object 3 no triangle
    good = {0: palette(4, None, 7, shrink_only=True)}
    relevant(sc, objects, skins, [good])
    rm, plain, bare = manager(sc), manager(sc), manager(sc)
    try:
        for m in (rm, plain):
            m.update(vertices=sc.vertices)
        rm.set_objects(objects)
        for o, (b, w) in skins.items():
            rm.set_skin(o, b, w)
        rm.skin(good)
        v, n, t = skin.pose(good[0], *skins[0], *(a.reshape(-1, 3, 3)[objects[0]] for a in (sc.vertices, sc.normals, sc.tangents)))
        plain.update(tri_ids=objects[0], vertices=v, normals=n, tangents=t)
        for m in (rm, plain):
            m.render(2)
        assert_same_outputs(outputs(rm), outputs(plain), "before the refusals")
        state = lambda: (raw_buffers(rm.debug_read_accel()), rm.update_info(), rm.skin_info(), rm.transform_info(), rm.sparse_info(), rm.accel_info(), rm.rebuild_info())
        before = state()
        I4, I3 = np.tile(np.eye(3, 4, dtype=np.float32), (4, 1, 1)), np.tile(np.eye(3, 4, dtype=np.float32), (3, 1, 1))

        def call(what=abi.UPDATE_GEOMETRY, poses=((0, I4),), count=None, null=False, handle=rm.handle, bone_count=None, no_palette=False):
            x = (abi.ErSkinPose * max(1, len(poses)))()
            keep = []
            for i, (o, P) in enumerate(poses):
                keep.append(np.ascontiguousarray(P, np.float32).reshape(-1, 12))
                x[i].object, x[i].bone_count = o, len(keep[-1]) if bone_count is None else bone_count
                if not no_palette:
                    x[i].palette = keep[-1].ctypes.data_as(C.POINTER(C.c_float))
            u = abi.ErSkinUpdate()
            u.what, u.count = what, len(poses) if count is None else count
            if not null:
                u.poses = x
            return rm.lib.er_render_skin(handle, C.byref(u))

        def bone(P, k, m):
            P = P.copy()
            P[k] = m
            return P

        nan, inf = np.eye(3, 4, dtype=np.float32), np.eye(3, 4, dtype=np.float32)
        nan[2, 1], inf[0, 3] = np.nan, -np.inf
        beyond = matrix(np.eye(3), (1e37 * (1 + 1e-6), 0, 0))
        large = matrix(np.diag([np.nextafter(np.float32(skin.MAX_LINEAR), np.float32(1e30)), 1.0, 1.0]))
        refused = {"what 0": call(what=0), "an unknown bit": call(what=abi.UPDATE_GEOMETRY | 4), "count 0": call(count=0), "NULL poses": call(null=True),
                   "an object index equal to the object count": call(poses=((len(objects), I4),)), "an object listed twice": call(poses=((1, I3), (0, I4), (1, I3))),
                   "a bone_count different from the skin's": call(poses=((1, I4),)), "a NULL palette": call(no_palette=True),
                   "a NaN in the last bone": call(poses=((1, bone(I3, 2, nan)),)), "an infinity": call(poses=((0, I4), (1, bone(I3, 0, inf)))),
                   "a mirror": call(poses=((1, bone(I3, 1, matrix(np.diag([1.0, 1.0, -1.0])))),)), "a singular bone": call(poses=((1, bone(I3, 1, matrix(np.diag([1.0, 0.0, 1.0])))),)),
                   "beyond the overflow bound": call(poses=((1, bone(I3, 2, beyond)),)), "a linear entry beyond the bound": call(poses=((1, bone(I3, 0, large)),)),
                   "a NULL update": rm.lib.er_render_skin(rm.handle, None), "a NULL scene": call(handle=None)}
        for what, rc in refused.items():
            assert rc == abi.ER_ERR_INVALID_ARG, what
        assert call(poses=((0, I4), (2, I3))) == abi.ER_ERR_STATE                 # an object without a skin
        assert b"er_skin_set" in rm.lib.er_last_error()
        assert call(handle=bare.handle) == abi.ER_ERR_STATE                       # begun, but no object table
        assert state() == before
        assert_same_outputs(outputs(rm), outputs(plain), "right after refused skins")
        rm.render(2)
        plain.render(2)
        assert_same_outputs(outputs(rm), outputs(plain), "a render continued after refused skins")
        # (the skins are still the old ones; a linear entry AT the bound passes)
        at = matrix(np.diag([skin.MAX_LINEAR, 1.0, 1.0]) * 1.0)
        assert skin.palette_ok(bone(I3, 0, at), np.abs(tris(sc)[objects[1]]).reshape(-1, 3).max(0))
        assert call(poses=((1, bone(I3, 0, at)),)) == abi.ER_OK
        assert rm.skin_info()["calls"] == 2 and rm.skin_info()["moved"] == 64 and rm.skin_info()["skinned"] == 2
    finally:
        close(rm, plain, bare)
