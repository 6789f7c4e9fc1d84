"""er_render_update_sparse on the GPU: listed triangles moved, only their ancestors refitted (csrc/er_refit.hip), against the contract of
include/eleven_hip.h: whatever the sparse call leaves equals, byte for byte, what er_render_update with the complete edited arrays leaves.

Every case begins two managers on the same scene: A gets the sparse update, B the full update() of the complete arrays.  The oracle is
the full path, which tests/test_gpu_update.py holds against a fresh build; nothing new has to be trusted."""
import ctypes as C

import numpy as np
import pytest

import accel_check
from elevenrender_amd import abi, scenes
from test_gpu_accel_structure import BARY, aimed_rays, raw_buffers, scene
from test_gpu_update import BLOB_INSTANCES, SCHEDULES, assert_same_outputs, edit_J, edit_M, manager, moved_camera, outputs, with_arrays

pytestmark = pytest.mark.gpu

SCENES = ["soup-3", "soup-257", "soup-6000", "blobs", "torture", "same-centroid", "duplicates", "flat-grid"]


def tris(sc):
    return sc.vertices.reshape(-1, 3, 3)


def vmax_bits(v):
    return np.abs(np.asarray(v, np.float32)).max().view(np.uint32)


def patched(sc, ids, vertices, normals=None):
    """the scene description with the listed triangles replaced: what the full update and a fresh create are given"""
    v = tris(sc).copy()
    v[ids] = vertices
    nn = None
    if normals is not None:
        nn = sc.normals.reshape(-1, 3, 3).copy()
        nn[ids] = normals
    return with_arrays(sc, vertices=v, normals=nn)


def both(A, B, sc, ids, vertices, normals=None, camera=None):
    """the sparse update on A, the full update of the same edit on B; returns the edited description"""
    ids = np.asarray(ids)
    sc_new = patched(sc, ids, vertices, normals)
    begun = A.accel_info()["upload_ms"]
    A.update(camera=camera, tri_ids=ids, vertices=vertices, normals=normals)
    if A.accel_info()["builder"] == 2:      # (a refit leaves the begin's own figure alone, as the full update does; a rebuild measures again)
        assert A.accel_info()["upload_ms"] == begun
    B.update(camera=camera, vertices=sc_new.vertices, normals=None if normals is None else sc_new.normals)
    return sc_new


def same_info(a, b):
    """ErAccelInfo field for field except build_ms -- and upload_ms, the wall time of each manager's OWN er_render_begin (or rebuild), which
    two managers cannot share; both() holds it against the same manager's value before the call instead"""
    timings = ("build_ms", "upload_ms")
    return {k: v for k, v in a.items() if k not in timings} == {k: v for k, v in b.items() if k not in timings}


def assert_same_structure(A, B, sc_new, what):
    da, db = A.debug_read_accel(), B.debug_read_accel()
    ra, rb = raw_buffers(da), raw_buffers(db)
    for k in ra:
        assert ra[k] == rb[k], f"{what}: {k} differs from the full update's"
    for k in ("lo", "hi", "lift_bound", "max_lift"):
        assert da[k].tobytes() == db[k].tobytes(), (what, k, da[k], db[k])
    ia, ib = A.accel_info(), B.accel_info()
    assert same_info(ia, ib), (what, sorted(ia.items()), sorted(ib.items()))
    ua, ub = A.update_info(), B.update_info()
    assert (ua["updates"], ua["refits"]) == (ub["updates"], ub["refits"]), (what, ua, ub)
    rep = accel_check.check(sc_new, da, accel_depth=ia["max_depth"])
    assert rep.ok, rep.message()
    return da


def warm(A, B, sc):
    """a full update of the unchanged arrays on both: the refit leaves the kept boxes"""
    for rm in (A, B):
        rm.update(vertices=sc.vertices)


def pair(sc, flags=0, rank=0, world=1, warm_up=True):
    A, B = manager(sc, flags, rank, world), manager(sc, flags, rank, world)
    if warm_up:
        warm(A, B, sc)
    return A, B


def inner_triangle(sc):
    """the triangle whose largest |coordinate| is smallest, nudged by 0.1 of its size towards the origin: well inside the bounds, and
    (checked) the scene's largest |coordinate| keeps its bits"""
    v = tris(sc)
    t = int(np.abs(v).reshape(len(v), -1).max(1).argmin())
    size = np.float32((v[t].max(0) - v[t].min(0)).max())
    new = (v[t] - np.float32(0.1) * size * np.sign(v[t].reshape(-1, 3).mean(0)).astype(np.float32)).astype(np.float32)
    assert vmax_bits(patched(sc, [t], new[None]).vertices) == vmax_bits(sc.vertices)
    return t, new


def padded_bounds(v):
    """the scene bounds as the builders compute them (csrc/er_build_dev.h prim_padded_box), in numpy float32"""
    v = np.asarray(v, np.float32).reshape(-1, 3, 3)
    pad_abs = np.abs(v).max() * np.float32(1e-6)
    lo, hi = v.min(1), v.max(1)
    pad = np.maximum(np.maximum(np.abs(lo), np.abs(hi)) * np.float32(4e-7) + np.float32(1e-37), pad_abs)
    bl, bh = lo - pad, hi + pad
    bl = np.where(bl.astype(np.float64) > lo.astype(np.float64) - pad.astype(np.float64), np.nextafter(bl, np.float32(-np.inf)), bl)
    bh = np.where(bh.astype(np.float64) < hi.astype(np.float64) + pad.astype(np.float64), np.nextafter(bh, np.float32(np.inf)), bh)
    return bl.min(0).astype(np.float32), bh.max(0).astype(np.float32)


# ---- 1: inside ----

@pytest.mark.parametrize("case", SCENES)
def test_one_triangle_inside_rewrites_only_its_ancestors(case):
    sc = scene(case)
    A, B = pair(sc)
    try:
        t, new = inner_triangle(sc)
        sc_new = both(A, B, sc, [t], new[None])
        info, acc = A.sparse_info(), A.accel_info()
        print(f"{case}: {info}  wide nodes {acc['node_count']}, max_depth {acc['max_depth']}")
        assert_same_structure(A, B, sc_new, case)
        assert info["calls"] == 1 and info["path"] == 1 and info["why_full"] == 0 and info["moved"] == 1
        assert 1 <= info["dirty_nodes8"] <= acc["max_depth"] + 1
        if acc["node_count"] > 1:
            assert info["dirty_nodes8"] < acc["node_count"]
        assert info["bytes_uploaded"] <= 3 * 36 + 4 + 64
        assert info["refit_ms"] == A.update_info()["refit_ms"] > 0
    finally:
        A.close()
        B.close()


# ---- 2, 3: the largest |coordinate| changes ----

@pytest.mark.parametrize("case", SCENES)
def test_maximum_up_takes_the_whole_refit(case):
    sc = scene(case)
    A, B = pair(sc)
    try:
        v = tris(sc)
        far = np.float32(3.0) * np.abs(v).max()
        new = (v[0] - v[0].reshape(-1, 3).mean(0) + far).astype(np.float32)
        sc_new = both(A, B, sc, [0], new[None])
        info = A.sparse_info()
        assert_same_structure(A, B, sc_new, case)
        assert info["path"] == 2 and info["why_full"] == 2, info
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("case", SCENES)
def test_maximum_down_takes_the_whole_refit(case):
    sc = scene(case)
    A, B = pair(sc)
    try:
        v = tris(sc)
        a = np.abs(v).reshape(len(v), -1).max(1)
        assert a[int(np.abs(v).argmax()) // 9] == a.max()
        ids = np.flatnonzero(a == a.max())      # the triangle that holds the maximum (every copy of it, in a scene of duplicates)
        centre = v.reshape(-1, 3).mean(0)
        own = v[ids].reshape(len(ids), -1, 3).mean(1)[:, None, :]
        new = (v[ids] - own + centre).astype(np.float32)
        if vmax_bits(patched(sc, ids, new).vertices) >= vmax_bits(sc.vertices):
            # (flat-grid, duplicates: the centroid lies as far out as the maximum itself -- halfway from there to the origin)
            new = (v[ids] - own + np.float32(0.5) * centre).astype(np.float32)
        sc_new = both(A, B, sc, ids, new)
        assert vmax_bits(sc_new.vertices) < vmax_bits(sc.vertices)
        info = A.sparse_info()
        dump = assert_same_structure(A, B, sc_new, case)
        assert info["path"] == 2 and info["why_full"] == 2, info
        if case == "soup-3":
            lo, hi = padded_bounds(sc_new.vertices)
            assert dump["lo"].tobytes() == lo.tobytes() and dump["hi"].tobytes() == hi.tobytes(), (dump["lo"], lo, dump["hi"], hi)
    finally:
        A.close()
        B.close()


# ---- 4: no kept boxes yet ----

@pytest.mark.parametrize("case", ["soup-257", "soup-6000", "blobs"])
def test_first_call_after_begin_then_the_dirty_path(case):
    sc = scene(case)
    A, B = pair(sc, warm_up=False)
    try:
        t, new = inner_triangle(sc)
        sc1 = both(A, B, sc, [t], new[None])
        info = A.sparse_info()
        assert_same_structure(A, B, sc1, f"{case} first")
        assert info["path"] == 2 and info["why_full"] == 1 and info["calls"] == 1, info
        other = (t + 1) % sc.tri_count
        v1 = tris(sc1)
        new2 = (v1[other] * np.float32(0.999)).astype(np.float32)      # (towards the origin: the maximum cannot rise)
        assert vmax_bits(patched(sc1, [other], new2[None]).vertices) == vmax_bits(sc1.vertices)
        sc2 = both(A, B, sc1, [other], new2[None])
        info = A.sparse_info()
        assert_same_structure(A, B, sc2, f"{case} second")
        assert info["path"] == 1 and info["calls"] == 2, info
    finally:
        A.close()
        B.close()


# ---- 5: an object ----

def moved_blob(sc, seed=3):
    per = sc.tri_count // BLOB_INSTANCES
    ids = np.random.default_rng(seed).permutation(per)
    return ids, edit_M(sc)["vertices"][ids]


def test_an_object_moved_onto_another():
    sc = scene("blobs")
    A, B = pair(sc)
    try:
        ids, new = moved_blob(sc)
        sc_new = both(A, B, sc, ids, new)
        info = A.sparse_info()
        print(f"blobs / M: {info}")
        assert_same_structure(A, B, sc_new, "blobs / M")
        assert info["moved"] == len(ids) and info["path"] in (1, 2)
        if info["path"] == 1:
            assert info["dirty_nodes8"] < A.accel_info()["node_count"]
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("edit", ["M", "J"])
def test_every_triangle_listed_in_a_seeded_permutation(edit):
    sc = scene("blobs")
    A, B = pair(sc)
    try:
        ids = np.random.default_rng(5).permutation(sc.tri_count)
        full = edit_M(sc)["vertices"] if edit == "M" else edit_J(sc)["vertices"]
        sc_new = both(A, B, sc, ids, full.reshape(-1, 3, 3)[ids])
        info = A.sparse_info()
        print(f"blobs / {edit}, count == tri_count: {info}")
        assert_same_structure(A, B, sc_new, f"blobs / {edit} / all")
        assert info["moved"] == sc.tri_count
        if info["path"] == 1:
            assert info["dirty_nodes8"] == A.accel_info()["node_count"]
    finally:
        A.close()
        B.close()


# ---- 6: normals only ----

def test_normals_only_change_the_lifts_and_nothing_else():
    sc = scene("soup-6000")
    A, B = pair(sc)
    try:
        n = sc.tri_count
        ids = np.random.default_rng(11).permutation(n)[: n // 10]
        turned = edit_J(sc)["normals"].reshape(-1, 3, 3)[ids]
        before = A.debug_read_accel()
        sc_new = both(A, B, sc, ids, tris(sc)[ids], normals=turned)
        after = assert_same_structure(A, B, sc_new, "normals only")
        info = A.sparse_info()
        assert info["path"] == 1, info
        assert A.accel_info()["lift_bound"] == B.accel_info()["lift_bound"]
        da, db = after["isect"]["lift"][:n], B.debug_read_accel()["isect"]["lift"][:n]
        assert da.tobytes() == db.tobytes()
        listed = np.isin(after["isect"]["tri_id"][:n], ids)
        assert before["attr"][:n][~listed].tobytes() == after["attr"][:n][~listed].tobytes()
        assert before["attr"][:n][listed].tobytes() != after["attr"][:n][listed].tobytes()
        assert (before["isect"]["lift"][:n][listed] != da[listed]).any()
    finally:
        A.close()
        B.close()


# ---- 7: sequences ----

def test_sparse_then_full_then_sparse():
    sc = scene("soup-6000")
    A, B = pair(sc)
    try:
        t, new = inner_triangle(sc)
        sc1 = both(A, B, sc, [t], new[None])
        assert_same_structure(A, B, sc1, "sparse")
        full = edit_J(sc1)
        for rm in (A, B):
            rm.update(**full)
        sc2 = with_arrays(sc1, **full)
        assert_same_structure(A, B, sc2, "full")
        ids = np.random.default_rng(2).permutation(sc.tri_count)[:50]
        new = (tris(sc2)[ids] * np.float32(0.99)).astype(np.float32)
        sc3 = both(A, B, sc2, ids, new)
        info = A.sparse_info()
        assert_same_structure(A, B, sc3, "sparse again")
        assert info["calls"] == 2 and info["moved"] == 50
        assert info["path"] == (1 if vmax_bits(sc3.vertices) == vmax_bits(sc2.vertices) else 2), info
    finally:
        A.close()
        B.close()


def test_sparse_under_always_then_never():
    sc = scene("soup-6000")
    A, B = pair(sc)
    try:
        for rm in (A, B):
            rm.set_update_policy(abi.REBUILD_ALWAYS)
        t, new = inner_triangle(sc)
        sc1 = both(A, B, sc, [t], new[None])
        assert_same_structure(A, B, sc1, "always")
        fresh = manager(sc1)
        try:
            ra, rf = raw_buffers(A.debug_read_accel()), raw_buffers(fresh.debug_read_accel())
            for k in ra:
                assert ra[k] == rf[k], k
        finally:
            fresh.close()
        info, ra, rb = A.sparse_info(), A.rebuild_info(), B.rebuild_info()
        assert info["path"] == 3 and info["calls"] == 1 and A.accel_info()["builder"] != 2, info
        assert (ra["rebuilds"], ra["last_decision"]) == (rb["rebuilds"], rb["last_decision"]) == (1, 3)
        for rm in (A, B):
            rm.set_update_policy(abi.REBUILD_NEVER)
        other = (t + 1) % sc.tri_count
        new2 = (tris(sc1)[other] * np.float32(0.999)).astype(np.float32)
        sc2 = both(A, B, sc1, [other], new2[None])
        info = A.sparse_info()
        assert_same_structure(A, B, sc2, "never after always")
        assert info["path"] == 2 and info["why_full"] == 1, info      # the rebuild dropped the kept boxes
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("ratio", [1.0, 1e9])
def test_sparse_under_auto_decides_as_the_full_update(ratio):
    sc = scene("soup-6000")
    A, B = pair(sc, warm_up=False)
    try:
        for rm in (A, B):
            rm.set_update_policy(abi.REBUILD_AUTO, ratio)
        cur = sc
        ids, new = np.arange(0, 600), None
        for step in range(2):
            new = (tris(cur)[ids] + np.float32(0.4) * (step + 1)).astype(np.float32)      # a tenth of the soup moved apart: the tree degrades
            cur = both(A, B, cur, ids, new)
            assert_same_structure(A, B, cur, f"auto {ratio} step {step}")
            ra, rb = A.rebuild_info(), B.rebuild_info()
            print(f"auto {ratio} step {step}: {ra}  sparse {A.sparse_info()}")
            for k in ("mode", "max_cost_ratio", "rebuilds", "last_decision"):
                assert ra[k] == rb[k], (k, ra, rb)
            for k in ("cost_built", "cost_refit", "cost_after"):
                assert np.float64(ra[k]).view(np.uint64) == np.float64(rb[k]).view(np.uint64), (k, ra, rb)
            ca, cb = A.accel_cost(), B.accel_cost()
            assert np.float64(ca["cost"]).view(np.uint64) == np.float64(cb["cost"]).view(np.uint64) and ca["builder"] == cb["builder"]
            assert A.sparse_info()["path"] == (3 if ra["last_decision"] != 1 else A.sparse_info()["path"])
        assert A.rebuild_info()["last_decision"] == (1 if ratio == 1e9 else 2)
    finally:
        A.close()
        B.close()


# ---- 8: outputs ----

def rendered_three_ways(sc, ids, vertices, flags=0, rank=0, world=1, before=None, camera=None):
    """4 spp, the update, 4 spp on A (sparse) and B (full); 4 spp on a fresh create + begin of the edited description"""
    A, B = pair(sc, flags, rank, world)
    fresh = None
    try:
        for rm in (A, B):
            if before:
                before(rm)
            rm.render(4)
        sc_new = both(A, B, sc, ids, vertices, camera=camera)
        if camera is not None:
            sc_new = with_arrays(sc_new, camera=camera)
        fresh = manager(sc_new, flags, rank, world)
        oa = outputs(A)
        assert_same_outputs(oa, outputs(B), "right after the update, against the full update")
        assert_same_outputs(oa, outputs(fresh), "right after the update, against a fresh begin")
        for rm in (A, B, fresh):
            rm.render(4)
        oa = outputs(A)
        assert_same_outputs(oa, outputs(B), "after 4 spp, against the full update")
        assert_same_outputs(oa, outputs(fresh), "after 4 spp, against a fresh begin")
        assert A.counters() == B.counters() == fresh.counters()
        assert A.get_render_info().samples == B.get_render_info().samples == fresh.get_render_info().samples == 5
        assert A.light_info() == B.light_info() == fresh.light_info()
        assert A.adaptive_info() == B.adaptive_info() == fresh.adaptive_info()
        return A.sparse_info(), A.light_info()
    finally:
        for rm in (A, B, fresh):
            if rm is not None:
                rm.close()


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_render_after_one_triangle_moved(schedule):
    sc = scene("soup-6000")
    t, new = inner_triangle(sc)
    info, _ = rendered_three_ways(sc, [t], new[None], SCHEDULES[schedule])
    assert info["path"] == 1


def test_render_after_an_object_moved():
    sc = scene("blobs")
    ids, new = moved_blob(sc)
    rendered_three_ways(sc, ids, new)


def test_render_on_rank_1_of_3_with_a_camera():
    sc = scene("soup-6000")
    t, new = inner_triangle(sc)
    rendered_three_ways(sc, [t], new[None], rank=1, world=3, camera=moved_camera(sc))


def test_render_with_mesh_lights_and_a_moved_emitter():
    sc = scenes.cornell(48, 48)
    ids = np.array([11, 10])
    new = (tris(sc)[ids] + np.array([0.3, -0.2, 0.25], np.float32)).astype(np.float32)      # the light: lower and off centre
    _, lights = rendered_three_ways(sc, ids, new, abi.FLAG_MESH_LIGHTS)
    assert lights["emitters"] == 2


def test_render_after_an_adaptive_render():
    sc = scene("soup-6000")
    t, new = inner_triangle(sc)
    rendered_three_ways(sc, [t], new[None], before=lambda m: m.set_adaptive(1e-3, 3, 1))


def test_aimed_rays_after_an_object_moved():
    sc = scene("blobs")
    A, B = pair(sc)
    try:
        ids, new = moved_blob(sc)
        sc_new = both(A, B, sc, ids, new)
        o, d, _, _ = aimed_rays(sc_new, BARY)
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


# ---- 9: refusals ----

def test_refused_sparse_updates_leave_everything_as_it_was():
    sc = scene("soup-6000")
    rm, plain = manager(sc), manager(sc)
    try:
        for m in (rm, plain):
            m.update(vertices=sc.vertices)
            m.render(2)
        before = raw_buffers(rm.debug_read_accel()), rm.update_info(), rm.sparse_info(), rm.accel_info()
        n = sc.tri_count
        v = np.ascontiguousarray(tris(sc)[:2])
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

        def call(what=abi.UPDATE_GEOMETRY, ids=(0, 1), vertices=v, count=None):
            ids = np.asarray(ids, np.uint32)
            u = abi.ErSparseUpdate()
            u.what, u.count = what, len(ids) if count is None else count
            u.tri_ids = ids.ctypes.data_as(C.POINTER(C.c_uint32))
            if vertices is not None:
                u.vertices = fp(vertices)
            return rm.lib.er_render_update_sparse(rm.handle, C.byref(u))

        bad = v.copy()
        bad[1, 2, 1] = np.nan
        inf = v.copy()
        inf[0, 0, 0] = np.inf
        refused = {"count 0": call(count=0), "an id equal to tri_count": call(ids=(0, n)), "a duplicated id": call(ids=(5, 5)), "a NaN": call(vertices=bad),
                   "an infinity": call(vertices=inf), "what 0": call(what=0), "an unknown bit": call(what=abi.UPDATE_GEOMETRY | 4), "NULL vertices": call(vertices=None),
                   "a NULL update": rm.lib.er_render_update_sparse(rm.handle, None)}
        for what, rc in refused.items():
            assert rc == abi.ER_ERR_INVALID_ARG, what
        u = abi.ErSparseUpdate()
        u.what, u.count, u.vertices = abi.UPDATE_GEOMETRY, 2, fp(v)
        assert rm.lib.er_render_update_sparse(rm.handle, C.byref(u)) == abi.ER_ERR_INVALID_ARG      # NULL tri_ids
        after = raw_buffers(rm.debug_read_accel()), rm.update_info(), rm.sparse_info(), rm.accel_info()
        assert before == after
        assert_same_outputs(outputs(rm), outputs(plain), "right after refused sparse updates")
        rm.render(2)
        plain.render(2)
        assert_same_outputs(outputs(rm), outputs(plain), "a render continued after refused sparse updates")
    finally:
        rm.close()
        plain.close()
