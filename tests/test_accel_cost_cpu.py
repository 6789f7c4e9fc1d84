"""The structure's measured cost without a device: the host compilation of csrc/er_cost.h (er_debug_accel_cost_host) against the numpy
replay of its definition (tests/accel_cost.py) on the host builder's structures; the metric's behaviour under the edits it is meant
to tell apart -- a translation and a scale leave it alone, scattered triangles raise it -- on a numpy refit of the built topology; and
the host state of er_update_policy_set.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import accel_check
import accel_cost
from elevenrender_amd import abi
from test_accel_check_cpu import host_dump
from test_gpu_accel_structure import scene
from test_gpu_update import edit_T, with_arrays

HOST_CASES = ["soup-3", "soup-257", "soup-6000", "torture", "same-centroid", "flat-grid"]


def edit_scale2(sc):
    return dict(vertices=(sc.vertices.reshape(-1, 3, 3) * np.float32(2.0)).astype(np.float32))


def edit_S(sc, share, seed=11):
    """the first `share` of the triangles moved, each as a whole, by U(-1/2, 1/2) x the scene's extent per axis"""
    v = sc.vertices.reshape(-1, 3, 3).copy()
    m = max(1, int(round(share * len(v))))
    extent = v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0)
    rng = np.random.default_rng(seed)
    v[:m] += (rng.uniform(-0.5, 0.5, size=(m, 1, 3)) * extent).astype(np.float32)
    return dict(vertices=v.astype(np.float32))


def edit_S5(sc):
    return edit_S(sc, 0.05)


@pytest.mark.parametrize("case", HOST_CASES)
def test_host_compilation_equals_the_replay(case):
    sc = scene(case)
    d = host_dump(sc)
    got = abi.debug_accel_cost_host(d["nodes8"], d["isect"], d["tri_count"])
    ref = accel_cost.replay(d)
    print(f"{case}: {d['node8_count']} wide nodes, node_area {ref['node_area']:.6g}, leaf_area {ref['leaf_area']:.6g}, tri_area {ref['tri_area']:.6g}, cost {ref['cost']:.6g}")
    assert ref["tri_area"] > 0 and ref["cost"] > 0
    accel_cost.assert_matches(got, ref, case)


def test_a_record_that_names_no_triangle_counts_nothing_and_an_empty_structure_costs_nothing():
    sc = scene("soup-257")
    d = host_dump(sc)
    d["isect"] = d["isect"].copy()
    d["isect"]["tri_id"][5], d["isect"]["tri_id"][200] = -1, 257
    got = abi.debug_accel_cost_host(d["nodes8"], d["isect"], d["tri_count"])
    assert got["tri_terms"][5] == 0 and got["tri_terms"][200] == 0 and (got["tri_terms"] > 0).sum() == 255
    accel_cost.assert_matches(got, accel_cost.replay(d), "records without a triangle")
    empty = abi.debug_accel_cost_host(np.zeros(0, abi.NODE8_DTYPE), np.zeros(1, abi.ISECT_DTYPE), 0)
    assert empty["cost"] == 0 and empty["node_area"] == 0 and empty["tri_area"] == 0
    # every triangle a point: nothing to divide by
    flat = host_dump(sc)
    flat["isect"] = flat["isect"].copy()
    flat["isect"]["v1"], flat["isect"]["v2"] = flat["isect"]["v0"], flat["isect"]["v0"]
    assert abi.debug_accel_cost_host(flat["nodes8"], flat["isect"], flat["tri_count"])["cost"] == 0


def test_short_buffers_and_a_short_stride_are_refused():
    lib = abi.load()
    d = host_dump(scene("soup-3"))
    sums = abi.ErCostSumsDebug()
    n8, rec = np.ascontiguousarray(d["nodes8"]), np.ascontiguousarray(d["isect"])
    nt = np.zeros((len(n8), 2))
    args = (n8.ctypes.data_as(C.c_void_p), len(n8), 5, rec.ctypes.data_as(C.c_void_p), 3, C.byref(sums))
    assert lib.er_debug_accel_cost_host(*args, nt.ctypes.data_as(C.POINTER(C.c_double)), nt.nbytes - 1, None, 0) == abi.ER_ERR_INVALID_ARG
    assert lib.er_debug_accel_cost_host(*args, nt.ctypes.data_as(C.POINTER(C.c_double)), nt.nbytes, None, 0) == abi.ER_OK
    assert lib.er_debug_accel_cost_host(args[0], len(n8), 4, *args[3:], None, 0, None, 0) == abi.ER_ERR_INVALID_ARG
    assert lib.er_debug_accel_cost_host(*args[:5], None, None, 0, None, 0) == abi.ER_ERR_INVALID_ARG


# ---- what the metric tells apart ----

@pytest.fixture(scope="module", params=["soup-6000", "blobs"])
def built(request):
    sc = scene(request.param)
    d = host_dump(sc)
    return request.param, sc, d, accel_cost.refitted_float_cost(sc, d)["cost"]


@pytest.mark.parametrize("edit,lo,hi", [(edit_T, 0.99, 1.01), (edit_scale2, 0.99, 1.01), (edit_S5, 3.0, np.inf)], ids=["T", "x2", "S5"])
def test_cost_ratio_of_a_refitted_topology(built, edit, lo, hi):
    name, sc, d, q_built = built
    q_refit = accel_cost.refitted_float_cost(with_arrays(sc, **edit(sc)), d)["cost"]
    print(f"{name} / {edit.__name__}: Q_refit / Q_built = {q_refit / q_built:.4f}")
    assert q_built > 0
    assert lo <= q_refit / q_built <= hi


# ---- host state ----

def created(sc):
    lib = abi.load()
    h = C.c_void_p()
    abi.check(lib.er_scene_create(C.byref(sc.desc()), C.byref(h)))
    return lib, h


def policy_of(lib, h):
    info = abi.ErRebuildInfo()
    abi.check(lib.er_rebuild_info(h, C.byref(info)))
    return info.mode, info.max_cost_ratio


def test_update_policy_refusals_and_persistence_on_a_created_scene():
    lib, h = created(scene("soup-3"))
    try:
        assert policy_of(lib, h) == (abi.REBUILD_NEVER, 0.0)
        info = abi.ErRebuildInfo()
        abi.check(lib.er_rebuild_info(h, C.byref(info)))
        assert (info.rebuilds, info.last_decision, info.cost_built, info.cost_refit, info.cost_after, info.cost_ms, info.rebuild_ms) == (0, 0, 0, 0, 0, 0, 0)
        abi.check(lib.er_update_policy_set(h, C.byref(abi.ErUpdatePolicy(abi.REBUILD_AUTO, 2.5))))
        assert policy_of(lib, h) == (abi.REBUILD_AUTO, 2.5)
        for mode, ratio in ((3, 2.0), (0xFFFFFFFF, 2.0), (abi.REBUILD_AUTO, 0.999), (abi.REBUILD_AUTO, 0.0), (abi.REBUILD_AUTO, -3.0),
                            (abi.REBUILD_AUTO, float("nan")), (abi.REBUILD_AUTO, float("inf"))):
            assert lib.er_update_policy_set(h, C.byref(abi.ErUpdatePolicy(mode, ratio))) == abi.ER_ERR_INVALID_ARG, (mode, ratio)
            assert policy_of(lib, h) == (abi.REBUILD_AUTO, 2.5), (mode, ratio)
        assert lib.er_update_policy_set(h, None) == abi.ER_ERR_INVALID_ARG and lib.er_update_policy_set(None, C.byref(abi.ErUpdatePolicy(0, 0))) == abi.ER_ERR_INVALID_ARG
        assert lib.er_rebuild_info(h, None) == abi.ER_ERR_INVALID_ARG
        abi.check(lib.er_update_policy_set(h, C.byref(abi.ErUpdatePolicy(abi.REBUILD_AUTO, 1.0))))      # 1 is allowed: any growth rebuilds
        abi.check(lib.er_update_policy_set(h, C.byref(abi.ErUpdatePolicy(abi.REBUILD_ALWAYS, float("nan")))))      # the ratio is read for AUTO only
        assert policy_of(lib, h)[0] == abi.REBUILD_ALWAYS
        abi.check(lib.er_update_policy_set(h, C.byref(abi.ErUpdatePolicy(abi.REBUILD_NEVER, 0.0))))
        assert policy_of(lib, h) == (abi.REBUILD_NEVER, 0.0)
    finally:
        lib.er_scene_destroy(h)


def test_accel_cost_before_begin_is_a_state_error():
    lib, h = created(scene("soup-3"))
    try:
        c = abi.ErAccelCost()
        assert lib.er_accel_cost(h, C.byref(c)) == abi.ER_ERR_STATE
        assert lib.er_accel_cost(h, None) == abi.ER_ERR_INVALID_ARG and lib.er_accel_cost(None, C.byref(c)) == abi.ER_ERR_INVALID_ARG
        sums = abi.ErCostSumsDebug()
        assert lib.er_debug_accel_cost_terms(h, C.byref(sums), None, 0, None, 0) == abi.ER_ERR_STATE
    finally:
        lib.er_scene_destroy(h)
