"""The structure's measured cost on the device (er_accel_cost, csrc/er_cost.hip) and the rebuild policies of er_render_update /
er_render_edit (er_update_policy_set) against the contract of include/eleven_hip.h:

cost     every per-node and per-record term of the device measurement equals the numpy replay of the definition (tests/accel_cost.py) bit for
         bit, the sums lie within the bound for reordering, two measurements return the same bits, and the render's state is not touched;
ALWAYS   after the update the four structure buffers equal a fresh create + begin of the edited scene byte for byte, and so does
         every readable output;
AUTO     the refit is kept where the measured ratio stays below the caller's, the structure is built fresh where it does not, and
         the decision is the one the reported numbers give.

The edits are those of tests/test_gpu_update.py (T, J, M) and S5 of tests/test_accel_cost_cpu.py: the first 5 % of the triangles
scattered over the scene's extent."""
import ctypes as C

import numpy as np
import pytest

import accel_check
import accel_cost
from elevenrender_amd import abi, scenes
from test_accel_cost_cpu import edit_S5
from test_gpu_accel_structure import BUILDERS, raw_buffers, scene
from test_gpu_edit import T as small_torture
from test_gpu_edit import changed, edit_args
from test_gpu_update import SCHEDULES, assert_same_outputs, edit_J, edit_M, edit_T, manager, outputs, with_arrays

pytestmark = pytest.mark.gpu

EDITS = {"T": edit_T, "J": edit_J, "M": edit_M, "S5": edit_S5}
COST_CASES = ["soup-3", "soup-257", "soup-6000", "soup-20001", "blobs", "torture", "same-centroid"]
INFO_FIELDS = ("node_count", "node_bytes", "leaf_count", "max_depth", "tri_record_bytes", "lift_bound", "builder")
SUMS = ("node_area", "leaf_area", "tri_area", "cost")


def bits(x):
    return np.float64(x).tobytes()


def assert_same_structure(rm, fresh, sc_new, what):
    """the four raw buffers byte for byte, the checker clean, accel_info equal apart from the two times"""
    dump, fresh_dump = rm.debug_read_accel(), fresh.debug_read_accel()
    a, b = raw_buffers(dump), raw_buffers(fresh_dump)
    for k in a:
        assert len(a[k]) == len(b[k]), f"{what}: {k} has {len(a[k])} bytes, fresh {len(b[k])}"
        assert a[k] == b[k], f"{what}: {k} differs from a fresh build's"
    info, fresh_info = rm.accel_info(), fresh.accel_info()
    for f in INFO_FIELDS:
        assert info[f] == fresh_info[f], (what, f, info[f], fresh_info[f])
    assert info["builder"] in (0, 1) and dump["builder"] == info["builder"]
    for f in ("lo", "hi", "lift_bound", "max_lift"):
        assert dump[f].tobytes() == fresh_dump[f].tobytes(), (what, f)
    assert dump["max_depth"] == fresh_dump["max_depth"] and dump["max_depth8"] == fresh_dump["max_depth8"]
    rep = accel_check.check(sc_new, dump, accel_depth=info["max_depth"])
    assert rep.ok, (what, rep.message())


# ---- 1. cost ----

@pytest.mark.parametrize("case,builder", [(c, b) for c in COST_CASES for b in ("host", "device")] + [("soup-20001", "default")])
def test_device_cost_equals_the_replay(case, builder):
    sc = scene(case)
    rm = manager(sc, BUILDERS[builder])
    try:
        rm.render(2)
        before = outputs(rm)
        info = rm.accel_info()
        if builder == "default":
            assert info["builder"] == 1
        elif sc.tri_count >= 6000:
            assert info["builder"] == (1 if builder == "device" else 0)
        for stage in ("built", "refitted"):
            if stage == "refitted":
                rm.update(**edit_J(sc))
                rm.render(2)
                before = outputs(rm)
            what = f"{case} / {builder} / {stage}"
            cost = rm.accel_cost()
            terms = rm.debug_accel_cost_terms()
            again = rm.accel_cost()
            ref = accel_cost.replay(rm.debug_read_accel())
            print(f"{what}: cost {cost['cost']:.6g} (replay {ref['cost']:.6g}), {cost['ms']:.3f} ms")
            accel_cost.assert_matches(terms, ref, what)
            for k in SUMS:      # two measurements (the kept one and the hook's own run): the same bits
                assert bits(cost[k]) == bits(terms[k]) == bits(again[k]), (what, k, cost[k], terms[k], again[k])
            assert cost["builder"] == rm.accel_info()["builder"] == (2 if stage == "refitted" else info["builder"])
            assert cost["ms"] == again["ms"] and cost["cost"] > 0
            assert_same_outputs(outputs(rm), before, what + ": outputs after the measurement")
        assert rm.rebuild_info()["rebuilds"] == 0 and rm.rebuild_info()["last_decision"] == 0
    finally:
        rm.close()


# ---- 2. ALWAYS ----

@pytest.mark.parametrize("case,edit", [(c, e) for c in ("soup-6000", "soup-20001") for e in ("T", "J", "S5")] + [("blobs", "M")])
def test_always_leaves_the_structure_of_a_fresh_build(case, edit):
    sc = scene(case)
    arrays = EDITS[edit](sc)
    sc_new = with_arrays(sc, **arrays)
    rm = manager(sc)
    fresh = manager(sc_new)
    try:
        assert rm.accel_info()["builder"] == (1 if case == "soup-20001" else 0)
        rm.set_update_policy(abi.REBUILD_ALWAYS)
        rm.update(**arrays)
        upd, reb = rm.update_info(), rm.rebuild_info()
        print(f"{case} / {edit}: update {upd['update_ms']:.3f} ms, structure stage {reb['rebuild_ms']:.3f} ms")
        assert_same_structure(rm, fresh, sc_new, f"{case} / {edit}")
        assert upd["updates"] == 1 and upd["refits"] == 0
        assert reb["rebuilds"] == 1 and reb["last_decision"] == 3 and reb["mode"] == abi.REBUILD_ALWAYS and reb["rebuild_ms"] > 0
    finally:
        rm.close()
        fresh.close()


def rebuilt_and_fresh(sc, args, flags=0, rank=0, world=1, before=None):
    """(manager, fresh manager) after: 4 spp, the update under ALWAYS, 4 spp -- and a fresh create + begin + 4 spp of the edited description"""
    rm = manager(sc, flags, rank, world)
    rm.set_update_policy(abi.REBUILD_ALWAYS)
    if before:
        before(rm)
    rm.render(4)
    rm.update(**args)
    fresh = manager(with_arrays(sc, **args), flags, rank, world)
    try:
        assert rm.get_render_info().samples == fresh.get_render_info().samples
        assert rm.adaptive_info() == fresh.adaptive_info() and rm.adaptive_info()["enabled"] == 0
        assert_same_outputs(outputs(rm), outputs(fresh), "right after the update")
        rm.render(4)
        fresh.render(4)
    except BaseException:
        rm.close()
        fresh.close()
        raise
    return rm, fresh


def assert_same_render(rm, fresh, what):
    try:
        assert_same_outputs(outputs(rm), outputs(fresh), what)
        assert rm.counters() == fresh.counters()
        assert rm.get_render_info().samples == fresh.get_render_info().samples == 5
        assert rm.light_info() == fresh.light_info() and rm.adaptive_info() == fresh.adaptive_info()
        assert rm.update_info()["refits"] == 0 and rm.rebuild_info()["rebuilds"] == 1
    finally:
        rm.close()
        fresh.close()


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_render_after_a_rebuilding_update_equals_a_fresh_render(schedule):
    sc = scene("soup-6000")
    rm, fresh = rebuilt_and_fresh(sc, edit_S5(sc), SCHEDULES[schedule])
    assert_same_render(rm, fresh, f"S5 / {schedule}")


def test_rebuilding_update_on_rank_1_of_3():
    sc = scene("soup-6000")
    rm, fresh = rebuilt_and_fresh(sc, edit_S5(sc), 0, rank=1, world=3)
    assert_same_render(rm, fresh, "rank 1 of 3")


def test_rebuilding_update_with_mesh_lights_and_a_moved_emitter():
    sc = scenes.cornell(48, 48)
    v = sc.vertices.reshape(-1, 3, 3).copy()
    v[10:12] += np.array([0.3, -0.2, 0.25], np.float32)      # the light: lower and off centre
    rm, fresh = rebuilt_and_fresh(sc, dict(vertices=v), abi.FLAG_MESH_LIGHTS)
    try:
        assert rm.light_info()["emitters"] == 2
        (tri_a, cdf_a), (tri_b, cdf_b) = rm.debug_light_table(), fresh.debug_light_table()
        assert tri_a.tolist() == tri_b.tolist() and sorted(tri_a.tolist()) == [10, 11] and cdf_a.tobytes() == cdf_b.tobytes()
    except BaseException:
        rm.close()
        fresh.close()
        raise
    assert_same_render(rm, fresh, "mesh lights")


def test_rebuilding_update_after_an_adaptive_render():
    sc = scene("soup-6000")
    rm, fresh = rebuilt_and_fresh(sc, edit_S5(sc), before=lambda m: m.set_adaptive(1e-3, 3, 1))
    assert_same_render(rm, fresh, "after an adaptive render")


def test_always_through_er_render_edit_with_geometry_and_materials():
    old = small_torture()
    ids = np.roll(old.material_id, 7)
    new = changed(old, materials={1: {"roughness": 0.3, "albedo": (0.2, 0.7, 0.4)}}, material_id=ids, **edit_S5(old))
    rm = manager(old)
    fresh = manager(new)
    try:
        rm.set_update_policy(abi.REBUILD_ALWAYS)
        rm.render(4)
        rm.edit(**edit_args(old, new, geometry=True))
        assert rm.edit_info()["edits"] == 1 and rm.update_info()["refits"] == 0 and rm.rebuild_info()["last_decision"] == 3
        assert_same_structure(rm, fresh, new, "edit: GEOMETRY | MATERIALS")
        assert_same_outputs(outputs(rm), outputs(fresh), "right after the edit")
        rm.render(4)
        fresh.render(4)
    except BaseException:
        rm.close()
        fresh.close()
        raise
    assert_same_render(rm, fresh, "edit: GEOMETRY | MATERIALS")


# ---- 3. AUTO ----

def never_ratio(sc, arrays):
    """the control, in numpy from a NEVER-policy run's dumps: (cost of the refitted tree) / (cost of the built tree), and the refit's raw buffers"""
    rm = manager(sc)
    try:
        built = accel_cost.replay(rm.debug_read_accel())["cost"]
        rm.update(**arrays)
        dump = rm.debug_read_accel()
        assert rm.accel_info()["builder"] == 2 and rm.rebuild_info()["last_decision"] == 0
        return accel_cost.replay(dump)["cost"] / built, raw_buffers(dump)
    finally:
        rm.close()


@pytest.mark.parametrize("case", ["soup-6000", "soup-20001"])
def test_auto_keeps_a_good_refit_and_rebuilds_a_degraded_one(case):
    sc = scene(case)
    t, s5 = edit_T(sc), edit_S5(sc)
    ratio_t, refit_t = never_ratio(sc, t)
    ratio_s, _ = never_ratio(sc, s5)
    print(f"{case}: numpy ratio of the NEVER-policy dumps: T {ratio_t:.4f}, S5 {ratio_s:.4f}")
    assert ratio_t <= 1.1 and ratio_s >= 3.0      # the controls: the edits are what the test takes them for
    decided = lambda r: (r["last_decision"] == 2) == (r["cost_refit"] > 2.0 * r["cost_built"])

    rm = manager(sc)
    try:
        rm.set_update_policy(abi.REBUILD_AUTO, 2.0)
        rm.update(**t)
        r = rm.rebuild_info()
        assert r["last_decision"] == 1 and decided(r) and r["rebuilds"] == 0 and r["cost_after"] == 0 and r["cost_built"] > 0 and r["rebuild_ms"] == 0
        assert rm.accel_info()["builder"] == 2 and rm.update_info()["refits"] == 1
        got = raw_buffers(rm.debug_read_accel())
        for k in got:
            assert got[k] == refit_t[k], f"T under AUTO: {k} differs from the NEVER refit's"
        assert bits(rm.accel_cost()["cost"]) == bits(r["cost_refit"])
    finally:
        rm.close()

    sc_s = with_arrays(sc, **s5)
    rm, fresh = manager(sc), manager(sc_s)
    try:
        rm.set_update_policy(abi.REBUILD_AUTO, 2.0)
        rm.render(2)
        rm.update(**s5)
        r = rm.rebuild_info()
        print(f"   S5 under AUTO: cost built {r['cost_built']:.6g}, refit {r['cost_refit']:.6g}, after {r['cost_after']:.6g}; measurements {r['cost_ms']:.3f} ms, structure stage {r['rebuild_ms']:.3f} ms")
        assert r["last_decision"] == 2 and decided(r) and r["rebuilds"] == 1 and rm.update_info()["refits"] == 0
        assert_same_structure(rm, fresh, sc_s, "S5 under AUTO")
        assert bits(r["cost_after"]) == bits(fresh.accel_cost()["cost"]) == bits(rm.accel_cost()["cost"])
        assert_same_outputs(outputs(rm), outputs(fresh), "S5 under AUTO")
        # a translation of the rebuilt scene is judged against the NEW baseline: the refit is kept
        t2 = edit_T(sc_s)
        rm.update(**t2)
        r2 = rm.rebuild_info()
        assert r2["last_decision"] == 1 and decided(r2) and r2["rebuilds"] == 1 and rm.accel_info()["builder"] == 2
        assert bits(r2["cost_built"]) == bits(r["cost_after"])
        assert rm.update_info()["refits"] == 1 and rm.update_info()["updates"] == 2
    finally:
        rm.close()
        fresh.close()


# ---- 4. no baseline ----

def test_auto_rebuilds_a_refit_of_unknown_ancestry():
    sc = scene("soup-6000")
    j = edit_J(sc)
    sc_j = with_arrays(sc, **j)
    rm, fresh = manager(sc), manager(sc_j)
    try:
        rm.update(**j)                                   # NEVER: a refit, nothing measured
        assert rm.accel_info()["builder"] == 2
        rm.set_update_policy(abi.REBUILD_AUTO, 2.0)
        rm.update(**j)                                   # the unchanged arrays
        r = rm.rebuild_info()
        assert r["last_decision"] == 4 and r["rebuilds"] == 1 and r["cost_built"] == 0 and r["cost_refit"] == 0 and r["cost_after"] > 0
        assert rm.update_info()["refits"] == 1 and rm.update_info()["updates"] == 2
        assert_same_structure(rm, fresh, sc_j, "no baseline")
        assert bits(r["cost_after"]) == bits(fresh.accel_cost()["cost"])
    finally:
        rm.close()
        fresh.close()


# ---- 5. refusals ----

def test_refused_updates_under_always_leave_everything_as_it_was():
    sc = scene("soup-6000")
    rm = manager(sc)
    try:
        rm.set_update_policy(abi.REBUILD_ALWAYS)
        rm.render(2)
        before = outputs(rm), raw_buffers(rm.debug_read_accel()), rm.accel_info(), rm.update_info(), rm.rebuild_info()
        u = abi.ErSceneUpdate()
        assert rm.lib.er_render_update(rm.handle, C.byref(u)) == abi.ER_ERR_INVALID_ARG                 # what = 0
        v = sc.vertices.copy()
        v.reshape(-1)[12345] = np.inf
        with pytest.raises(abi.ErError) as e:
            rm.update(vertices=v)
        assert e.value.code == abi.ER_ERR_INVALID_ARG and "finite" in str(e.value)
        after = outputs(rm), raw_buffers(rm.debug_read_accel()), rm.accel_info(), rm.update_info(), rm.rebuild_info()
        assert_same_outputs(after[0], before[0], "after refused updates")
        assert after[1:] == before[1:]
        assert after[4]["mode"] == abi.REBUILD_ALWAYS and after[4]["rebuilds"] == 0 and after[4]["last_decision"] == 0
    finally:
        rm.close()
