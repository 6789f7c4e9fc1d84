"""The scene of tests/deep_tree_scenes.py judged WITHOUT a GPU (the precedents: tests/test_long_path_scenes_cpu.py, tests/test_accel_check_cpu.py).

tests/test_gpu_deep_tree.py holds every wide traversal to the oracle on rays whose stacks go beyond the WF_LDS_STACK levels kept in LDS
(DESIGN.md section 2).  It says something only if the scene really produces such stacks and is worth shading; the host builder, the
replay of the first descent and the oracle alone show here that it does, for every description the GPU file renders:
  * the host-built structure passes accel_check.check; its wide depth is at most ER_STACK8 and at least WF_LDS_STACK + 6;
  * over the pixel-centre rays of the frame at most 2 % are marginal (a box decision within 1e-4 of a face) and left out, at least half of
    the others leave WF_LDS_STACK + 4 entries or more on their first descent, and some ray leaves WF_LDS_STACK + 6;
  * the oracle's two traversal orders (its reference BVH and brute force) agree on every bit, so the GPU comparisons need no allowance
    for ties;
  * between a quarter and three quarters of the pixels hit geometry, the mean path is at least 2 iterations at max_bounces 8, and at
    least a quarter of the hit pixels have values of their own.
A parameter set that failed a condition would be answered by another scene (ratio, ring size, seed, materials), never by another condition.

Measured with the host builder (printed by the tests): 648 triangles, binary depth 20, wide depth 15; on the 24 x 16 frame 0.5 % of the rays
marginal and of the others 1 / 2 / 1 / 8 / 370 leave 10 / 11 / 12 / 13 / 14 entries; on the 160 x 120 frame 0.6 % marginal and
70 / 93 / 127 / 494 / 18 305 leave 10 / 11 / 12 / 13 / 14; 60 % of the pixels hit, 2.1 iterations per path.

And the negative result this file exists for: on scenes.soup(6000) and scenes.cornell no camera ray leaves more than WF_LDS_STACK entries."""
import functools

import numpy as np
import pytest

import accel_check
import deep_tree_scenes as dts
from elevenrender_amd import abi, scenes

LDS, STACK8 = dts.WF_LDS_STACK, dts.ER_STACK8
# every description tests/test_gpu_deep_tree.py renders: (name, frame)
RENDERED = [("shells", (24, 16)), ("shells", (160, 120)), ("scaled", (24, 16)), ("posed", (24, 16))]
IDS = [f"{n}-{w}x{h}" for n, (w, h) in RENDERED]
SPP, MAX_BOUNCES = 4, 8


@functools.lru_cache(maxsize=None)
def scene(name, frame):
    sc = dts.nested_shells(*frame)
    return {"shells": lambda s: s, "scaled": dts.scaled, "posed": dts.posed}[name](sc)


@functools.lru_cache(maxsize=None)
def dump(name, frame):
    return dts.host_dump(scene(name, frame))


def run(oracle_mod, sc, traversal):
    orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, max_bounces=MAX_BOUNCES, traversal=traversal, threads=8)
    orc.render(SPP)
    out = {name: orc.read_pass(p) for name, p in abi.PASS_NAMES.items()}
    out["samples"], out["rng"], out["counters"] = orc.read_samples(), orc.read_rng(), orc.counters()
    orc.close()
    return out


def test_the_smallest_edge_is_bounded():
    with pytest.raises(AssertionError):
        dts.nested_shells(smallest=3.0e-10)
    sc = scene("shells", (24, 16))
    v = sc.vertices.astype(np.float64)
    edge = np.linalg.norm(v[:, 1] - v[:, 0], axis=-1)
    assert sc.tri_count == 648 and edge.min() >= 1e-10 and edge.min() ** 2 > 1e10 * np.finfo(np.float32).tiny
    assert len(set(sc.material_id.tolist())) == 4 and any(m.opacity < 1 for m in sc.materials)


@pytest.mark.parametrize("name,frame", RENDERED, ids=IDS)
def test_the_host_built_tree_is_sound_and_deep(name, frame):
    sc, d = scene(name, frame), dump(name, frame)
    rep = accel_check.check(sc, d)
    assert rep.ok, rep.message()
    print(f"{name}: {sc.tri_count} triangles, binary depth {d['max_depth']}, wide depth {d['max_depth8']}")
    assert LDS + 6 <= d["max_depth8"] <= STACK8


@pytest.mark.parametrize("name,frame", RENDERED, ids=IDS)
def test_camera_rays_leave_entries_beyond_the_lds_levels(name, frame):
    sc, d = scene(name, frame), dump(name, frame)
    o, dr = dts.pixel_centre_rays(sc)
    entries, marginal = dts.first_descent_entries(d, o, dr)
    keep = ~marginal
    print(f"{name} {frame[0]} x {frame[1]}: wide depth {d['max_depth8']}, marginal rays {marginal.mean():.4f}, first-descent entries "
          f"{{entries: rays}} {dts.distribution(entries, keep)}")
    assert marginal.mean() <= 0.02
    assert (entries[keep] >= LDS + 4).mean() >= 0.5
    assert entries[keep].max() >= LDS + 6
    assert entries.max() < d["max_depth8"]          # one entry per level below the root at most (csrc/er_trav.h)


@pytest.mark.parametrize("name,frame", RENDERED, ids=IDS)
def test_the_oracles_two_orders_agree_and_the_image_is_worth_comparing(oracle_mod, name, frame):
    sc = scene(name, frame)
    a = run(oracle_mod, sc, oracle_mod.TRAV_REFERENCE_BVH)
    b = run(oracle_mod, sc, oracle_mod.TRAV_BRUTE)
    for k in list(abi.PASS_NAMES) + ["samples", "rng"]:
        assert (np.ascontiguousarray(a[k]).view(np.uint32) == np.ascontiguousarray(b[k]).view(np.uint32)).all(), (name, k)
    for k in ("paths", "bounce_samples", "rays", "shaded_hits", "hdri_samples", "texel_fetches"):      # (not the traversal's own work)
        assert a["counters"][k] == b["counters"][k], (name, k)
    assert np.isfinite(a["beauty"]).all()
    orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, max_bounces=1)
    tri, _ = orc.closest_hit(*dts.pixel_centre_rays(sc))
    orc.close()
    hit = tri >= 0
    c = a["counters"]
    mean_path = c["bounce_samples"] / c["paths"]
    values = a["beauty"].reshape(-1, 4)[hit].view(np.uint32)
    distinct = len(np.unique(values, axis=0)) / max(1, int(hit.sum()))
    print(f"{name} {frame[0]} x {frame[1]}: {hit.mean():.3f} of the pixels hit, {mean_path:.2f} iterations per path, {distinct:.3f} of the hit pixels distinct")
    assert c["paths"] == frame[0] * frame[1] * SPP
    assert 0.25 <= hit.mean() <= 0.75
    assert mean_path >= 2.0
    assert distinct >= 0.25


@pytest.mark.parametrize("name", ["soup", "cornell"])
def test_ordinary_scenes_never_leave_the_lds_levels(name):
    """why the scene above exists: the suite's ordinary scenes stay within the LDS levels on every camera ray"""
    sc = scenes.soup(6000, 64, 48, seed=13, hdri_size=(64, 32)) if name == "soup" else scenes.cornell(64, 48)
    d = abi.debug_bvh_dump(sc.vertices, sc.normals)
    entries, _ = dts.first_descent_entries(d, *dts.pixel_centre_rays(sc))
    print(f"{name}: wide depth {d['max_depth8']}, most first-descent entries {int(entries.max())}")
    assert entries.max() <= LDS and d["max_depth8"] <= LDS + 1


def test_the_replay_on_a_hand_made_tree():
    """first_descent_entries against a two-level tree written by hand: the order is `slot ^ octant`, a level with a hit sibling counts one
    entry, a ray grazing a face is marginal"""
    n8 = np.zeros(3, abi.NODE8_DTYPE)
    # root: boxes of one unit per quantisation step (p = 0, e = 127): slot 0 = [0, 4]^3, slot 7 = [4, 8]^3, both inner
    n8["e"][:] = 127
    n8["imask"][0], n8["child_base"][0] = 0b10000001, 1
    for s, (lo, hi) in ((0, (0, 4)), (7, (4, 8))):
        n8["qlo"][0, :, s], n8["qhi"][0, :, s] = lo, hi
    # both children: leaves only
    o = np.array([[-1, -1, -1], [9, 9, 9], [-1, 1, 1], [-1, 4.0002, 4.0002]], np.float32)
    d = np.array([[1, 1, 1], [-1, -1, -1], [1, 0, 0], [1, 0, 0]], np.float32)
    entries, marginal = dts.first_descent_entries({"nodes8": n8}, o, d)
    assert entries.tolist() == [1, 1, 0, 0] and marginal.tolist() == [False, False, False, True]


def test_the_levels_hook_validates_its_arguments_and_reports_the_constants_without_a_device():
    """er_debug_trace_rays_levels: NULL outputs are refused before anything else is looked at; WF_LDS_STACK and ER_STACK8 as compiled are
    reported even so, and are what this file and tests/deep_tree_scenes.py state"""
    import ctypes as C
    lib = abi.load()
    lds, stack = C.c_uint32(), C.c_uint32()
    assert lib.er_debug_trace_rays_levels(None, None, None, 0, None, None, None, None, None, None, None, None, C.byref(lds), C.byref(stack)) == abi.ER_ERR_INVALID_ARG
    assert b"er_debug_trace_rays_levels" in lib.er_last_error()
    levels = (C.c_uint32 * 1)()
    assert lib.er_debug_trace_rays_levels(None, None, None, 0, None, None, None, None, None, None, None, levels, C.byref(lds), C.byref(stack)) == abi.ER_ERR_INVALID_ARG
    assert (lds.value, stack.value) == (LDS, STACK8)


def spill_area(n):
    """an untouched spill area for n rays: [blocks][levels][64 lanes][2 words] of 0xFFFFFFFF"""
    return np.full((-(-n // 64), STACK8, 64, 2), 0xFFFFFFFF, np.uint32)


def test_the_judgement_of_a_spill_area_on_hand_made_buffers():
    """er_debug_spill_levels (host code): the leading written levels per ray, and each of the three verdicts that make
    er_debug_trace_rays_levels fail"""
    n, usable = 70, 7                                   # two blocks, the second with 6 rays and 58 idle lanes
    a = spill_area(n)
    assert abi.debug_spill_levels(a, n, usable).tolist() == [0] * n
    a[0, 0:3, 5] = (12, 0x0104)                         # ray 5: three levels
    a[1, 0:7, 2] = (40, 0xFFFF)                         # ray 66: all usable levels, the largest second word an entry can have
    a[0, 0, 63] = (0xFFFFFFFF, 0)                       # ray 63: one level, whose first word alone looks like the fill
    want = np.zeros(n, np.uint32)
    want[[5, 66, 63]] = (3, 7, 1)
    assert (abi.debug_spill_levels(a, n, usable) == want).all()
    for what, (b, k, l), text in (("above an unwritten level", (0, 4, 5), b"above the unwritten level 3"),
                                  ("at the first level the tree has none for", (1, 7, 2), b"only 7 levels"),
                                  ("in an idle lane's column", (1, 0, 6), b"no ray")):
        bad = a.copy()
        bad[b, k, l] = (1, 1)
        with pytest.raises(abi.ErError) as e:
            abi.debug_spill_levels(bad, n, usable)
        assert e.value.code == abi.ER_ERR_STATE and text in abi.load().er_last_error(), what
    with pytest.raises(abi.ErError) as e:                # a buffer of another size is refused, not read
        abi.debug_spill_levels(a[:1], n, usable)
    assert e.value.code == abi.ER_ERR_INVALID_ARG
