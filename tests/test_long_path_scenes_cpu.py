"""The scenes of tests/long_path_scenes.py judged WITHOUT a GPU (the precedent: tests/test_mesh_light_scenes_cpu.py).

tests/test_gpu_long_paths.py holds the kernels to the oracle on paths of 24 to 1 001 iterations, at the edges of fields the kernels pack
(DESIGN.md "Parity").  It says something only if the scenes really produce such paths; the oracle alone shows here that they do:
  * 64 shells: every path of every configuration the GPU file renders runs exactly max_bounces iterations, each of them a shaded, opaque hit;
  * 2 shells at max_bounces 32: at least a tenth of the traced pixels on each side of 127 draws (csrc/er_stream.hip ST_DRAWS_MASK), with 4
    draws per opaque hit and, in the point-light variant, 5; and at least a tenth on each side of 32 iterations (mean length x 16 against
    the clamp at 511, ST_LONG_SHIFT);
  * the oracle's two traversal orders (its reference BVH and brute force over all triangles) agree on every bit of every scene and
    max_bounces used: no path meets two hits at exactly equal distance, so the GPU comparisons need no allowance for ties.
A size that failed a condition would be answered by another scene (seed, shells, frame), not by another condition."""
import functools

import numpy as np
import pytest

import long_path_scenes as lps
from elevenrender_amd import abi

POINT, MESH = abi.FLAG_POINT_LIGHTS | abi.FLAG_MIS, abi.FLAG_MESH_LIGHTS | abi.FLAG_MIS
# (scene kind, flags, max_bounces, spp) of every 64-shell render of tests/test_gpu_long_paths.py
FULL_LENGTH = [("plain", 0, mb, 3) for mb in (24, 25, 32, 43, 200, 1000, 1001)] + \
              [("point", POINT, 25, 3), ("point", POINT, 200, 3), ("plain", MESH, 25, 3), ("plain", MESH, 200, 3)]
# ... and of every 2-shell one (there at 160 x 120; here at 32 x 24, the frame the draw counts are measured on)
SPREAD = [("plain", 0, 32), ("plain", 0, 42), ("plain", 0, 43), ("point", POINT, 32)]


@functools.lru_cache(maxsize=None)
def scene(kind, n_shells, x_res, y_res):
    return lps.shells(x_res, y_res, n_shells) if kind == "plain" else lps.shells_point_lights(x_res, y_res, n_shells)


def run(oracle_mod, sc, flags, mb, spp, traversal):
    orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, max_bounces=mb, traversal=traversal, threads=8, flags=flags)
    if flags & abi.FLAG_MESH_LIGHTS:
        orc.set_emitters(lps.emitter_order(sc))
    orc.render(spp)
    out = {name: orc.read_pass(p) for name, p in abi.PASS_NAMES.items()}
    out["samples"], out["rng"], out["counters"] = orc.read_samples(), orc.read_rng(), orc.counters()
    orc.close()
    return out


def assert_same_bits(a, b, what):
    for k in list(abi.PASS_NAMES) + ["samples", "rng"]:
        assert (np.ascontiguousarray(a[k]).view(np.uint32) == np.ascontiguousarray(b[k]).view(np.uint32)).all(), (what, k)
    for k in ("paths", "bounce_samples", "rays", "shaded_hits", "hdri_samples", "texel_fetches"):      # (not the traversal's own work)
        assert a["counters"][k] == b["counters"][k], (what, k)


@pytest.mark.parametrize("kind,flags,mb,spp", FULL_LENGTH, ids=[f"{k}-flags{f}-mb{mb}" for k, f, mb, _ in FULL_LENGTH])
def test_64_shells_every_path_runs_max_bounces_iterations(oracle_mod, kind, flags, mb, spp):
    sc = scene(kind, 64, 16, 12)
    assert sc.tri_count == 1968
    a = run(oracle_mod, sc, flags, mb, spp, oracle_mod.TRAV_REFERENCE_BVH)
    c = a["counters"]
    assert c["paths"] == 16 * 12 * spp
    assert c["bounce_samples"] == c["shaded_hits"] == c["hdri_samples"] == c["paths"] * mb, c
    assert np.isfinite(a["beauty"]).all() and a["beauty"][..., :3].max() > 0
    b = run(oracle_mod, sc, flags, mb, spp, oracle_mod.TRAV_BRUTE)
    assert_same_bits(a, b, f"{kind} flags {flags} max_bounces {mb}")


@pytest.mark.parametrize("kind,flags,mb", SPREAD, ids=[f"{k}-mb{mb}" for k, _, mb in SPREAD])
def test_2_shells_two_traversal_orders_agree(oracle_mod, kind, flags, mb):
    sc = scene(kind, 2, 32, 24)
    assert sc.tri_count == 1224
    a = run(oracle_mod, sc, flags, mb, 4, oracle_mod.TRAV_REFERENCE_BVH)
    b = run(oracle_mod, sc, flags, mb, 4, oracle_mod.TRAV_BRUTE)
    assert_same_bits(a, b, f"{kind} max_bounces {mb}")
    assert a["counters"]["bounce_samples"] < a["counters"]["paths"] * mb      # (some paths do end early here)


@pytest.mark.parametrize("kind,flags,per_opaque", [("plain", 0, 4), ("point", POINT, 5)], ids=["plain", "point-lights"])
def test_2_shells_lie_on_both_sides_of_127_draws_and_32_iterations(oracle_mod, kind, flags, per_opaque):
    sc = scene(kind, 2, 32, 24)
    orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, max_bounces=32, threads=1, flags=flags)
    orc.render(2)
    draws, its = [], []
    for idx in lps.traced_pixels(sc, 128):
        recs = orc.trace_pixel(int(idx), max_recs=34)
        draws.append(lps.draw_count(recs, per_opaque))
        its.append(len(recs))
    orc.close()
    draws, its = np.array(draws), np.array(its)
    print(f"{kind}: draw counts <= 127: {(draws <= 127).sum()}, > 127: {(draws > 127).sum()}, {len(set(draws.tolist()))} distinct; "
          f"iterations: quartiles {np.percentile(its, [0, 25, 50, 75, 100]).tolist()}, < 32: {(its < 32).sum()}, 32: {(its == 32).sum()}")
    assert its.max() == 32
    assert (draws <= 127).mean() >= 0.1 and (draws > 127).mean() >= 0.1
    assert (its < 32).mean() >= 0.1 and (its == 32).mean() >= 0.1
    assert len(set(draws.tolist())) >= 8      # (guesses that will be right and guesses that will be wrong)


def test_draw_count_replays_the_rng(oracle_mod):
    """draw_count against the generator itself: after one traced sample of a pixel, the pixel's state is its state before advanced
    by exactly that many draws (xorshift32, oracle_xorshift32) -- for 4 and for 5 draws per opaque hit."""
    import ctypes as C
    for kind, flags, per_opaque in (("plain", 0, 4), ("point", POINT, 5)):
        sc = scene(kind, 2, 32, 24)
        orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, max_bounces=32, threads=1, flags=flags)
        orc.render(1)
        for idx in lps.traced_pixels(sc, 16):
            before = int(orc.read_rng()[idx])
            n = lps.draw_count(orc.trace_pixel(int(idx), max_recs=34), per_opaque)
            after = int(orc.read_rng()[idx])
            state = C.c_uint32(before)
            for _ in range(n):
                oracle_mod.lib().oracle_xorshift32(C.byref(state))
            assert state.value == after, (kind, int(idx), n)
        orc.close()
