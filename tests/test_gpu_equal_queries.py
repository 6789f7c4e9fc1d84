"""Shadow queries whose verdict cannot change the pixel are not traced (csrc/er_bounce.inc).

A shadow query selects one of two addends that are both computed before it is issued; where the two are the same bits
(a dead path: `reduction` exactly zero after a back-facing hit; an HDRI sample that is exactly black) the addend is added
at once and no ray is traced.  ER_TRACE_EVERY_QUERY=1 (read by er_render_begin) restores the old behaviour: every query
whose BRDF term is not exactly zero is traced.  The rule must change nothing but the `rays` counter: planes, RNG states,
sample counts and the other event counters are compared bit for bit between the two settings, between the schedules, and
with the oracle (which, like the reference, always traces).
"""
import os

import numpy as np
import pytest

from elevenrender_amd import abi, scenes
from test_gpu_parity import compare, gpu_render, oracle_render

pytestmark = pytest.mark.gpu

PLANES = ("beauty", "normal", "tangent", "bitangent")
COUNTS = ("paths", "bounce_samples", "shaded_hits", "hdri_samples")
SCHEDULES = {"stream": abi.FLAG_STREAM, "wavefront": abi.FLAG_WAVEFRONT, "megakernel": abi.FLAG_MEGAKERNEL}
KNOB = "ER_TRACE_EVERY_QUERY"


def render_with_knob(sc, spp, max_bounces, flags, every):
    """One render with the knob set (every = True) or unset; the environment is left as it was found."""
    before = os.environ.pop(KNOB, None)
    try:
        if every:
            os.environ[KNOB] = "1"
        return gpu_render(sc, spp, max_bounces=max_bounces, flags=flags)
    finally:
        os.environ.pop(KNOB, None)
        if before is not None:
            os.environ[KNOB] = before


def assert_same_result(a, b, what):
    for p in PLANES:
        assert (a[p].view(np.uint32) == b[p].view(np.uint32)).all(), (what, p)
    assert (a["rng"] == b["rng"]).all(), what
    assert (a["samples"] == b["samples"]).all(), what
    for k in COUNTS:
        assert a["counters"][k] == b["counters"][k], (what, k, a["counters"][k], b["counters"][k])


def queries(r):
    """Shadow queries traced: one closest-hit ray per bounce-loop iteration, the rest are queries."""
    return r["counters"]["rays"] - r["counters"]["bounce_samples"]


def the_soup():
    return scenes.soup(4000, 48, 36, seed=23, hdri_size=(64, 32))


@pytest.fixture(scope="module")
def soup_renders():
    """The soup in the three schedules, with the rule and with every query traced: rendered once, read by two tests."""
    sc = the_soup()
    return {(name, every): render_with_knob(sc, 6, 8, flags, every) for name, flags in SCHEDULES.items() for every in (False, True)}


def test_soup_rule_changes_only_the_ray_count(soup_renders):
    """scenes.soup(4000, 48, 36, seed=23), 8 bounces, 6 samples: identical results with the knob on and off and in every schedule,
    equal `rays` between the schedules under each setting, and at most three quarters of the queries left (the oracle's own count of
    queries with two different addends on this scene is 0.51 of those traced before: the cap tests the rule, not the scene)."""
    ref = soup_renders[("stream", True)]
    for key, r in soup_renders.items():
        assert_same_result(ref, r, key)
    for every in (False, True):
        rays = {name: soup_renders[(name, every)]["counters"]["rays"] for name in SCHEDULES}
        assert len(set(rays.values())) == 1, (every, rays)
    q_rule, q_every = queries(soup_renders[("stream", False)]), queries(soup_renders[("stream", True)])
    print(f"soup: shadow queries traced {q_rule} with the rule, {q_every} without: {q_rule / q_every:.4f}")
    assert q_rule <= 0.75 * q_every, (q_rule, q_every)


def test_soup_default_schedule_against_the_oracle(oracle_mod, soup_renders):
    """The same scene in the product's default schedule against the oracle, bit for bit like the other soup parity tests."""
    sc = the_soup()
    g = render_with_knob(sc, 6, 8, 0, False)
    o = oracle_render(oracle_mod, sc, 6, max_bounces=8)
    compare(g, o, min_exact=1.0, what="soup 4000, rule on, default schedule")
    assert g["counters"]["bounce_samples"] == o["counters"]["bounce_samples"]
    assert g["counters"]["rays"] == soup_renders[("stream", False)]["counters"]["rays"]


def test_soup_with_point_lights_and_mis():
    """Point lights and MIS: the light query follows the same rule; bit-exact with the knob on and off in the streaming and the
    wavefront schedule, and strictly fewer rays with the rule."""
    sc = the_soup()
    sc.point_lights = scenes.point_lights(5, seed=3, lo=(-0.8, -0.8, 2.2), hi=(0.8, 0.8, 3.8))
    sc._desc = None
    ext = abi.FLAG_POINT_LIGHTS | abi.FLAG_MIS
    r = {(name, every): render_with_knob(sc, 6, 8, SCHEDULES[name] | ext, every) for name in ("stream", "wavefront") for every in (False, True)}
    for key, other in r.items():
        assert_same_result(r[("stream", True)], other, key)
    for every in (False, True):
        assert r[("stream", every)]["counters"]["rays"] == r[("wavefront", every)]["counters"]["rays"], every
    print(f"soup with lights: rays {r[('stream', False)]['counters']['rays']} with the rule, {r[('stream', True)]['counters']['rays']} without")
    assert r[("stream", False)]["counters"]["rays"] < r[("stream", True)]["counters"]["rays"]


def test_live_paths_skip_a_black_hdri_sample(oracle_mod):
    """Cornell box under an HDRI whose lower half is exactly black, 5 bounces, 4 samples: hdriValue == 0 on live paths, and a scene
    in which few paths are dead.  Knob on and off bit for bit; against the oracle with the allowance the per-bounce trace test makes
    for Cornell (exact distance ties on the walls' shared edges: 0.999 of the pixels bit-exact)."""
    sc = scenes.cornell(48, 36)
    data = scenes.sky_hdri(64, 32)[0].copy()
    data[16:] = 0.0
    sc.hdri = (np.ascontiguousarray(data), 64, 32, 3, 0)
    sc._desc = None
    r = {(name, every): render_with_knob(sc, 4, 5, SCHEDULES[name], every) for name in ("stream", "wavefront") for every in (False, True)}
    for key, other in r.items():
        assert_same_result(r[("stream", True)], other, key)
    q_rule, q_every = queries(r[("stream", False)]), queries(r[("stream", True)])
    print(f"cornell, half-black HDRI: shadow queries traced {q_rule} with the rule, {q_every} without")
    assert 0 < q_rule < q_every
    o = oracle_render(oracle_mod, sc, 4, max_bounces=5)
    compare(r[("stream", False)], o, min_exact=0.999, what="cornell, half-black HDRI, rule on")
    assert r[("stream", False)]["counters"]["bounce_samples"] == o["counters"]["bounce_samples"]


def test_emission_is_part_of_both_addends():
    """A soup whose material emits: `emission` enters c_vis and c_occ alike, so a live path's two addends differ although neither is
    zero, and a rule that compared the HDRI term alone would be caught here.  Knob on and off, bit for bit, in every schedule."""
    sc = scenes.soup(2000, 48, 36, seed=29, hdri_size=(64, 32))
    sc.materials[0] = abi.default_material(emission=(0.3, 0.2, 0.1))
    sc._desc = None
    r = {(name, every): render_with_knob(sc, 6, 8, flags, every) for name, flags in SCHEDULES.items() for every in (False, True)}
    for key, other in r.items():
        assert_same_result(r[("stream", True)], other, key)
    for every in (False, True):
        assert len({r[(name, every)]["counters"]["rays"] for name in SCHEDULES}) == 1, every
    assert queries(r[("stream", False)]) < queries(r[("stream", True)])
    assert r[("stream", True)]["beauty"][..., :3].max() > 0.0
