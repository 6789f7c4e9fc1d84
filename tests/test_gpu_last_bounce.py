"""No continuation on a path's last iteration (csrc/er_bounce.inc).

When `bounce + 1 >= max_bounces` the bounce step still takes its three BRDF draws but no longer computes DisneySample, DisneyPdf and
DisneyEval of the sampled direction, the `reduction` and `prev_pdf` updates and the new ray: they went to variables nothing reads once
the path is done.  The result must not move: planes, RNG states, sample counts and counters against the oracle (which computes all of
it) in the three schedules, and the per-bounce records of er_debug_trace_pixel -- whose kernel keeps the full computation
(ER_BOUNCE_KEEP_LAST), since its records carry the next direction and the throughput -- against the oracle's.
"""
import numpy as np
import pytest

from elevenrender_amd import abi, render, scenes
from test_gpu_function_level import _rec_tuple
from test_gpu_parity import compare, gpu_render

pytestmark = pytest.mark.gpu

PLANES = ("beauty", "denoise", "normal", "tangent", "bitangent")
COUNTS = ("paths", "bounce_samples", "rays", "shaded_hits", "hdri_samples")
SCHEDULES = {"stream": abi.FLAG_STREAM, "wavefront": abi.FLAG_WAVEFRONT, "megakernel": abi.FLAG_MEGAKERNEL}
CASES = [("cornell", 1), ("cornell", 2), ("cornell", 5), ("soup", 1), ("soup", 2), ("soup", 5), ("textured", 16)]


def make_scene(kind):
    if kind == "cornell":
        return scenes.cornell(32, 24)
    if kind == "soup":
        return scenes.soup(2000, 32, 24, seed=23, hdri_size=(64, 32))
    return scenes.torture(3000, 16, 12, seed=5, n_materials=8, tex_size=16, hdri_size=(128, 64), n_lights=0)


@pytest.fixture(scope="module")
def oracles(oracle_mod):
    """One oracle per case, rendered once (4 samples) and read by both tests; the trace test goes on from that state."""
    made = {}

    def get(kind, mb):
        if (kind, mb) not in made:
            o = oracle_mod.Oracle(make_scene(kind), math_mode=oracle_mod.MATH_ER, max_bounces=mb, threads=8)
            o.render(4)
            snap = {name: o.read_pass(p) for name, p in abi.PASS_NAMES.items()}
            snap["samples"], snap["rng"], snap["counters"] = o.read_samples(), o.read_rng(), o.counters()
            made[(kind, mb)] = (o, snap)      # (the snapshot is what the image test reads: the trace test advances the oracle)
        return made[(kind, mb)]

    yield get
    for o, _ in made.values():
        o.close()


@pytest.mark.parametrize("kind,mb", CASES)
def test_images_and_counts_equal_the_oracles_in_every_schedule(oracles, kind, mb):
    """4 samples.  Soup and the textured scene: every pixel bit-exact; Cornell: the other Cornell parity tests' allowance for exact
    distance ties on the walls' shared edges (0.999 of the pixels).  The schedules among themselves: every bit and every counter."""
    sc = make_scene(kind)
    o = oracles(kind, mb)[1]
    r = {name: gpu_render(sc, 4, max_bounces=mb, flags=flags) for name, flags in SCHEDULES.items()}
    for name, g in r.items():
        compare(g, o, min_exact=0.999 if kind == "cornell" else 1.0, what=f"{kind}, {mb} bounces, {name}")
        for k in ("bounce_samples", "shaded_hits", "hdri_samples"):
            assert g["counters"][k] == o["counters"][k], (kind, mb, name, k)
    for name in ("wavefront", "megakernel"):
        for p in PLANES:
            assert (r[name][p].view(np.uint32) == r["stream"][p].view(np.uint32)).all(), (kind, mb, name, p)
        assert (r[name]["rng"] == r["stream"]["rng"]).all() and (r[name]["samples"] == r["stream"]["samples"]).all(), (kind, mb, name)
        for k in COUNTS:
            assert r[name]["counters"][k] == r["stream"]["counters"][k], (kind, mb, name, k)


@pytest.mark.parametrize("kind,mb", CASES)
def test_trace_records_are_unchanged_against_the_oracle(oracles, kind, mb):
    """The fifth sample of 40 pixels, record by record -- the last iteration's next direction and throughput among them."""
    sc = make_scene(kind)
    orc = oracles(kind, mb)[0]
    rm = render.RenderingManager(render.RenderParameters(max_bounces=mb))
    rm.start_rendering(sc)
    rm.render(4)
    pixels = np.random.default_rng(11).choice(sc.x_res * sc.y_res, 40, replace=False)
    n_rec = n_last = n_bad = 0
    for idx in pixels:
        g = rm.debug_trace_pixel(int(idx), max_recs=32)
        o = orc.trace_pixel(int(idx), max_recs=32)
        assert len(g) == len(o), (idx, len(g), len(o))
        for a, b in zip(g, o):
            n_rec += 1
            n_last += int(a.bounce + 1 >= mb and a.opaque != 0)
            traced = a.shadow_occ >= 0      # (a query whose BRDF term is exactly zero is not traced by the kernels: no shadow fields)
            n_bad += int(_rec_tuple(a, traced) != _rec_tuple(b, traced))
    print(f"{kind}, {mb} bounces: {n_rec} records, {n_last} of opaque last iterations, {n_bad} differ")
    assert n_last > 0 or mb > 5      # (few paths of the textured scene live for 16 iterations: its records are compared, a last one is not required)
    assert n_bad <= (2 if kind == "cornell" else 0)            # cornell: exact ties on the walls' shared edges
    rm.close()
