"""Paths of 24 to 1 001 iterations in every schedule, against the oracle and against each other, on bits.

No other test renders with more than 16 bounces, and several fields the kernels pack have their edges above that (DESIGN.md "Parity"):
   24 / 25    127 guessed draws, 5 + hits + 4 * opaque (csrc/er_stream.hip ST_DRAWS_MASK); with point lights (5 per opaque hit) 20 / 21,
              with mesh lights (7) 15 / 16 -- the 2-shell scene at 32 bounces puts pixels on both sides of each
   32         mean path length x 16 against its clamp at 511 (ST_LONG_SHIFT)
   42 / 43    long_thr = max_bounces * 12 switched off above 511 (er_stream_launch_form, the 12-wave form)
   200        a length no tally, field or stack of the suite has seen; the builders and the per-bounce records run there
   1000/1001  three 10-bit per-sample tallies added in one atomic (tally_a); form 2 is taken only up to 1 000
The scenes are tests/long_path_scenes.py: in 64 concentric shells every path runs exactly max_bounces iterations, in 2 shells the lengths
spread over 1 .. max_bounces; tests/test_long_path_scenes_cpu.py shows both on the oracle alone, and that the oracle's two traversal orders
agree on every bit of them -- there are no exact-distance ties, so every comparison here asks for EVERY pixel (min_exact = 1.0).

What these found: with ER_FLAG_COUNTERS the wavefront schedule's shading kernel summed the node visits and triangle tests of its exact
re-traces (a ray with more than two candidates inside one t-interval -- rare in a soup, common between walls 0.05 apart) and never added
them to the counters, so its node_visits and tri_tests fell short of the streaming schedule's by 0.01 ... 0.04 % on both shell scenes.
The instrumented comparisons below (speculation, long_thr, the gate) hold the two schedules to each other in these counters too.

ER_MAX_BOUNCES: nothing here renders above it; the range beyond is tested by refusals that launch nothing (and tests/test_abi_cpu.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import accel_check
import long_path_scenes as lps
from elevenrender_amd import abi, render, scenes

from test_gpu_function_level import _rec_tuple
from test_gpu_parity import compare
from test_gpu_stream_handoff import COUNTS, KNOBS, assert_no_bit_differs

pytestmark = pytest.mark.gpu

PLANES = ("beauty", "denoise", "normal", "tangent", "bitangent")
SCHEDULES = {"wavefront": abi.FLAG_WAVEFRONT, "megakernel": abi.FLAG_MEGAKERNEL, "stream": abi.FLAG_STREAM}
POINT, MESH = abi.FLAG_POINT_LIGHTS | abi.FLAG_MIS, abi.FLAG_MESH_LIGHTS | abi.FLAG_MIS
LIGHTING = {"plain": ("plain", 0), "point-lights": ("point", POINT), "mesh-lights": ("plain", MESH)}      # name: (scene kind, flags)
SPP = 3      # (1 001 bounces x 3 spp of the wavefront host loop is 6 012 launches, well under a second: no case drops to 2 spp)


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def scene(kind, n_shells):
    """64 shells at 16 x 12 (the oracle is involved), 2 shells at 160 x 120 (300 tiles: every workgroup of the streaming kernel owns one)"""
    x, y = (16, 12) if n_shells == 64 else (160, 120)
    return lps.shells(x, y, n_shells) if kind == "plain" else lps.shells_point_lights(x, y, n_shells)


def gpu(sc, chunks, flags, mb):
    rm = render.RenderingManager(render.RenderParameters(max_bounces=mb, flags=flags))
    rm.start_rendering(sc)
    for n in chunks:
        rm.render(n)
    out = {p: rm.get_pass(p) for p in PLANES}
    out["samples"], out["rng"], out["counters"] = rm.read_samples(), rm.read_rng(), rm.counters()
    out["stream"] = rm.stream_info() if flags & abi.FLAG_STREAM else None
    out["order"] = rm.debug_light_table()[0] if flags & abi.FLAG_MESH_LIGHTS else np.zeros(0, np.int32)
    rm.close()
    return out


_gpu_frames, _oracle_frames = {}, {}


def gpu_64(lighting, schedule, mb, chunks=(SPP,), builder=0):
    """one render of the 64-shell scene without knobs, made once and left unchanged"""
    key = (lighting, schedule, mb, chunks, builder)
    if key not in _gpu_frames:
        kind, flags = LIGHTING[lighting]
        _gpu_frames[key] = gpu(scene(kind, 64), chunks, flags | SCHEDULES[schedule] | builder, mb)
    return _gpu_frames[key]


def oracle_64(oracle_mod, lighting, mb, order=()):
    """the oracle's frame after SPP samples (for mesh lights: with the emitter order of the device's table), made once"""
    order = np.ascontiguousarray(order, np.int32)
    key = (lighting, mb, order.tobytes())
    if key not in _oracle_frames:
        kind, flags = LIGHTING[lighting]
        orc = oracle_mod.Oracle(scene(kind, 64), math_mode=oracle_mod.MATH_ER, max_bounces=mb, threads=8, flags=flags)
        if flags & abi.FLAG_MESH_LIGHTS:
            orc.set_emitters(order)
        orc.render(SPP)
        out = {p: orc.read_pass(abi.PASS_NAMES[p]) for p in PLANES}
        out["samples"], out["rng"], out["counters"] = orc.read_samples(), orc.read_rng(), orc.counters()
        orc.close()
        for p in PLANES + ("samples", "rng"):
            out[p].setflags(write=False)
        _oracle_frames[key] = out
    return _oracle_frames[key]


def assert_equals_oracle(g, o, mb, what):
    compare(g, o, min_exact=1.0, what=what)
    for k in ("bounce_samples", "shaded_hits", "hdri_samples"):
        assert g["counters"][k] == o["counters"][k] == 16 * 12 * SPP * mb, (what, k, g["counters"][k], o["counters"][k])
    assert g["counters"]["paths"] == o["counters"]["paths"] == 16 * 12 * SPP


EDGE_CASES = [("plain", mb) for mb in (24, 25, 32, 43, 200, 1000, 1001)] + [("point-lights", 25), ("point-lights", 200), ("mesh-lights", 25), ("mesh-lights", 200)]


@pytest.mark.parametrize("lighting,mb", EDGE_CASES, ids=[f"{l}-{mb}" for l, mb in EDGE_CASES])
def test_every_schedule_equals_the_oracle_at_the_edges(oracle_mod, lighting, mb):
    """64 shells, 16 x 12, 3 spp: each schedule against the oracle in every pixel and in bounce_samples, shaded_hits and hdri_samples
    (all paths x max_bounces: every iteration of every path is a shaded opaque hit); among the schedules every plane, RNG state, sample
    count and all five event counters."""
    frames = {name: gpu_64(lighting, name, mb) for name in SCHEDULES}
    for name, g in frames.items():
        if lighting == "mesh-lights":
            assert len(g["order"]) == 2 * 64 and (g["order"] == frames["wavefront"]["order"]).all()
        assert_equals_oracle(g, oracle_64(oracle_mod, lighting, mb, g["order"]), mb, f"{lighting} max_bounces {mb} {name}")
    for name in ("megakernel", "stream"):
        assert_no_bit_differs(frames[name], frames["wavefront"], (lighting, mb, name))
    assert frames["wavefront"]["counters"]["rays"] > 16 * 12 * SPP * mb      # (shadow queries were traced as well)


@pytest.mark.parametrize("builder", ["host-build", "gpu-build"])
def test_both_builders_at_200_bounces(oracle_mod, builder):
    """64 nested boxes of scene-sized triangles around 1 200 small ones is a tree shape no other test has: the structure each builder
    left in device memory under tests/accel_check.py, and the image through it against the oracle in every schedule."""
    flag = {"host-build": abi.FLAG_HOST_BUILD, "gpu-build": abi.FLAG_GPU_BUILD}[builder]
    sc = scene("plain", 64)
    rm = render.RenderingManager(render.RenderParameters(max_bounces=200, flags=flag))
    rm.start_rendering(sc)
    dump, info = rm.debug_read_accel(), rm.accel_info()
    rm.close()
    assert info["builder"] == (1 if builder == "gpu-build" else 0) and dump["tri_count"] == sc.tri_count
    rep = accel_check.check(sc, dump, accel_depth=info["max_depth"])
    print(f"{builder}: {dump['node_count']} binary nodes (depth {rep.depth2}), {dump['node8_count']} wide nodes (depth {rep.depth8})")
    assert rep.ok, rep.message()
    for name in SCHEDULES:
        assert_equals_oracle(gpu_64("plain", name, 200, builder=flag), oracle_64(oracle_mod, "plain", 200), 200, f"{builder} {name}")


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_chunked_equals_one_call_at_200_bounces(schedule):
    a, b = gpu_64("plain", schedule, 200), gpu_64("plain", schedule, 200, chunks=(1, 2))
    assert_no_bit_differs(b, a, ("chunks 1 + 2", schedule))


@pytest.mark.parametrize("lighting", list(LIGHTING))
def test_per_bounce_records_at_200_bounces(oracle_mod, lighting):
    """er_debug_trace_pixel against Oracle.trace_pixel: 12 pixels after 2 rendered samples, every field of every one of the 200 records.
    Throughput dies after a few dozen iterations (the rest are dead paths that still trace and draw): both kinds are compared."""
    kind, flags = LIGHTING[lighting]
    sc, mb = scene(kind, 64), 200
    rm = render.RenderingManager(render.RenderParameters(max_bounces=mb, flags=flags | abi.FLAG_HOST_BUILD))
    rm.start_rendering(sc)
    orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, max_bounces=mb, threads=1, flags=flags)
    if flags & abi.FLAG_MESH_LIGHTS:
        order = rm.debug_light_table()[0]
        assert (order == lps.emitter_order(sc)).all()
        orc.set_emitters(order)
    rm.render(2)
    orc.render(2)
    n_rec = n_bad = n_dead = n_live = 0
    for idx in lps.traced_pixels(sc, 12):
        g = rm.debug_trace_pixel(int(idx), max_recs=mb + 2)
        o = orc.trace_pixel(int(idx), max_recs=mb + 2)
        assert len(g) == len(o) == mb, (idx, len(g), len(o))
        for a, b in zip(g, o):
            n_rec += 1
            traced = a.shadow_occ >= 0      # (the kernels skip an HDRI shadow ray whose outcomes add the same value)
            same = _rec_tuple(a, traced) == _rec_tuple(b, traced)
            n_bad += int(not same)
            if not same and n_bad <= 3:
                print("pixel", idx, "bounce", a.bounce, _rec_tuple(a, traced), "!=", _rec_tuple(b, traced))
            dead = all(v == 0.0 for v in b.reduction)
            n_dead += int(same and dead)
            n_live += int(same and not dead)
    print(f"{lighting}: {n_rec} records, {n_bad} differ; {n_live} with live throughput, {n_dead} with dead")
    assert n_bad == 0 and n_live > 0 and n_dead > 0
    img, ref = rm.get_pass("beauty"), orc.read_pass(0)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()
    assert (rm.read_samples() == orc.read_samples()).all() and (rm.read_rng() == orc.read_rng()).all()
    rm.close()
    orc.close()


def stream_and_wavefront(sc, flags, mb, chunks):
    return gpu(sc, chunks, flags | abi.FLAG_STREAM, mb), gpu(sc, chunks, flags | abi.FLAG_WAVEFRONT, mb)


@pytest.mark.parametrize("lighting", ["plain", "point-lights"])
@pytest.mark.parametrize("waves", [12, 16])
def test_speculation_across_the_draw_count_edge(lighting, waves, monkeypatch):
    """2 shells, 160 x 120, 32 bounces, 12 spp in calls of 5 and 7, the speculative form forced: samples draw fewer and more than 127
    numbers (about a third of the pixels more), so guesses are made, kept, missed and given up ("no guess") side by side.  The streaming
    render equals the wavefront render in every bit and counter, plain and with ER_FLAG_COUNTERS; how many guesses were right and wrong
    is a scheduling outcome -- printed, and asserted only in that both kinds occurred."""
    monkeypatch.setenv("ER_STREAM_SPEC_FORM", "1")
    monkeypatch.setenv("ER_STREAM_WAVES", str(waves))
    kind, flags = LIGHTING[lighting]
    sc = scene(kind, 2)
    for count in (0, abi.FLAG_COUNTERS):
        s, w = stream_and_wavefront(sc, flags | count, 32, (5, 7))
        si = s["stream"]
        print(f"{lighting}, {waves} waves, counters {count}: speculative samples started {si['spec_started']}, right {si['spec_right']}, wrong {si['spec_wrong']}")
        assert (si["form"], si["waves"]) == (2, waves), si
        assert_no_bit_differs(s, w, (lighting, waves, count), instrumented=count != 0)
        assert s["counters"]["paths"] == 160 * 120 * 12
        assert si["spec_right"] > 0 and si["spec_wrong"] > 0 and si["spec_started"] >= si["spec_right"] + si["spec_wrong"], si


@pytest.mark.parametrize("mb", [42, 43])
def test_long_pixel_threshold_on_and_off(mb, monkeypatch):
    """12 waves: long_thr = 12 * max_bounces is 504 at 42 bounces (pixels whose paths average 31.5 iterations always start a successor)
    and 516 at 43, which the 9-bit field cannot hold: switched off.  Image and counters against the wavefront schedule."""
    monkeypatch.setenv("ER_STREAM_SPEC_FORM", "1")
    monkeypatch.setenv("ER_STREAM_WAVES", "12")
    s, w = stream_and_wavefront(scene("plain", 2), abi.FLAG_COUNTERS, mb, (5, 7))
    si = s["stream"]
    print(f"max_bounces {mb}: speculative samples started {si['spec_started']}, right {si['spec_right']}, wrong {si['spec_wrong']}")
    assert (si["form"], si["waves"]) == (2, 12), si
    assert_no_bit_differs(s, w, ("long_thr", mb), instrumented=True)


@pytest.mark.parametrize("mb", [1000, 1001])
def test_the_gate_of_the_speculative_form_at_1000_bounces(oracle_mod, mb, monkeypatch):
    """The speculative form adds a sample's iterations, shaded hits and HDRI samples as three 10-bit fields of one word: at 1 000 bounces in
    64 shells each of them is exactly 1 000 for every sample.  At 1 001 the launcher must not take that form, even when asked to."""
    monkeypatch.setenv("ER_STREAM_SPEC_FORM", "1")
    s, w = stream_and_wavefront(scene("plain", 64), abi.FLAG_COUNTERS, mb, (SPP,))
    si = s["stream"]
    print(f"max_bounces {mb}: form {si['form']}, {si['waves']} waves; speculative samples started {si['spec_started']}, right {si['spec_right']}, wrong {si['spec_wrong']}")
    assert (si["form"] == 2) == (mb == 1000), si
    assert_no_bit_differs(s, w, ("gate", mb), instrumented=True)
    o = oracle_64(oracle_mod, "plain", mb)
    for g in (s, w):
        assert_equals_oracle(g, o, mb, f"gate {mb}")


def test_max_bounces_0_means_5():
    """in 64 shells every path runs as many iterations as the limit allows: exactly 5 with max_bounces 0, in every schedule"""
    sc = scene("plain", 64)
    for name, flag in SCHEDULES.items():
        a, b = gpu(sc, (SPP,), flag, 0), gpu(sc, (SPP,), flag, 5)
        assert_no_bit_differs(a, b, ("max_bounces 0 and 5", name))
        assert a["counters"]["bounce_samples"] == 16 * 12 * SPP * 5, name


def test_max_bounces_above_the_limit_and_wrapping_iteration_counts_are_refused():
    """Refusals only, nothing is launched: er_render_begin above ER_MAX_BOUNCES on a machine WITH a device, and a call of the wavefront
    schedule whose n * (max_bounces + 1) iterations do not fit 32 bits (65 536 x 65 536 = 2^32, which wrapped to 0 iterations)."""
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    h = C.c_void_p()
    abi.check(lib.er_scene_create(C.byref(sc.desc()), C.byref(h)))
    try:
        for mb in (abi.MAX_BOUNCES + 1, 0xFFFFFFFF):
            p = abi.ErRenderParams(16, 8, mb, 0, 0, 1, abi.FLAG_WAVEFRONT)
            assert lib.er_render_begin(h, C.byref(p)) == abi.ER_ERR_INVALID_ARG
            assert b"ER_MAX_BOUNCES" in lib.er_last_error()
            assert lib.er_render_samples(h, 1) == abi.ER_ERR_STATE
        p = abi.ErRenderParams(16, 8, abi.MAX_BOUNCES, 0, 0, 1, abi.FLAG_WAVEFRONT)
        abi.check(lib.er_render_begin(h, C.byref(p)))
        done, counters = C.c_uint32(), abi.ErCounters()
        for n in (65536, 65537, 0xFFFFFFFF):
            assert lib.er_render_samples(h, n) == abi.ER_ERR_INVALID_ARG, n
            assert b"iterations" in lib.er_last_error()
            abi.check(lib.er_samples_done(h, C.byref(done)))
            abi.check(lib.er_get_counters(h, C.byref(counters)))
            assert done.value == 1 and counters.paths == 0      # (1: the count starts at the setup sample; nothing was rendered)
        abi.check(lib.er_render_samples(h, 0))                  # (the scene is still usable: no samples is no iterations)
    finally:
        lib.er_scene_destroy(h)
