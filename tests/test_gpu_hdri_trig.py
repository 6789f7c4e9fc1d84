"""The row and column tables of the HDRI's next-event sample directions (csrc/er_hdri_trig.h) change no bit of any result.

The bounce step (csrc/er_bounce.inc) reads the sampled texel's cos(phi - pi), sin(phi - pi), cos(theta) and the sine of HDRI::pdf from
a width + height table that one kernel fills at er_render_begin -- and again when er_render_edit replaces the HDRI -- by calling the
device functions the step would call.  ER_HDRI_TRIG_ON_DEVICE=1 (read by er_render_begin) leaves the table unused and the kernels
evaluate.  Checked here: (a) planes, sample counts, RNG states and event counters are the same bits with the knob on and off in the
streaming, wavefront and megakernel schedules, and equal the oracle's; (b) an edit from a 6x4 to a 7x5 HDRI leaves what a fresh begin
with the 7x5 one gives; (c) the table read back from the device equals er_debug_eval of the same functions on every row and column,
bit for bit (NaN = NaN).
"""
import os

import numpy as np
import pytest

from elevenrender_amd import abi, render, scenes
from test_gpu_parity import compare, gpu_render

pytestmark = pytest.mark.gpu

PLANES = ("beauty", "denoise", "normal", "tangent", "bitangent")
COUNTS = ("paths", "bounce_samples", "rays", "shaded_hits", "hdri_samples")
SCHEDULES = {"stream": abi.FLAG_STREAM, "wavefront": abi.FLAG_WAVEFRONT, "megakernel": abi.FLAG_MEGAKERNEL}
KNOB = "ER_HDRI_TRIG_ON_DEVICE"
PIF = np.float32(3.14159265358979323846)
FN_REV_SPHERICAL, FN_MATH = 7, 11      # include/eleven_hip_debug.h ER_FN_*
# (width, height, zero-luminance row or None)
HDRIS = {"1x1": (1, 1, None), "2x1": (2, 1, None), "6x4": (6, 4, None), "7x5": (7, 5, None), "64x32": (64, 32, None), "6x4_zero_row": (6, 4, 1)}
CASES = {"one_bounce": (1, 0), "eight_bounces": (8, 0), "mis": (8, abi.FLAG_MIS)}


def make_hdri(name):
    w, h, zero = HDRIS[name]
    data = abi._f32(0.2 + 2.0 * scenes.Rand(91, 7).u01(h, w, 3))
    if zero is not None:
        data[zero] = 0.0
    return (np.ascontiguousarray(data), w, h, 3, 0)


def make_scene(kind, hdri_name):
    sc = scenes.cornell(32, 24) if kind == "cornell" else scenes.soup(2000, 32, 24, seed=23, hdri_size=(64, 32))
    sc.hdri = make_hdri(hdri_name)
    sc.hdri_cdf = None
    sc._desc = None
    return sc


def render_with_knob(sc, spp, max_bounces, flags, on_device):
    """One render with the knob set (on_device = True: no table) or unset; the environment is left as it was found."""
    before = os.environ.pop(KNOB, None)
    try:
        if on_device:
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


def oracle_result(oracle_mod, sc, spp, max_bounces, flags):
    o = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, max_bounces=max_bounces, threads=8, flags=flags)
    o.render(spp)
    out = {name: o.read_pass(p) for name, p in abi.PASS_NAMES.items()}
    out["samples"], out["rng"], out["counters"] = o.read_samples(), o.read_rng(), o.counters()
    o.close()
    return out


@pytest.mark.parametrize("kind", ["cornell", "soup"])
@pytest.mark.parametrize("hdri_name", list(HDRIS))
def test_table_and_evaluation_give_the_same_bits_and_the_oracles(oracle_mod, hdri_name, kind):
    """32x24, 4 samples; 1 bounce, 8 bounces and 8 bounces with ER_FLAG_MIS: the three schedules with and without the table are one
    result, and that result is the oracle's (soup: every pixel; Cornell: the allowance the other Cornell parity tests make for exact
    distance ties on the walls' shared edges, 0.999 of the pixels -- at 768 pixels that is every pixel too)."""
    sc = make_scene(kind, hdri_name)
    for case, (mb, ext) in CASES.items():
        ref = render_with_knob(sc, 4, mb, abi.FLAG_STREAM | ext, False)
        for name, flags in SCHEDULES.items():
            for on_device in (False, True):
                if name == "stream" and not on_device:
                    continue
                assert_same_result(ref, render_with_knob(sc, 4, mb, flags | ext, on_device), (hdri_name, kind, case, name, on_device))
        o = oracle_result(oracle_mod, sc, 4, mb, ext)
        compare(ref, o, min_exact=1.0 if kind == "soup" else 0.999, what=f"{kind}, HDRI {hdri_name}, {case}")
        for k in ("bounce_samples", "shaded_hits", "hdri_samples"):
            assert ref["counters"][k] == o["counters"][k], (hdri_name, kind, case, k)


def test_count_minus_one_is_evaluated_not_looked_up(oracle_mod):
    """An HDRI whose first texels are black: the reference's search can end at -1 for a small draw, which is no texel of the table; the
    step then evaluates as it always did.  Bits equal with the knob on and off and to the oracle."""
    sc = scenes.soup(2000, 32, 24, seed=23, hdri_size=(64, 32))
    data = make_hdri("6x4")[0].copy()
    data[0, :3] = 0.0
    sc.hdri = (np.ascontiguousarray(data), 6, 4, 3, 0)
    sc.hdri_cdf = None
    sc._desc = None
    a, b = render_with_knob(sc, 4, 8, abi.FLAG_STREAM, False), render_with_knob(sc, 4, 8, abi.FLAG_STREAM, True)
    assert_same_result(a, b, "black first texels")
    compare(a, oracle_result(oracle_mod, sc, 4, 8, 0), min_exact=1.0, what="soup, black first texels")


def read_state(rm):
    out = {p: rm.get_pass(p) for p in PLANES}
    out["samples"], out["rng"], out["counters"] = rm.read_samples(), rm.read_rng(), rm.counters()
    return out


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_an_edited_hdri_gets_a_new_table(schedule):
    """er_render_edit replaces a 6x4 HDRI by a 7x5 one on a begun scene: the render and the table equal a fresh begin's with the 7x5 one."""
    old, new = make_scene("soup", "6x4"), make_scene("soup", "7x5")
    params = dict(max_bounces=8, flags=SCHEDULES[schedule] | abi.FLAG_MIS)
    rm = render.RenderingManager(render.RenderParameters(**params))
    rm.start_rendering(old)
    rm.render(2)
    rm.edit(hdri=new.hdri)
    rm.render(4)
    edited, edited_tab = read_state(rm), rm.debug_hdri_trig(7, 5)
    rm.close()
    rm = render.RenderingManager(render.RenderParameters(**params))
    rm.start_rendering(new)
    rm.render(4)
    fresh, fresh_tab = read_state(rm), rm.debug_hdri_trig(7, 5)
    rm.close()
    assert_same_result(edited, fresh, schedule)
    for a, b in zip(edited_tab, fresh_tab):
        assert (a == b).all()


def f2i(x):
    """ermath::f2i on float32 arrays: truncation, INT_MIN out of range."""
    x = np.asarray(x, np.float32)
    ok = (x >= np.float32(-2147483648.0)) & (x < np.float32(2147483648.0))
    return np.where(ok, np.where(ok, x, 0).astype(np.int64), -2147483648).astype(np.int32)


def limit_uv(u):
    return (u + (-(u > 1).astype(np.int32) - (u < 0).astype(np.int32)).astype(np.float32)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits_or_nan(got_words, want_f32):
    got = np.ascontiguousarray(got_words, np.uint32).view(np.float32)
    want = np.ascontiguousarray(want_f32, np.float32)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


@pytest.mark.parametrize("hdri_name", list(HDRIS))
def test_table_entries_are_the_device_functions_values(hdri_name):
    """Every column and row of the table read back from the device against er_debug_eval of er_sin / er_cos
    (ER_FN_MATH) and reverse_spherical_mapping (ER_FN_REV_SPHERICAL) on the arguments the bounce step forms: zero bits differ."""
    w, h, _ = HDRIS[hdri_name]
    rm = render.RenderingManager(render.RenderParameters(max_bounces=2))
    rm.start_rendering(make_scene("cornell", hdri_name))
    cols, rows = rm.debug_hdri_trig(w, h)

    def math(op, x):
        items = np.zeros((len(x), 3), np.float32)
        items[:, 0] = np.full(len(x), op, np.int32).view(np.float32)
        items[:, 1] = x
        return rm.debug_eval(FN_MATH, items, 1)[:, 0]

    fw, fh = np.float32(w), np.float32(h)
    x, y = np.arange(w, dtype=np.int32), np.arange(h, dtype=np.int32)
    iu = limit_uv(f2i((x.astype(np.float32) / fw) * fw).astype(np.float32) / fw)      # inverse_transform_uv
    iv = limit_uv(f2i((y.astype(np.float32) / fh) * fh).astype(np.float32) / fh)
    arg = ((iu * np.float32(2)) * PIF - PIF).astype(np.float32)
    theta = (iv * PIF).astype(np.float32)
    iy = f2i(iv * fh)
    py = -math(1, theta)
    want_cols = {0: math(1, arg), 1: -math(0, arg), 3: iu}
    want_rows = {0: py, 1: np.sqrt(np.float32(1) - py * py, dtype=np.float32), 3: math(0, (iy.astype(np.float32) / fh) * PIF), 4: iv,
                 5: math(0, (y.astype(np.float32) / fh) * PIF)}
    for k, v in want_cols.items():
        assert same_bits_or_nan(cols[:, k], v).all(), (hdri_name, "column word", k)
    for k, v in want_rows.items():
        assert same_bits_or_nan(rows[:, k], v).all(), (hdri_name, "row word", k)
    assert (cols[:, 2].view(np.int32) == f2i(iu * fw)).all() and (rows[:, 2].view(np.int32) == iy).all()
    # the whole direction, texel by texel: reverse_spherical_mapping(iu, iv) = (a px, py, a pz)
    gx, gy = np.meshgrid(x, y)
    gx, gy = gx.reshape(-1), gy.reshape(-1)
    want = rm.debug_eval(FN_REV_SPHERICAL, np.stack([iu[gx], iv[gy]], 1), 3)
    cf, rf = cols.view(np.float32), rows.view(np.float32)
    got = np.stack([rf[gy, 1] * cf[gx, 0], rf[gy, 0], rf[gy, 1] * cf[gx, 1]], 1).astype(np.float32)
    assert ((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(), hdri_name
    rm.close()
