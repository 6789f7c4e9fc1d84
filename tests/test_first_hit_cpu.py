"""The mode in which the first-hit pass sees through cut-outs (include/eleven_hip.h er_first_hit_set, er_first_hit_info) on a machine
without a GPU: the symbols and the layouts of ErFirstHitParams and ErFirstHitInfo against the C compiler's, the refusals, both calls on a
scene that is not begun, csrc/er_cutout.h's routines (through er_debug_cutout_*: the functions the kernels call) against their numpy
restatement (elevenrender_amd/first_hit.py) bit for bit on edge values, and the header as a stand-alone program under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np

from elevenrender_amd import abi, first_hit, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)
same = lambda a, b: bool((bits(a) == bits(b)).all())


def test_library_exports_the_entry_points():
    lib = abi.load()
    for name in ("er_first_hit_set", "er_first_hit_info"):
        assert hasattr(lib, name) and name in abi.SYMBOLS, name
    for name in ("er_debug_cutout_threshold", "er_debug_cutout_stops", "er_debug_cutout_continue", "er_debug_first_hit_rays"):
        assert hasattr(lib, name) and name in abi.OPTIONAL_SYMBOLS, name
    assert lib.er_abi_version() == 2         # entry points and two structs were added, none grew


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    structs = {"ErFirstHitParams": abi.ErFirstHitParams, "ErFirstHitInfo": abi.ErFirstHitInfo}
    body = ""
    for name, S in structs.items():
        body += f'  printf("%zu", sizeof({name}));\n' + "".join(f'  printf(" %zu", offsetof({name}, {f}));\n' for f, _ in S._fields_) + '  printf("\\n");\n'
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eleven_hip.h"\nint main(void) {\n' + body +
                   '  printf("%zu %zu %zu\\n", sizeof(ErFeatureInfo), sizeof(ErIdInfo), sizeof(ErPick));\n  return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = [[int(x) for x in l.split()] for l in subprocess.check_output([exe], text=True).splitlines()]
    for got, S in zip(lines, structs.values()):
        assert got == [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
    assert lines[0][0] == 8 and lines[1][0] == 48
    assert lines[2] == [C.sizeof(abi.ErFeatureInfo), C.sizeof(abi.ErIdInfo), C.sizeof(abi.ErPick)] == [24, 40, 40]      # (the consumers' structs did not grow)


def test_refusals_and_a_scene_that_is_not_begun():
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    h = C.c_void_p()
    abi.check(lib.er_scene_create(C.byref(sc.desc()), C.byref(h)))
    INV, STATE = abi.ER_ERR_INVALID_ARG, abi.ER_ERR_STATE
    info = abi.ErFirstHitInfo()
    P = abi.ErFirstHitParams
    buf = np.zeros(3, f32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    ip, up = np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32)), np.zeros(1, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))
    try:
        assert lib.er_first_hit_set(None, C.byref(P(1, 0.0))) == INV and lib.er_first_hit_set(h, None) == INV
        assert lib.er_first_hit_info(None, C.byref(info)) == INV and lib.er_first_hit_info(h, None) == INV
        assert b"NULL" in lib.er_last_error()
        # a threshold that is NaN, negative or above 1 -- and a mode that is neither 0 nor 1 -- is refused, begun or not
        for bad in (float("nan"), -0.25, -1e-30, float(np.nextafter(f32(1), f32(2))), 2.0, float("inf"), float("-inf")):
            assert lib.er_first_hit_set(h, C.byref(P(1, bad))) == INV, bad
            assert b"opacity_threshold" in lib.er_last_error()
            assert lib.er_debug_first_hit_rays(h, fp, fp, 1, bad, ip, up, fp, fp) == INV
        assert lib.er_first_hit_set(h, C.byref(P(2, 0.0))) == INV and b"cutouts" in lib.er_last_error()
        # a created scene that is not begun: a state error from both, whatever the (legal) values
        for ok in (P(0, 0.0), P(1, 0.0), P(1, 0.5), P(1, 1.0), P(1, 1e-30), P(0, -0.0)):
            assert lib.er_first_hit_set(h, C.byref(ok)) == STATE
            assert b"er_render_begin" in lib.er_last_error()
        assert lib.er_first_hit_info(h, C.byref(info)) == STATE and b"er_render_begin" in lib.er_last_error()
        assert lib.er_debug_first_hit_rays(h, fp, fp, 1, 0.0, ip, up, fp, fp) == STATE
        assert lib.er_debug_first_hit_rays(h, None, fp, 1, 0.0, ip, up, fp, fp) == INV
        # the mode is not part of the state
        size = C.c_uint64()
        assert lib.er_state_size(h, C.byref(size)) == abi.ER_OK and size.value == 64 + 16 * 16 * (5 * 16 + 8)
    finally:
        lib.er_scene_destroy(h)
    assert lib.er_debug_cutout_stops(1, None, fp, up) == INV and lib.er_debug_cutout_continue(1, fp, None, fp, fp) == INV
    assert lib.er_debug_cutout_threshold(1, fp, None, fp) == INV and lib.er_debug_cutout_stops(0, None, None, None) == abi.ER_OK


def edge_values():
    nan = np.array([np.nan], f32)
    payload = np.array([0x7FC12345, 0xFFC00001], np.uint32).view(f32)
    e = [0.0, -0.0, 0.5, 1.0, 0.3, 1e-30, -1e-30, -1.5, 2.5, np.inf, -np.inf, 1e-45, -1e-45]
    for c in (0.5, 1.0, 0.3, 1e-30):
        e += [np.nextafter(f32(c), f32(-9)), np.nextafter(f32(c), f32(9))]
    return np.concatenate([np.array(e, f32), nan, payload])


def test_threshold_and_stop_test_equal_the_numpy_restatement_on_edge_values():
    v = edge_values()
    ok, res = abi.debug_cutout_threshold(v)
    assert [bool(x) for x in ok] == [first_hit.threshold_ok(x) for x in v]
    assert same(res, first_hit.threshold(v))
    legal = {float(x) for x in v[ok != 0]}
    assert {0.0, 0.5, 1.0, float(f32(0.3))} <= legal and not any(np.isnan(x) or x < 0 or x > 1 for x in legal)
    assert same(res[v == 0], np.full(2, 0.5, f32)) and same(res[(v != 0) & (ok != 0)], v[(v != 0) & (ok != 0)])
    # every opacity against every resolved threshold: equal to the threshold, +-0, NaN, beyond [0, 1]
    thr = res[ok != 0]
    a, t = np.repeat(v, len(thr)), np.tile(thr, len(v))
    got = abi.debug_cutout_stops(a, t)
    assert (got.astype(bool) == first_hit.stops(a, t)).all()
    assert got[a == t].all() and not got[np.isnan(a)].any()                      # equal stops; a NaN passes
    assert not got[a < 0].any() and not got[(a == 0)].any()                      # (no threshold is 0 once resolved)
    assert got[a > 1].all() and got[np.isposinf(a)].all()
    below = np.nextafter(t, f32(-9))
    assert not abi.debug_cutout_stops(below, t).any()
    # the render's own test u <= opacity with u = threshold agrees wherever neither is NaN
    with np.errstate(invalid="ignore"):
        assert (got.astype(bool) == (t <= a)).all()


def test_the_continuation_equals_the_numpy_restatement():
    rng = np.random.default_rng(3)
    p = rng.uniform(-5, 5, (4000, 3)).astype(f32)
    d = rng.normal(size=(4000, 3)).astype(f32)
    d[:2000] /= np.linalg.norm(d[:2000], axis=1, keepdims=True).astype(f32)          # unit to rounding, as the camera's are
    d[0] = 0                                                                      # a zero direction is kept
    d[1] = (0, 0, 1)
    d[2] = (1e-30, 0, 0)                                                          # its square underflows: length 0, kept too
    p[4] = (np.inf, 0, 0)
    go, gd = abi.debug_cutout_continue(p, d)
    wo, wd = first_hit.continuation(p, d)
    assert same(go, wo) and same(gd, wd)
    assert same(gd[0], d[0]) and same(gd[1], d[1]) and same(gd[2], d[2])
    assert same(go[1], p[1] + d[1] * f32(0.001))
    # normalising again is not always the identity on a unit vector: that is why the routine keeps the quotient
    assert 0 < (bits(gd[5:2000]) != bits(d[5:2000])).any(1).sum()
    assert np.allclose(np.linalg.norm(gd[5:], axis=1), 1, atol=1e-6)


def test_host_routines_under_sanitizers(tmp_path):
    """tests/native/cutout_host.cpp: er_cutout.h alone with ASan + UBSan, on heap arrays of exactly three floats"""
    exe = str(tmp_path / "cutout_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "elevenrender_amd", "csrc"), os.path.join(ROOT, "tests", "native", "cutout_host.cpp"), "-o", exe])
    out = subprocess.run([exe], text=True, capture_output=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cutout_host ok" in out.stdout
