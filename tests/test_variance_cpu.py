"""The variance plane and the filter guided by it (include/eleven_hip.h er_variance_fold, er_variance_info, er_read_variance,
er_denoise_variance) on a machine without a GPU: the symbols, the struct layouts against the C compiler's, the argument and call-order
errors that need no device, the header's routines (csrc/er_variance.h through er_debug_variance_*: the functions the kernels call)
against their numpy restatement (elevenrender_amd/variance.py) word for word, the estimator's unbiasedness on synthetic pixels driven
through the reference's running-mean recurrence, and the header as a stand-alone program under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from elevenrender_amd import abi, scenes, variance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("er_variance_fold", "er_variance_info", "er_read_variance", "er_denoise_variance")
DEBUG = ("er_debug_variance_mark", "er_debug_variance_fold", "er_debug_variance_value", "er_debug_variance_split", "er_debug_variance_level_px")
f32 = np.float32
bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)


def test_library_exports_the_variance_entry_points():
    lib = abi.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in abi.SYMBOLS, name
    for name in DEBUG:
        assert hasattr(lib, name), name
    assert lib.er_abi_version() == 2          # entry points and structs were added, none grew
    assert abi.FEATURE_COUNT == 2 and abi.PASS_COUNT == 5


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    src = tmp_path / "sizes.c"
    fi = ("folds", "reserved", "pixels_folded", "pixels_known", "fold_ms", "filter_ms")
    fd = ("levels", "colour_sigma", "albedo_sigma", "depth_sigma")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eleven_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(ErVarianceInfo), sizeof(ErDenoiseVariance));\n'
                   + "".join(f'  printf(" %zu", offsetof(ErVarianceInfo, {f}));\n' for f in fi)
                   + "".join(f'  printf(" %zu", offsetof(ErDenoiseVariance, {f}));\n' for f in fd) + '  printf("\\n"); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    I, D = abi.ErVarianceInfo, abi.ErDenoiseVariance
    assert got == [C.sizeof(I), C.sizeof(D)] + [getattr(I, f).offset for f in fi] + [getattr(D, f).offset for f in fd]
    assert C.sizeof(I) == 32 and C.sizeof(D) == 16


def test_arguments_and_call_order_without_a_device():
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    h = C.c_void_p()
    abi.check(lib.er_scene_create(C.byref(sc.desc()), C.byref(h)))
    plane = np.zeros(16 * 16 * 4, f32)
    fp = plane.ctypes.data_as(C.POINTER(C.c_float))
    info, par = abi.ErVarianceInfo(), abi.ErDenoiseVariance(0, 0.0, 0.0, 0.0)
    INV, STATE = abi.ER_ERR_INVALID_ARG, abi.ER_ERR_STATE
    try:
        # NULL arguments
        assert lib.er_variance_fold(None) == INV
        assert lib.er_variance_info(None, C.byref(info)) == INV and lib.er_variance_info(h, None) == INV
        assert lib.er_read_variance(None, fp) == INV and lib.er_read_variance(h, None) == INV
        assert lib.er_denoise_variance(None, C.byref(par)) == INV and lib.er_denoise_variance(h, None) == INV
        assert b"NULL" in lib.er_last_error()
        # parameters out of range, begun or not
        for bad in ((9, 0.0, 0.0, 0.0), (0, -1.0, 0.0, 0.0), (0, 0.0, -0.1, 0.0), (0, 0.0, 0.0, -2.0), (0, float("nan"), 0.0, 0.0), (0, 0.0, 0.0, float("nan"))):
            assert lib.er_denoise_variance(h, C.byref(abi.ErDenoiseVariance(*bad))) == INV, bad
        # a created scene that is not begun: a state error from all four
        assert lib.er_variance_fold(h) == STATE
        assert b"er_render_begin" in lib.er_last_error()
        assert lib.er_variance_info(h, C.byref(info)) == STATE
        assert lib.er_read_variance(h, fp) == STATE
        assert lib.er_denoise_variance(h, C.byref(par)) == STATE and lib.er_denoise_variance(h, C.byref(abi.ErDenoiseVariance(8, 2.0, 0.3, 0.2))) == STATE
        # the state is not part of er_state_*
        size = C.c_uint64()
        assert lib.er_state_size(h, C.byref(size)) == abi.ER_OK and size.value == 64 + 16 * 16 * (5 * 16 + 8)
    finally:
        lib.er_scene_destroy(h)


# ---- the header's routines against variance.py ----

def recurrence(beauty, samples, L):
    """one sample L [n][3] through the reference's running mean (src/kernel.cpp:602-643) in float32: I <- I * sa / (sa + 1) + L / (sa + 1)"""
    sa = samples.astype(f32)[:, None]
    out = beauty.copy()
    out[:, :3] = beauty[:, :3] * sa / (sa + f32(1)) + L.astype(f32) / (sa + f32(1))
    return out, samples + np.uint32(1)


def random_state(rng, n):
    st = np.zeros((n, 12), f32)
    st[:, 0:3] = rng.uniform(0, 4, (n, 3))
    st[:, 4:7] = rng.uniform(0, 4, (n, 3))
    st[:, 7] = rng.integers(1, 200, n)
    st[:, 8:11] = rng.uniform(0, 3, (n, 3))
    u = st.view(np.uint32)
    u[:, 3] = rng.integers(1, 300, n)
    u[:, 11] = rng.integers(0, 40, n)
    return st


def test_mark_fold_and_value_equal_the_numpy_restatement():
    rng = np.random.default_rng(17)
    n = 6000
    st = random_state(rng, n)
    u = st.view(np.uint32)
    M = (u[:, 3] + rng.integers(1, 9, n)).astype(np.uint32)
    beauty = rng.uniform(0, 4, (n, 4)).astype(f32)
    # the named cases
    M[:200] = u[:200, 3]                                              # n = 0
    u[200:300, 11] = 0                                                # K = 0: a first batch
    st[200:300, 4:11] = 0
    u[300:400, 11] = 1                                                # K = 1: the second
    u[400:450, 3] = 1                                                 # from the setup state ...
    st[400:450, 0:3] = 0
    M[400:450] = 1 + rng.integers(1, 9, 50)
    M[450:460] = 1                                                    # ... and M = 1 with m = 1 (n = 0), M = 1 in the value
    u[450:460, 3] = 1
    u[500:600, 3] = (1 << 24) - rng.integers(0, 4, 100)               # counts near 2^24: (float)M rounds
    M[500:600] = u[500:600, 3] + rng.integers(1, 6, 100)
    st[600:700, 8:11] = 0                                             # zero variance: M2 = 0 and J = mu
    st[600:700, 4:7] = st[600:700, 0:3]
    beauty[600:700, :3] = st[600:700, 0:3]
    u[700:720, 3] = 0xFFFFFFF0                                        # the count wraps (not a render, but the header is total)
    M[700:720] = 5
    beauty[720:730, 0] = np.nan
    g_mark, w_mark = abi.debug_variance_mark(beauty, M), variance.mark(beauty, M)
    assert (bits(g_mark) == bits(w_mark)).all() and (bits(variance.start(4)) == bits(abi.debug_variance_mark(np.zeros((4, 4), f32), np.ones(4, np.uint32)))).all()
    g, gf = abi.debug_variance_fold(st, beauty, M)
    w, wf = variance.fold(st, beauty, M)
    assert (gf == wf).all() and (bits(g) == bits(w)).all()
    assert not gf[:200].any() and (bits(g[:200]) == bits(st[:200])).all() and gf[200:450].all()      # n = 0: word for word as it was
    assert (g.view(np.uint32)[gf, 11] == u[gf, 11] + 1).all() and (g.view(np.uint32)[gf, 3] == M[gf]).all()
    assert (g[200:300, 8:11] == 0).all()                              # a first batch: mu' = J exactly, M2 stays 0
    for samples in (M, np.maximum(M, 2), np.ones(n, np.uint32)):
        gv, wv = abi.debug_variance_value(g, samples), variance.value(g, samples)
        assert (bits(gv) == bits(wv)).all()
        K = g.view(np.uint32)[:, 11]
        assert (gv[:, 3] == K).all() and (gv[K < 2, :3] == 0).all() and not (gv[:, :3] < 0).any() and not np.isnan(gv).any()
    assert (abi.debug_variance_value(g, np.ones(n, np.uint32))[:, :3] == 0).all()      # M = 1: nothing but the setup sample


def test_a_batch_whose_mean_does_not_round_to_j_gives_no_negative_variance():
    """The max(0, .) of the value.  A first batch onto mu = 0 gives mu' = J exactly; onto any other mu (W = 0, n / W' = 1) mu + d need not
    round to J and can land beyond it: d * (J - mu') then comes out negative by an ulp or so.  (With a weight already there n / W' < 1 and
    rounding is monotone: mu' stays between mu and J.)  Seeded inputs that hold such pixels; both sides must agree word for word, and
    the value must read 0 there."""
    rng = np.random.default_rng(23)
    n = 200000
    first = np.zeros((n, 12), f32)                                     # K = 0, W = 0, a mean left over: mu + (J - mu) against J
    first[:, 4:7] = rng.uniform(0.5, 2, (n, 1)).astype(f32)
    first.view(np.uint32)[:, 3] = 1
    b1 = np.zeros((n, 4), f32)
    b1[:, :3] = rng.uniform(0.001, 8, (n, 1)).astype(f32)
    M1 = np.full(n, 3, np.uint32)
    g1, _ = abi.debug_variance_fold(first, b1, M1)
    w1, _ = variance.fold(first, b1, M1)
    assert (bits(g1) == bits(w1)).all()
    J1 = (b1[:, 0] * f32(3) - f32(0) * f32(1)) / f32(2)
    off = g1[:, 4] != J1
    print("first batches whose mu + d does not round to J:", int(off.sum()), "of", n, "; with M2 < 0:", int((g1[:, 8] < 0).sum()))
    assert off.any() and (g1[:, 8] < 0).any()
    g1.view(np.uint32)[:, 11] = 2                                      # (read as if a second batch had left it so)
    v1 = abi.debug_variance_value(g1, M1)
    assert (bits(v1) == bits(variance.value(g1, M1))).all() and (v1[g1[:, 8] < 0, :3] == 0).all() and (v1[:, :3] >= 0).all()


def planes(rng, w, h, flags):
    n = w * h
    e = rng.uniform(0, 3, (n, 4)).astype(f32)
    ve = (rng.uniform(0, 0.2, (n, 4)) ** 2).astype(f32)
    ve[:, 3] = flags
    ve[rng.random(n) < 0.1, :3] = 0                                   # zero variance: sky seen directly, a black pixel
    normal = rng.normal(size=(n, 4)).astype(f32)
    normal[:, :3] /= np.linalg.norm(normal[:, :3], axis=1, keepdims=True)
    normal[rng.random(n) < 0.15, :3] = 0
    albedo = rng.uniform(0, 1, (n, 4)).astype(f32)
    depth = np.repeat(rng.uniform(0, 5, (n, 1)), 4, 1).astype(f32)
    depth[rng.random(n) < 0.1] = 0
    return e, ve, normal, albedo, depth


@pytest.mark.parametrize("shape", [(23, 17), (5, 3), (1, 1)])
def test_split_and_level_equal_the_numpy_restatement(shape):
    w, h = shape
    rng = np.random.default_rng(31 + w)
    n = w * h
    for flags in (np.ones(n, f32), np.zeros(n, f32), (rng.random(n) < 0.6).astype(f32)):      # every centre known, none (wc = 1), mixed
        e, ve, normal, albedo, depth = planes(rng, w, h, flags)
        levels, kc, ka, kz = variance.sigmas()
        assert levels == 5 and kc == f32(1) / (f32(6) * f32(6))
        for step in (1, 2, 16):
            g_e, g_v = abi.debug_variance_level(e, ve, normal, albedo, depth, w, h, step, kc, ka, kz)
            w_e, w_v = variance.level(e, ve, normal, albedo, depth, w, h, step, kc, ka, kz)
            assert (bits(g_e) == bits(w_e)).all() and (bits(g_v) == bits(w_v)).all(), (shape, step)
            assert (g_e[:, 3] == e[:, 3]).all() and (g_v[:, 3] == ve[:, 3]).all()          # alpha and the flag are the centre's
            assert np.isfinite(g_e).all() and (g_v[:, :3] >= 0).all()
        unknown = flags == 0
        if unknown.all() and n > 1:                                    # wc = 1: the colour stop is off, whatever colour_sigma
            a_e, _ = abi.debug_variance_level(e, ve, normal, albedo, depth, w, h, 1, kc, ka, kz)
            b_e, _ = abi.debug_variance_level(e, ve, normal, albedo, depth, w, h, 1, f32(100.0), ka, kz)
            assert (bits(a_e) == bits(b_e)).all()
    value = np.concatenate([rng.uniform(0, 0.1, (n, 3)), rng.integers(0, 5, (n, 1))], 1).astype(f32)
    albedo = rng.uniform(0, 1, (n, 4)).astype(f32)
    beauty = rng.uniform(0, 3, (n, 4)).astype(f32)
    g = abi.debug_variance_split(value, albedo)
    _, wv = variance.split(beauty, albedo, value)
    assert (bits(g) == bits(wv)).all() and ((g[:, 3] == 1) == (value[:, 3] >= 2)).all()


def test_a_pixel_of_zero_variance_keeps_its_value():
    """a known centre with variance 0 in its 3 x 3 neighbourhood weighs unequal taps by about 1e-8 / d^2: it stays what it was"""
    rng = np.random.default_rng(5)
    w, h = 9, 9
    e, ve, normal, albedo, depth = planes(rng, w, h, np.ones(w * h, f32))
    ve[:, :3] = 0
    normal[:, :3] = (0, 0, 1)
    albedo[:], depth[:] = 0.5, 2.0
    levels, kc, ka, kz = variance.sigmas()
    g_e, g_v = abi.debug_variance_level(e, ve, normal, albedo, depth, w, h, 1, kc, ka, kz)
    assert np.abs(g_e[:, :3] - e[:, :3]).max() < 1e-5 and (g_v[:, :3] == 0).all()


# ---- the estimator ----

@pytest.mark.parametrize("pattern,bound", [((2,) * 8, 0.050), ((1, 2, 3, 2), 0.077), ((4,) * 16, 0.034)])
def test_the_estimate_is_unbiased(pattern, bound):
    """4 096 Gaussian pixels (per-pixel mean and sigma, one channel each of rgb) through the reference's recurrence in float32, folded in
    the given batches: sum(v) / sum(true variance of the stored value) within 6 standard deviations sqrt(2 / ((K - 1) * 4096)) of 1.
    The stored value after M - 1 samples is their sum over M, so its variance is sigma^2 (M - 1) / M^2."""
    P = 4096
    K = len(pattern)
    assert abs(6 * np.sqrt(2 / ((K - 1) * P)) - bound) < 5e-4          # the bound is the estimator's own spread, derived, not tuned
    rng = np.random.default_rng(101 + K)
    sigma = np.full(P, 0.5)
    mean = rng.uniform(0.2, 2.0, P)
    beauty, samples = np.zeros((P, 4), f32), np.ones(P, np.uint32)
    beauty[:, 3] = 1
    st = variance.start(P)
    for b in pattern:
        for _ in range(b):
            L = np.repeat((mean + sigma * rng.standard_normal(P))[:, None], 3, 1)
            beauty, samples = recurrence(beauty, samples, L)
        st, folded = variance.fold(st, beauty, samples)
        assert folded.all()
    v = variance.value(st, samples)
    M = samples.astype(np.float64)
    truth = sigma ** 2 * (M - 1) / (M * M)
    ratio = float(v[:, 0].astype(np.float64).sum() / truth.sum())
    print(f"fold pattern {pattern}: sum(v) / sum(truth) = {ratio:.4f} (bound +-{bound})")
    assert (v[:, 3] == K).all() and (bits(v[:, 0]) == bits(v[:, 1])).all()
    assert abs(ratio - 1) <= bound


def test_an_untouched_pixel_keeps_all_twelve_words():
    rng = np.random.default_rng(3)
    n = 64
    beauty, samples = np.zeros((n, 4), f32), np.ones(n, np.uint32)
    st = variance.start(n)
    stopped = np.arange(n) % 4 == 0
    for batch in range(3):
        for _ in range(2):
            nb, ns = recurrence(beauty, samples, rng.uniform(0, 2, (n, 3)))
            keep = stopped & (batch == 1)                              # a tile the adaptive sampler stopped for the second batch
            beauty, samples = np.where(keep[:, None], beauty, nb).astype(f32), np.where(keep, samples, ns).astype(np.uint32)
        before = st.copy()
        g, gf = abi.debug_variance_fold(st, beauty, samples)
        st, wf = variance.fold(st, beauty, samples)
        assert (bits(g) == bits(st)).all() and (gf == wf).all()
        if batch == 1:
            assert (gf == ~stopped).all() and (bits(st[stopped]) == bits(before[stopped])).all()
    K = st.view(np.uint32)[:, 11]
    assert (K[stopped] == 2).all() and (K[~stopped] == 3).all()


def test_host_routines_under_sanitizers(tmp_path):
    """tests/native/variance_host.cpp: er_variance.h alone -- mark, fold, value, split and every step of the filter on a frame of exactly
    x_res * y_res entries -- with ASan + UBSan"""
    exe = str(tmp_path / "variance_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "elevenrender_amd", "csrc"), os.path.join(ROOT, "tests", "native", "variance_host.cpp"), "-o", exe])
    out = subprocess.run([exe], text=True, capture_output=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "variance_host ok" in out.stdout
