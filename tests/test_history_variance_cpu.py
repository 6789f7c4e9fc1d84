"""The variance carried through the history (include/eleven_hip.h er_history_variance_info, er_read_history_variance,
er_read_blended_variance, er_denoise_blended) on a machine without a GPU: the symbols and the layout of ErHistoryVarianceInfo against
the C compiler's, the argument and call-order errors that need no device, (a) the header's routines (csrc/er_history_variance.h through
er_debug_history_variance_*: the functions the kernels call) against their numpy restatement (elevenrender_amd/history_variance.py) word
for word, (b) the variance of a blend of Gaussian pixels against its true value, (c) the header as a stand-alone program under ASan +
UBSan, and (d) that the three edits of the GPU test reach every way the carried variance can arrive at a pixel."""
import ctypes as C
import os
import subprocess

import numpy as np

from elevenrender_amd import abi, history, history_variance as hvar, scenes, variance
from history_variance_replay import Replay, steps
from test_history_cpu import NOTCHES, cameras, captured_frame, pixel_point

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("er_history_variance_info", "er_read_history_variance", "er_read_blended_variance", "er_denoise_blended")
DEBUG = tuple("er_debug_history_variance_" + n for n in ("current", "pool", "capture", "mean", "taps", "blend", "split"))
f32 = np.float32
bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)
same = lambda a, b: bool((bits(a) == bits(b)).all())
NONE = history.NONE


def test_library_exports_the_entry_points():
    lib = abi.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in abi.SYMBOLS, name
    for name in DEBUG:
        assert hasattr(lib, name), name
    assert lib.er_abi_version() == 2          # entry points and a struct were added, none grew


def test_struct_layout_equals_the_c_compilers(tmp_path):
    fields = [n for n, _ in abi.ErHistoryVarianceInfo._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eleven_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu", sizeof(ErHistoryVarianceInfo), sizeof(ErHistoryInfo), sizeof(ErVarianceInfo));\n'
                   + "".join(f'  printf(" %zu", offsetof(ErHistoryVarianceInfo, {f}));\n' for f in fields) + '  printf("\\n"); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    I = abi.ErHistoryVarianceInfo
    assert got == [C.sizeof(I), C.sizeof(abi.ErHistoryInfo), C.sizeof(abi.ErVarianceInfo)] + [getattr(I, f).offset for f in fields]
    assert got[:3] == [40, 64, 32]            # (the two parents' structs did not grow)


def test_arguments_and_call_order_without_a_device():
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    h = C.c_void_p()
    abi.check(lib.er_scene_create(C.byref(sc.desc()), C.byref(h)))
    plane = np.zeros(16 * 16 * 4, f32)
    fp = plane.ctypes.data_as(C.POINTER(C.c_float))
    info, par = abi.ErHistoryVarianceInfo(), abi.ErDenoiseVariance(0, 0.0, 0.0, 0.0)
    INV, STATE = abi.ER_ERR_INVALID_ARG, abi.ER_ERR_STATE
    try:
        assert lib.er_history_variance_info(None, C.byref(info)) == INV and lib.er_history_variance_info(h, None) == INV
        assert lib.er_read_history_variance(None, fp) == INV and lib.er_read_history_variance(h, None) == INV
        assert lib.er_read_blended_variance(None, fp) == INV and lib.er_read_blended_variance(h, None) == INV
        assert lib.er_denoise_blended(None, C.byref(par)) == INV and lib.er_denoise_blended(h, None) == INV
        assert b"NULL" in lib.er_last_error()
        # er_denoise_variance's argument checks, begun or not
        assert lib.er_denoise_blended(h, C.byref(abi.ErDenoiseVariance(9, 0.0, 0.0, 0.0))) == INV
        assert b"8 levels" in lib.er_last_error()
        for bad in ((-1.0, 0.0, 0.0), (0.0, -0.5, 0.0), (0.0, 0.0, -2.0), (float("nan"), 0.0, 0.0), (0.0, float("nan"), 0.0), (0.0, 0.0, float("nan"))):
            assert lib.er_denoise_blended(h, C.byref(abi.ErDenoiseVariance(0, *bad))) == INV, bad
        # a created scene that is not begun: a state error from all four
        assert lib.er_history_variance_info(h, C.byref(info)) == STATE
        assert b"er_render_begin" in lib.er_last_error()
        assert lib.er_read_history_variance(h, fp) == STATE and lib.er_read_blended_variance(h, fp) == STATE
        assert lib.er_denoise_blended(h, C.byref(par)) == STATE and lib.er_denoise_blended(h, C.byref(abi.ErDenoiseVariance(8, 1.0, 1.0, 1.0))) == STATE
        # the carried planes are not part of the state
        size = C.c_uint64()
        assert lib.er_state_size(h, C.byref(size)) == abi.ER_OK and size.value == 64 + 16 * 16 * (5 * 16 + 8)
    finally:
        lib.er_scene_destroy(h)


# ---- (a) the header's routines against history_variance.py ----

def states(rng, n):
    """variance states [n][12] whose K runs over 0, 1, 2, 9 and random counts, with negative and NaN M2 among them"""
    st = rng.uniform(0, 5, (n, 12)).astype(f32)
    K = rng.integers(0, 12, n).astype(np.uint32)
    K[:40] = np.repeat([0, 1, 2, 9], 10)
    st.view(np.uint32)[:, 11] = K
    st.view(np.uint32)[:, 3] = rng.integers(1, 40, n)
    st[5::11, 8] = -st[5::11, 8]
    st[7::13, 9] = np.nan
    st[0:40:3, 10] = -1.0          # (among the four named K too)
    st[1:40:3, 8] = np.nan
    return st


def planes(rng, n, zero_flags=5):
    """(rgb, flag) planes with flags of 0 among them"""
    p = rng.uniform(0, 3, (n, 4)).astype(f32)
    p[:, 3] = 1.0
    p[::zero_flags, 3] = 0.0
    return p


def weights(rng, n):
    w = rng.integers(0, 33, n).astype(f32)
    w[1::6] = rng.uniform(0, 4, len(w[1::6]))
    w[::4] = 0
    return w


def test_current_pool_capture_blend_and_split_equal_the_numpy_restatement():
    rng = np.random.default_rng(17)
    n = 6000
    st = states(rng, n)
    g, w = abi.debug_history_variance_current(st), hvar.current(st)
    assert same(g, w)
    K = st.view(np.uint32)[:, 11]
    assert (g[K < 2] == 0).all() and (g[K >= 2, 3] == 1).all() and (g[:, :3] >= 0).all() and np.isfinite(g).all()
    assert (g[(K >= 2) & (st[:, 8] > 0), 0] > 0).any() and (g[(K >= 2) & ~(st[:, 9] > 0), 1] == 0).all()          # a negative or NaN M2 is 0

    # the pool: w = 0, n = 0, both 0, each flag 0, a NaN payload carried through "that one, bit for bit"
    sh, sc = planes(rng, n, 5), planes(rng, n, 7)
    wh, nc = weights(rng, n), rng.permutation(weights(rng, n))
    wh[:8], nc[:8] = [0, 0, 3, 3, 0, 0, 3, 3], [0, 2, 0, 2, 0, 2, 0, 2]
    sh[:8, 3], sc[:8, 3] = 1, 1
    sh[8, :], wh[8], nc[8] = (np.nan, 1.0, 2.0, 1.0), 4.0, 0.0
    sh.view(np.uint32)[8, 0] = 0x7FC12345
    g, w = abi.debug_history_variance_pool(sh, wh, sc, nc), hvar.pool(sh, wh, sc, nc)
    assert same(g, w)
    use_h, use_c = (sh[:, 3] != 0) & (wh > 0), (sc[:, 3] != 0) & (nc > 0)
    assert all(int(m.sum()) >= 100 for m in (use_h & use_c, use_h & ~use_c, use_c & ~use_h, ~use_h & ~use_c))
    assert same(g[use_h & ~use_c, :3], sh[use_h & ~use_c, :3]) and same(g[use_c & ~use_h, :3], sc[use_c & ~use_h, :3])
    assert (g[~use_h & ~use_c] == 0).all() and (g[use_h | use_c, 3] == 1).all()
    assert list(g[:8, 3]) == [0, 1, 1, 1, 0, 1, 1, 1] and bits(g)[8, 0] == 0x7FC12345

    # capture and blend: with and without moments, a resolved history, a carried plane
    samples = rng.integers(0, 70, n).astype(np.uint32)
    samples[:40] = np.tile([0, 1, 2, 3], 10)
    hist = rng.uniform(0, 10, (n, 4)).astype(f32)
    hist[:, 3] = weights(rng, n)
    hv = planes(rng, n, 3)
    for s in (st, None):
        for h, v in ((None, None), (hist, None), (hist, hv)):
            g, w = abi.debug_history_variance_capture(s, samples, h, v), hvar.capture(s, samples, h, v)
            assert same(g, w), (s is None, h is None, v is None)
            assert ((g[:, 3] == 0) | (g[:, 3] == 1)).all() and (g[g[:, 3] == 0] == 0).all()
            if s is None and v is None:
                assert (g == 0).all()                                   # nothing known: flag 0 everywhere
            if h is not None:
                g, w = abi.debug_history_variance_blend(s, samples, h, v), hvar.blend(s, samples, h, v)
                assert same(g, w)
                assert (g[g[:, 3] == 0] == 0).all() and (g[:, :3] >= 0).all()
    vb = abi.debug_history_variance_blend(st, samples, hist, hv)
    assert 0.2 * n < (vb[:, 3] != 0).sum() < 0.98 * n
    # a pixel known on both sides: (w s2_H + n s2_C) / (w + n)^2 to rounding
    cur, nf = hvar.current(st), hvar.samples_n(samples)
    both = (hv[:, 3] != 0) & (hist[:, 3] > 0) & (cur[:, 3] != 0) & (nf > 0)
    want = (hist[both, 3, None] * hv[both, :3].astype(np.float64) + nf[both, None] * cur[both, :3]) / (hist[both, 3, None] + nf[both, None]) ** 2
    assert both.sum() > 500 and np.allclose(vb[both, :3], want, rtol=1e-5)

    blend = abi.debug_history_blend(rng.uniform(0, 10, (n, 4)).astype(f32), samples, hist)
    albedo = rng.uniform(0, 1, (n, 4)).astype(f32)
    albedo[::9, :3] = 0
    (ge, gv), (we, wv) = abi.debug_history_variance_split(blend, vb, albedo), hvar.split(blend, vb, albedo)
    assert same(ge, we) and same(gv, wv) and (ge[:, 3] == 1).all() and same(gv[:, 3], vb[:, 3])
    # the shape of er_variance_split_px: the same planes from the same inputs where the flag agrees
    val = vb.copy()
    val[:, 3] = np.where(vb[:, 3] != 0, 2.0, 0.0)
    assert same(abi.debug_variance_split(val, albedo), gv)


def test_the_mean_over_known_taps_equals_the_numpy_restatement():
    rng = np.random.default_rng(19)
    n = 5000
    state = rng.integers(0, 5, (n, 4)).astype(np.uint32)
    state[rng.random(n) < 0.5] = history.TAP_VALID
    state[:50] = rng.integers(1, 5, (50, 4))                    # all taps invalid
    tw = rng.uniform(0, 1, (n, 4)).astype(f32)
    tw[::17, 0] = 0
    sv = rng.uniform(0, 3, (n, 4, 4)).astype(f32)
    sv[..., 3] = rng.random((n, 4)) < 0.7                       # flags of 0 among valid taps
    sv[50:100, :, 3] = 0                                        # valid taps, none known
    g, w = abi.debug_history_variance_mean(state, tw, sv), hvar.mean(state, tw, sv)
    assert same(g, w)
    counted = (state == history.TAP_VALID) & (sv[..., 3] != 0)
    assert (g[~counted.any(1)] == 0).all() and (g[:100] == 0).all() and (g[counted.any(1) & (tw > 0).all(1), 3] == 1).all()
    valid = state == history.TAP_VALID
    assert ((valid & ~counted).any(1) & (g[:, 3] == 1)).sum() > 500          # a flag of 0 among valid taps, the rest carried
    lo = np.where(counted[..., None], sv[..., :3], np.inf).min(1)
    hi = np.where(counted[..., None], sv[..., :3], -np.inf).max(1)
    k = g[:, 3] == 1
    assert ((g[k, :3] >= lo[k] - 1e-4) & (g[k, :3] <= hi[k] + 1e-4)).all()    # a mean lies between its terms


def test_taps_with_the_carried_plane_equal_the_numpy_restatement():
    """test_history_cpu's captured frame and queries with an SV plane beside (C, W): the colour, the states and the classes are the plain
    resolve's, HV is the restatement's"""
    rng = np.random.default_rng(9)
    x_res, y_res, tol = 70, 45, f32(0.02)
    cam = cameras(rng, 2)[1]
    old_hit, old_obj, old_dist, old_cw = captured_frame(rng, x_res, y_res)
    old_sv = planes(rng, x_res * y_res, 3).reshape(y_res, x_res, 4)
    old_sv[10:30, 4:16, 3] = 0                                   # a region that was never known: pixels all of whose valid taps carry nothing
    old_sv[old_sv[..., 3] == 0] = 0
    old_sv = old_sv.reshape(-1, 4)
    band = lambda x: 0 if x < 20 else 1 if x < 35 else NONE if x < 50 else 2
    hit, obj, P = [], [], []
    for _ in range(3000):
        x, y, t = rng.uniform(-4, x_res + 3), rng.uniform(-4, y_res + 3), 4.0 * (1 + rng.uniform(-0.03, 0.03))
        h = int(rng.random() < 0.85)
        p = pixel_point(cam, x_res, y_res, x, y, t)
        hit.append(h)
        obj.append(band(int(np.floor(x))))
        P.append(p if h else (p - cam[0:3].astype(np.float64)) / t)
    for x, y in NOTCHES:
        for dx, dy in ((-0.5, -0.5), (0.4, -0.7)):
            hit.append(1), obj.append(0), P.append(pixel_point(cam, x_res, y_res, x + dx, y + dy, 4.0))
    hit, obj, P = np.asarray(hit, np.uint32), np.asarray(obj, np.uint32), np.asarray(P, f32)
    n = len(hit)
    moved = (rng.random(n) < 0.3).astype(np.uint32)
    back = np.zeros((n, 12), f32)
    for i in np.nonzero(moved)[0]:
        back[i] = (np.concatenate([np.eye(3), rng.uniform(-0.004, 0.004, (3, 1))], 1) + rng.uniform(-0.0005, 0.0005, (3, 4))).astype(f32).reshape(12)
    args = (cam, x_res, y_res, tol, hit, obj, P, moved, back, old_hit, old_obj, old_dist, old_cw)
    g_rgbw, g_hv, g_state, g_cls = abi.debug_history_variance_taps(*args, old_sv)
    w_rgbw, w_hv, w_state, w_cls = hvar.resolve(*args, old_sv)
    p_rgbw, p_state, p_cls = abi.debug_history_taps(*args)
    assert same(g_rgbw, p_rgbw) and (g_state == p_state).all() and (g_cls == p_cls).all()          # the colour's, bit for bit
    assert same(g_rgbw, w_rgbw) and (g_state == w_state).all() and (g_cls == w_cls).all() and same(g_hv, w_hv)
    nvalid = (g_state == history.TAP_VALID).sum(1)
    flag, w = g_hv[:, 3] != 0, g_rgbw[:, 3] > 0
    assert (g_hv[~flag] == 0).all() and not flag[nvalid == 0].any()
    assert (flag & (nvalid == 4)).sum() > 200 and (flag & (nvalid < 4)).sum() > 20 and (~flag & w).sum() > 20 and (~w).sum() > 20


# ---- (b) the statistics, without a device ----

def test_the_variance_of_a_blend_is_unbiased():
    """4 096 Gaussian pixels through the reference's recurrence I <- I * sa / (sa + 1) + L / (sa + 1) in float32: 16 samples folded in
    batches of 2 (K = 8), captured, carried through an identity resolve (every pixel its own four taps, one of weight 1), then joined by
    2 new samples with no second fold, so the blend's variance rests on the carried plane alone.  The blend is (16 m_old + 2 m_new) / 18
    with the true variance sigma^2 / 18 per pixel; sum(VB) / sum(true) lies within 6 of the estimator's own standard deviations
    sqrt(2 / ((K - 1) * 4096)) of 1."""
    rng = np.random.default_rng(23)
    P, K, per = 4096, 8, 2
    sigma = rng.uniform(0.2, 2.0, (P, 3))
    mean = rng.uniform(1.0, 4.0, (P, 3))

    def run(nsamples, fold_every):
        I, M = np.zeros((P, 4), f32), np.ones(P, np.uint32)
        st = variance.start(P)
        for s in range(nsamples):
            L = (mean + sigma * rng.standard_normal((P, 3))).astype(f32)
            sa = M.astype(f32)
            I[:, :3] = I[:, :3] * (sa / (sa + f32(1)))[:, None] + L / (sa + f32(1))[:, None]
            M = M + np.uint32(1)
            if fold_every and (s + 1) % fold_every == 0:
                st, _ = variance.fold(st, I, M)
        return I, M, st

    I, M, st = run(K * per, per)
    assert (st.view(np.uint32)[:, 11] == K).all()
    cw = history.capture(I, M, None, 32.0)
    sv = hvar.capture(st, M, None, None)
    assert (cw[:, 3] == 16).all() and (sv[:, 3] == 1).all()
    # an identity resolve: four valid taps on the pixel itself, weights (1, 0, 0, 0)
    state = np.zeros((P, 4), np.uint32)
    tw = np.tile(np.array([1, 0, 0, 0], f32), (P, 1))
    hv = hvar.mean(state, tw, np.repeat(sv[:, None, :], 4, 1))
    assert same(hv, sv)
    hist = cw.copy()
    I2, M2, _ = run(2, 0)                                      # the render started over: two samples, no fold -> K = 0
    vb = hvar.blend(None, M2, hist, hv)
    assert (vb[:, 3] == 1).all() and same(vb, abi.debug_history_variance_blend(None, M2, hist, hv))
    true = sigma ** 2 / 18.0
    ratio = float(vb[:, :3].astype(np.float64).sum() / true.sum())
    bound = 6 * np.sqrt(2 / ((K - 1) * P))
    print(f"sum(VB) / sum(true variance of the blend) = {ratio:.4f}, bound 1 +- {bound:.4f}")
    assert abs(ratio - 1) < bound
    # and the blend it describes scatters by that much: its squared error against the true mean, summed, over sum(true)
    blend = history.blend(I2, M2, hist)[:, :3].astype(np.float64)
    scatter = float(((blend - mean) ** 2).sum() / true.sum())
    assert abs(scatter - 1) < 6 * np.sqrt(2 / (3 * P))


# ---- (c) ----

def test_host_routines_under_sanitizers(tmp_path):
    """tests/native/history_variance_host.cpp: er_history_variance.h alone with ASan + UBSan, on heap arrays of exactly x_res * y_res entries"""
    exe = str(tmp_path / "history_variance_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "elevenrender_amd", "csrc"), os.path.join(ROOT, "tests", "native", "history_variance_host.cpp"), "-o", exe])
    out = subprocess.run([exe], text=True, capture_output=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "history_variance_host ok" in out.stdout


# ---- (d) ----

def synthetic_session(name):
    """the GPU test's sequence with made-up colours: 8 samples in folds of 2, then three edits with 2 samples and one fold each -- what
    is known where depends on the geometry and the counts alone"""
    rp = Replay(name)
    rng = np.random.default_rng(3)
    out = []
    for frame, (camera, poses) in enumerate([(None, None)] + steps(name)):
        if frame:
            rp.capture(beauty, samples)
            rp.edit(camera, poses)
            rp.resolve()
            out.append((rp.coverage(), rp.known()))
        for k in range(4 if frame == 0 else 1):
            beauty = rng.uniform(0, 2, (rp.npx, 4)).astype(f32)
            samples = np.full(rp.npx, 1 + 2 * (k + 1), np.uint32)
            rp.fold(beauty, samples)
    return out


def test_the_three_edits_reach_every_way_the_variance_arrives():
    """the oracle and numpy alone: after the last resolve on `large` each class holds at least 20 pixels"""
    out = synthetic_session("large")
    for cov, known in out:
        print(cov, known)
    cov, known = out[-1]
    assert sum(cov.values()) == 70 * 45
    for k in ("all_known", "some_unknown", "none_known", "no_history"):
        assert cov[k] >= 20, (k, cov)
    assert out[0][0]["some_unknown"] == out[0][0]["none_known"] == 0          # the first capture knows every pixel
