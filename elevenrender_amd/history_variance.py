"""The arithmetic of the variance carried through the history (csrc/er_history_variance.h; include/eleven_hip.h er_read_history_variance,
er_read_blended_variance, er_denoise_blended) restated in numpy: every float32 operation in the header's order, nothing fused, so that
the results are the header's word for word.  The tests compare the library's debug exports and the device's planes against these
functions.

Planes are float32 [n][4]: rgb and a flag (0.0 or 1.0).  A variance state is variance.py's [n][12]; None stands for K = 0 everywhere (a
pending restart, or a state that was never allocated)."""
import numpy as np

from . import history, variance

F = np.float32


def _f(a):
    return np.ascontiguousarray(a, np.float32)


def _u(a):
    return np.ascontiguousarray(a, np.uint32).reshape(-1)


def current(state, n=None):
    """er_hv_current_px: (s2.rgb, flag) float32[n][4] -- M2 / (K - 1), values not > 0 become 0; K < 2: zeros"""
    if state is None:
        return np.zeros((n, 4), np.float32)
    st = _f(state).reshape(-1, 12)
    K = st.view(np.uint32)[:, 11]
    known = K >= 2
    out = np.zeros((len(st), 4), np.float32)
    with np.errstate(all="ignore"):
        fk = (K - np.uint32(1)).astype(np.float32)
        for c in range(3):
            v = st[:, 8 + c] / fk
            out[:, c] = np.where(known & (v > 0), v, F(0))
    out[:, 3] = known
    return out


def samples_n(samples):
    """er_hv_samples_n: (float)(samples - 1), 0 for samples = 0"""
    s = _u(samples)
    return np.where(s > 0, s - np.uint32(1), np.uint32(0)).astype(np.uint32).astype(np.float32)


def pool(s_h, w, s_c, n):
    """er_hv_pool_px: (pool.rgb, flag) float32[n][4] of (s_h [n][4] with its flag, w [n]) and (s_c [n][4], n [n])"""
    a, b = _f(s_h).reshape(-1, 4), _f(s_c).reshape(-1, 4)
    w, n = _f(w).reshape(-1), _f(n).reshape(-1)
    use_h, use_c = (a[:, 3] != 0) & (w > 0), (b[:, 3] != 0) & (n > 0)
    out = np.zeros_like(a)
    with np.errstate(all="ignore"):
        total = w + n
        both = (w[:, None] * a[:, :3] + n[:, None] * b[:, :3]) / total[:, None]
    out[:, :3] = np.where((use_h & use_c)[:, None], both, np.where(use_h[:, None], a[:, :3], np.where(use_c[:, None], b[:, :3], F(0))))
    out[:, 3] = use_h | use_c
    # (words, not values: "that one, bit for bit" keeps a NaN's payload)
    ov, av, bv = out.view(np.uint32), a.view(np.uint32), b.view(np.uint32)
    only_h, only_c = use_h & ~use_c, use_c & ~use_h
    ov[only_h, :3] = av[only_h, :3]
    ov[only_c, :3] = bv[only_c, :3]
    return out


def capture(state, samples, hist, hv):
    """er_hv_capture_px: SV float32[n][4].  hist: the resolved (H.rgb, w) or None (w = 0); hv: the resolved HV or None"""
    n = samples_n(samples)
    w = np.zeros(len(n), np.float32) if hist is None else _f(hist).reshape(-1, 4)[:, 3]
    h = np.zeros((len(n), 4), np.float32) if hv is None else _f(hv).reshape(-1, 4)
    return pool(h, w, current(state, len(n)), n)


def mean(tap_state, tap_w, tap_sv):
    """er_hv_mean: HV float32[n][4] from the tap states [n][4], the tap weights [n][4] and the taps' SV [n][4][4]"""
    st = np.ascontiguousarray(tap_state, np.uint32).reshape(-1, 4)
    tw, sv = _f(tap_w).reshape(-1, 4), _f(tap_sv).reshape(-1, 4, 4)
    ws = np.zeros(len(st), np.float32)
    acc = np.zeros((len(st), 3), np.float32)
    with np.errstate(all="ignore"):
        for k in range(4):
            v = (st[:, k] == history.TAP_VALID) & (sv[:, k, 3] != 0)
            ws = ws + np.where(v, tw[:, k], F(0))
            acc = acc + np.where(v[:, None], tw[:, k, None] * sv[:, k, :3], F(0))
        any_w = ws > 0
        out = np.zeros((len(st), 4), np.float32)
        out[:, :3] = np.where(any_w[:, None], acc / ws[:, None], F(0))
    out[:, 3] = any_w
    return out


def taps(cam, x_res, y_res, tol, hit, obj, P, moved, back, old_hit, old_obj, old_dist):
    """er_history_tap_set for n pixels: (state uint32[n][4], weight float32[n][4], q int64[n][4]) -- history.resolve()'s taps, with the
    pixel each one reads (0 for a tap outside the frame)"""
    c = _f(cam).reshape(12)
    n = len(_u(hit))
    # history.resolve() on a plane that holds each pixel's own index gives nothing about single taps: restate its geometry
    Po = history.old_points(c, hit, P, moved, back)
    xy, ok = history.project(c, x_res, y_res, Po)
    fx, fy = xy[:, 0], xy[:, 1]
    with np.errstate(all="ignore"):
        near = ok & (fx > F(-1)) & (fx < F(x_res)) & (fy > F(-1)) & (fy < F(y_res))
        flx, fly = np.floor(fx), np.floor(fy)
        tx, ty = fx - flx, fy - fly
        ux, uy = F(1) - tx, F(1) - ty
        w = [ux * uy, tx * uy, ux * ty, tx * ty]
    x0 = np.where(near, flx, 0).astype(np.int64)
    y0 = np.where(near, fly, 0).astype(np.int64)
    q, tw = np.zeros((n, 4), np.int64), np.zeros((n, 4), np.float32)
    for k in range(4):
        tx_k, ty_k = x0 + (k & 1), y0 + (k >> 1)
        inside = near & (tx_k >= 0) & (tx_k < x_res) & (ty_k >= 0) & (ty_k < y_res)
        q[:, k] = np.where(inside, ty_k * x_res + tx_k, 0)
        tw[:, k] = np.where(near, w[k], F(0))
    # the states are history.resolve()'s own
    _, state, _ = history.resolve(cam, x_res, y_res, tol, hit, obj, P, moved, back, old_hit, old_obj, old_dist, np.zeros((x_res * y_res, 4), np.float32))
    return state, tw, q


def resolve(cam, x_res, y_res, tol, hit, obj, P, moved, back, old_hit, old_obj, old_dist, old_cw, old_sv):
    """er_hv_resolve_px for n pixels: (rgbw, hv float32[n][4], state uint32[n][4], cls uint32[n]) -- the colour is history.resolve()'s"""
    rgbw, state, cls = history.resolve(cam, x_res, y_res, tol, hit, obj, P, moved, back, old_hit, old_obj, old_dist, old_cw)
    _, tw, q = taps(cam, x_res, y_res, tol, hit, obj, P, moved, back, old_hit, old_obj, old_dist)
    sv = _f(old_sv).reshape(-1, 4)[q]
    return rgbw, mean(state, tw, sv), state, cls


def blend(state, samples, hist, hv):
    """er_hv_blend_px: VB float32[n][4] -- the variance of history.blend()'s colour and its flag"""
    n = samples_n(samples)
    w = _f(hist).reshape(-1, 4)[:, 3]
    h = np.zeros((len(n), 4), np.float32) if hv is None else _f(hv).reshape(-1, 4)
    p = pool(h, w, current(state, len(n)), n)
    with np.errstate(all="ignore"):
        total = w + n
        any_v = (p[:, 3] != 0) & (total > 0)
        out = np.zeros_like(p)
        out[:, :3] = np.where(any_v[:, None], p[:, :3] / total[:, None], F(0))
    out[:, 3] = p[:, 3]
    return out


def split(blended, vb, albedo):
    """er_hv_split_px: (e, ve) float32[n][4]"""
    b, v, a = _f(blended).reshape(-1, 4), _f(vb).reshape(-1, 4), _f(albedo).reshape(-1, 4)
    e, ve = np.zeros_like(b), np.zeros_like(b)
    with np.errstate(all="ignore"):
        for c in range(3):
            ap = a[:, c] + F(0.01)
            e[:, c] = b[:, c] / ap
            ve[:, c] = v[:, c] / (ap * ap)
    e[:, 3] = b[:, 3]
    ve[:, 3] = v[:, 3]
    return e, ve


def denoise(beauty, samples, state, hist, hv, normal, albedo, depth, w, h, levels=0, colour_sigma=0.0, albedo_sigma=0.0, depth_sigma=0.0):
    """er_denoise_blended: the DENOISE plane float32[h * w][4] from BEAUTY, the counts, the variance state (None: K = 0), the resolved
    history and its variance (None: none carried), NORMAL and the two feature planes"""
    levels, kc, ka, kz = variance.sigmas(levels, colour_sigma, albedo_sigma, depth_sigma)
    blended = history.blend(beauty, samples, hist)
    e, ve = split(blended, blend(state, samples, hist, hv), albedo)
    for k in range(levels):
        e, ve = variance.level(e, ve, normal, albedo, depth, w, h, 1 << k, kc, ka, kz)
    return variance.join(e, albedo, blended)
