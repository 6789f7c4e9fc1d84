"""The arithmetic of the temporal reprojection (csrc/er_reproject.h; include/eleven_hip.h er_history_capture, er_history_resolve,
er_read_history, er_read_blended) restated in numpy: every float32 operation in the header's order, nothing fused, so that the results
are the header's word for word.  The tests compare the library's debug exports and the device's planes against these functions.

A projection camera is 12 float32: position[3], sensor_width, sensor_height, focal_length, cx, sx, cy, sy, cz, sz (the rotation's
cosines and sines as the library evaluates them; abi.debug_history_camera gives them for an ErCamera)."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
TAP_VALID, TAP_OUTSIDE, TAP_FLAG, TAP_OBJECT, TAP_DEPTH = 0, 1, 2, 3, 4
VALID, PARTIAL, OFFSCREEN, REJECTED, SKY = 0, 1, 2, 3, 4
CLASS_NAMES = ("valid", "partial", "offscreen", "rejected", "sky")


def _f(a):
    return np.ascontiguousarray(a, np.float32)


def project(cam, x_res, y_res, points):
    """er_history_project: world points [n][3] -> (xy float32[n][2], ok bool[n]); xy is 0 where ok is False"""
    c = _f(cam).reshape(12)
    p = _f(points).reshape(-1, 3)
    pos, sw, sh, focal = c[0:3], c[3], c[4], c[5]
    cx, sx, cy, sy, cz, sz = c[6:12]
    with np.errstate(all="ignore"):
        vx, vy, vz = p[:, 0] - pos[0], p[:, 1] - pos[1], p[:, 2] - pos[2]
        yx, yy, yz = vx * cz + vy * sz, vy * cz - vx * sz, vz
        xx, xy, xz = yx * cy - yz * sy, yy, yx * sy + yz * cy
        dx, dy, dz = xx, xy * cx + xz * sx, xz * cx - xy * sx
        s = focal / dz
        gx = ((dx * s) / sw + F(0.5)) * F(x_res)
        gy = ((dy * s) / sh + F(0.5)) * F(y_res)
        ok = (dz > 0) & np.isfinite(gx) & np.isfinite(gy)
    out = np.zeros((len(p), 2), np.float32)
    out[ok, 0], out[ok, 1] = gx[ok], gy[ok]
    return out, ok


def back_matrix(m_capture, m_now):
    """er_history_back_matrix: B = M_capture o M_now^-1 as float32[12], in float64 with the header's association; None where the
    header refuses"""
    mc = np.ascontiguousarray(m_capture, np.float32).reshape(12)
    mn = np.ascontiguousarray(m_now, np.float32).reshape(12)
    if not (np.isfinite(mc).all() and np.isfinite(mn).all()):
        return None
    D = np.float64
    L = [D(mn[4 * i + j]) for i in range(3) for j in range(3)]
    A = [D(mc[4 * i + j]) for i in range(3) for j in range(3)]
    Cf = [L[4] * L[8] - L[5] * L[7], L[5] * L[6] - L[3] * L[8], L[3] * L[7] - L[4] * L[6],
          L[2] * L[7] - L[1] * L[8], L[0] * L[8] - L[2] * L[6], L[1] * L[6] - L[0] * L[7],
          L[1] * L[5] - L[2] * L[4], L[2] * L[3] - L[0] * L[5], L[0] * L[4] - L[1] * L[3]]
    det = (L[0] * Cf[0] + L[1] * Cf[1]) + L[2] * Cf[2]
    if not det > 0:
        return None
    inv = [Cf[3 * j + i] / det for i in range(3) for j in range(3)]
    out = np.zeros(12, np.float32)
    for i in range(3):
        R = [(A[3 * i] * inv[j] + A[3 * i + 1] * inv[3 + j]) + A[3 * i + 2] * inv[6 + j] for j in range(3)]
        t = D(mc[4 * i + 3]) - ((R[0] * D(mn[3]) + R[1] * D(mn[7])) + R[2] * D(mn[11]))
        out[4 * i:4 * i + 3] = [F(r) for r in R]
        out[4 * i + 3] = F(t)
    return out


def back_table(cap_m, now_m):
    """per object: (back float32[n][12], moved uint32[n]) -- moved 0 where the two poses are bitwise equal (the back matrix is then 0)"""
    a = np.ascontiguousarray(cap_m, np.float32).reshape(-1, 12)
    b = np.ascontiguousarray(now_m, np.float32).reshape(-1, 12)
    back, moved = np.zeros((len(a), 12), np.float32), np.zeros(len(a), np.uint32)
    for o in range(len(a)):
        if a[o].tobytes() != b[o].tobytes():
            back[o], moved[o] = back_matrix(a[o], b[o]), 1
    return back, moved


def old_points(cam, hit, P, moved, back):
    """er_history_old_point per pixel: hit uint[n], P float32[n][3], moved uint[n], back float32[n][12] (per pixel)"""
    c = _f(cam).reshape(12)
    P = _f(P).reshape(-1, 3)
    m = _f(back).reshape(-1, 12)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        posed = np.stack([((m[:, 4 * i] * x + m[:, 4 * i + 1] * y) + m[:, 4 * i + 2] * z) + m[:, 4 * i + 3] for i in range(3)], 1)
        sky = c[0:3][None, :] + P
    hit = np.asarray(hit) != 0
    mv = np.asarray(moved) != 0
    return np.where(hit[:, None], np.where(mv[:, None], posed, P), sky).astype(np.float32)


def resolve(cam, x_res, y_res, tol, hit, obj, P, moved, back, old_hit, old_obj, old_dist, old_cw):
    """er_history_resolve_px for n pixels against a captured frame: (rgbw float32[n][4], state uint32[n][4], cls uint32[n]).
    moved / back are per pixel (its object's); the captured planes are flat [y_res * x_res] (old_cw [..][4])."""
    c = _f(cam).reshape(12)
    hit = np.ascontiguousarray(hit, np.uint32).reshape(-1)
    obj = np.ascontiguousarray(obj, np.uint32).reshape(-1)
    old_hit = np.ascontiguousarray(old_hit, np.uint32).reshape(-1)
    old_obj = np.ascontiguousarray(old_obj, np.uint32).reshape(-1)
    old_dist = _f(old_dist).reshape(-1)
    old_cw = _f(old_cw).reshape(-1, 4)
    tol = F(tol)
    n = len(hit)
    Po = old_points(c, hit, P, moved, back)
    xy, ok = project(c, x_res, y_res, Po)
    fx, fy = xy[:, 0], xy[:, 1]
    with np.errstate(all="ignore"):
        ex, ey, ez = Po[:, 0] - c[0], Po[:, 1] - c[1], Po[:, 2] - c[2]
        d_exp = np.sqrt((ex * ex + ey * ey) + ez * ez)
        near = ok & (fx > F(-1)) & (fx < F(x_res)) & (fy > F(-1)) & (fy < F(y_res))
        flx, fly = np.floor(fx), np.floor(fy)
        tx, ty = fx - flx, fy - fly
        ux, uy = F(1) - tx, F(1) - ty
        w = [ux * uy, tx * uy, ux * ty, tx * ty]
        x0 = np.where(near, flx, 0).astype(np.int64)
        y0 = np.where(near, fly, 0).astype(np.int64)
        state = np.zeros((n, 4), np.uint32)
        ws = np.zeros(n, np.float32)
        acc = np.zeros((n, 4), np.float32)
        new_hit = hit != 0
        for k in range(4):
            tx_k, ty_k = x0 + (k & 1), y0 + (k >> 1)
            inside = near & (tx_k >= 0) & (tx_k < x_res) & (ty_k >= 0) & (ty_k < y_res)
            q = np.where(inside, ty_k * x_res + tx_k, 0)
            oh, oo, od = old_hit[q] != 0, old_obj[q], old_dist[q]
            depth_ok = np.abs(d_exp - od) <= tol * d_exp
            st = np.full(n, TAP_VALID, np.uint32)
            st[new_hit & ~depth_ok] = TAP_DEPTH
            st[new_hit & (obj != oo)] = TAP_OBJECT
            st[new_hit != oh] = TAP_FLAG
            st[~inside] = TAP_OUTSIDE
            state[:, k] = st
            v = st == TAP_VALID
            wk = np.where(near, w[k], F(0)).astype(np.float32)
            ws = ws + np.where(v, wk, F(0))
            acc = acc + np.where(v[:, None], wk[:, None] * old_cw[q], F(0))
        any_w = ws > 0
        out = np.where(any_w[:, None], acc / ws[:, None], F(0)).astype(np.float32)
    nvalid = (state == TAP_VALID).sum(1)
    noutside = (state == TAP_OUTSIDE).sum(1)
    cls = np.where(nvalid == 4, VALID, np.where(nvalid > 0, PARTIAL, np.where(noutside == 4, OFFSCREEN, REJECTED)))
    cls = np.where(new_hit, cls, SKY).astype(np.uint32)
    return out, state, cls


def render_mean(beauty, samples):
    """er_history_render_mean: (m float32[n][3], n as float32[n])"""
    b = _f(beauty).reshape(-1, 4)[:, :3]
    s = np.ascontiguousarray(samples, np.uint32).reshape(-1)
    n = np.where(s > 0, s - np.uint32(1), np.uint32(0)).astype(np.uint32)
    nf = n.astype(np.float32)
    with np.errstate(all="ignore"):
        scale = np.where(n > 0, s.astype(np.float32) / nf, F(0)).astype(np.float32)
        m = np.where((n > 0)[:, None], b * scale[:, None], F(0)).astype(np.float32)
    return m, nf


def mix(H, w, m, nf):
    """er_history_mix: ((w H + n m) / (w + n) or 0, any bool[n])"""
    with np.errstate(all="ignore"):
        total = w + nf
        any_w = total > 0
        out = np.where(any_w[:, None], (w[:, None] * H + nf[:, None] * m) / total[:, None], F(0)).astype(np.float32)
    return out, any_w


def capture(beauty, samples, hist, max_weight):
    """er_history_capture_px: (C.rgb, W) float32[n][4]; hist None = no resolved history"""
    m, nf = render_mean(beauty, samples)
    h = np.zeros((len(nf), 4), np.float32) if hist is None else _f(hist).reshape(-1, 4)
    rgb, _ = mix(h[:, :3], h[:, 3], m, nf)
    total = h[:, 3] + nf
    W = np.where(total < F(max_weight), total, F(max_weight)).astype(np.float32)
    return np.concatenate([rgb, W[:, None]], 1).astype(np.float32)


def blend(beauty, samples, hist):
    """er_history_blend_px: float32[n][4], alpha 1; BEAUTY as it lies where w + n = 0"""
    m, nf = render_mean(beauty, samples)
    h = _f(hist).reshape(-1, 4)
    rgb, any_w = mix(h[:, :3], h[:, 3], m, nf)
    rgb = np.where(any_w[:, None], rgb, _f(beauty).reshape(-1, 4)[:, :3]).astype(np.float32)
    return np.concatenate([rgb, np.ones((len(nf), 1), np.float32)], 1)


def class_counts(cls):
    """the five counts of ErHistoryInfo from resolve()'s classes, by name"""
    return {name: int((np.asarray(cls) == i).sum()) for i, name in enumerate(CLASS_NAMES)}
