"""The arithmetic of the variance plane and of the filter guided by it (csrc/er_variance.h; include/eleven_hip.h er_variance_fold,
er_read_variance, er_denoise_variance) restated in numpy: every float32 operation in the header's order, nothing fused, so that the
results are the header's word for word.  The tests compare the library's debug exports and the device's planes against these functions.

A state is a float32 array [n][12]: S.rgb, m, mu.rgb, W, M2.rgb, K -- m and K are uint32 words (state.view(np.uint32)[:, 3] and [:, 11])."""
import numpy as np

F = np.float32
KERNEL = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)
K3 = np.array([0.25, 0.5, 0.25], np.float32)


def _f(a):
    return np.ascontiguousarray(a, np.float32)


def _u(a):
    return np.ascontiguousarray(a, np.uint32).reshape(-1)


def mark(beauty, samples):
    """er_variance_mark_px: the state of a reset from BEAUTY [n][4] and the sample counts [n]"""
    b, s = _f(beauty).reshape(-1, 4), _u(samples)
    st = np.zeros((len(s), 12), np.float32)
    st[:, 0:3] = b[:, 0:3]
    st.view(np.uint32)[:, 3] = s
    return st


def start(n):
    """the state of a render that has just started: S = (0, 0, 0), m = 1"""
    return mark(np.zeros((n, 4), np.float32), np.ones(n, np.uint32))


def fold(state, beauty, samples):
    """er_variance_fold_px: (new state [n][12], folded bool[n]); pixels with n = 0 keep their 12 words"""
    st = _f(state).reshape(-1, 12).copy()
    b, M = _f(beauty).reshape(-1, 4), _u(samples)
    u = st.view(np.uint32)
    m = u[:, 3].copy()
    n = (M - m).astype(np.uint32)      # (uint32 wrap-around, as the header's)
    folded = n != 0
    with np.errstate(all="ignore"):
        fM, fm, fn = M.astype(np.float32), m.astype(np.float32), n.astype(np.float32)
        W1 = st[:, 7] + fn
        r = fn / W1
        new = st.copy()
        for c in range(3):
            J = (b[:, c] * fM - st[:, c] * fm) / fn
            d = J - st[:, 4 + c]
            mu = st[:, 4 + c] + d * r
            new[:, 8 + c] = st[:, 8 + c] + fn * (d * (J - mu))
            new[:, 4 + c] = mu
            new[:, c] = b[:, c]
        new[:, 7] = W1
    nu = new.view(np.uint32)
    nu[:, 11] = u[:, 11] + np.uint32(1)
    nu[:, 3] = M
    out = np.where(folded[:, None], nu, u).astype(np.uint32)      # (words, not floats: a NaN keeps its payload)
    return out.view(np.float32), folded


def value(state, samples):
    """er_variance_value_px: float32[n][4] -- xyz the variance of BEAUTY as stored at the count M, w = (float)K"""
    st, M = _f(state).reshape(-1, 12), _u(samples)
    K = st.view(np.uint32)[:, 11]
    out = np.zeros((len(M), 4), np.float32)
    out[:, 3] = K.astype(np.float32)
    with np.errstate(all="ignore"):
        fk, fm1, fM = (K - np.uint32(1)).astype(np.float32), (M - np.uint32(1)).astype(np.float32), M.astype(np.float32)
        mm = fM * fM
        for c in range(3):
            v = ((st[:, 8 + c] / fk) * fm1) / mm
            out[:, c] = np.where((K >= 2) & (v > 0), v, F(0))
    return out


def split(beauty, albedo, val):
    """er_variance_split_kernel: (e, ve) float32[n][4] from BEAUTY, the ALBEDO feature and value()"""
    b, a, v = _f(beauty).reshape(-1, 4), _f(albedo).reshape(-1, 4), _f(val).reshape(-1, 4)
    e, ve = np.zeros_like(b), np.zeros_like(b)
    with np.errstate(all="ignore"):
        for c in range(3):
            ap = a[:, c] + F(0.01)
            e[:, c] = b[:, c] / ap
            ve[:, c] = v[:, c] / (ap * ap)
    e[:, 3] = b[:, 3]
    ve[:, 3] = np.where(v[:, 3] >= 2, F(1), F(0))
    return e, ve


def level(e, ve, normal, albedo, depth, w, h, step, kc, ka, kz):
    """er_variance_level_px over a frame: planes [h * w][4] -> (e', ve')"""
    e, ve, n, a = (_f(x).reshape(h, w, 4) for x in (e, ve, normal, albedo))
    z = _f(depth).reshape(h, w, 4)[..., 0]
    kc, ka, kz = F(kc), F(ka), F(kz)
    ys, xs = np.mgrid[0:h, 0:w]
    known = ve[..., 3] != 0
    with np.errstate(all="ignore"):
        vb = np.zeros((h, w, 3), np.float32)
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                qy, qx = np.clip(ys + j, 0, h - 1), np.clip(xs + i, 0, w - 1)
                vb = vb + ve[qy, qx, :3] * (K3[i + 1] * K3[j + 1])
        ev = vb + F(1e-8)
        s = np.zeros((h, w, 3), np.float32)
        t = np.zeros((h, w, 3), np.float32)
        sw = np.zeros((h, w), np.float32)
        none = (n[..., :3] == 0).all(-1)
        for j in range(-2, 3):
            for i in range(-2, 3):
                qy, qx = np.clip(ys + j * step, 0, h - 1), np.clip(xs + i * step, 0, w - 1)
                cq, vq, nq, aq, zq = e[qy, qx], ve[qy, qx], n[qy, qx], a[qy, qx], z[qy, qx]
                d = e[..., :3] - cq[..., :3]
                d2 = ((d[..., 0] * d[..., 0]) / ev[..., 0] + (d[..., 1] * d[..., 1]) / ev[..., 1]) + (d[..., 2] * d[..., 2]) / ev[..., 2]
                wc = np.where(known, F(1) / (F(1) + kc * d2), F(1)).astype(np.float32)
                nd = n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1] + n[..., 2] * nq[..., 2]
                noneq = (nq[..., :3] == 0).all(-1)
                nd = np.where(none & noneq, F(1), np.where(nd < 0, F(0), nd)).astype(np.float32)
                ad = a[..., :3] - aq[..., :3]
                a2 = ad[..., 0] * ad[..., 0] + ad[..., 1] * ad[..., 1] + ad[..., 2] * ad[..., 2]
                wa = F(1) / (F(1) + a2 * ka)
                r = (z - zq) / (np.fmax(z, zq) + F(1e-6))
                wz = F(1) / (F(1) + (r * r) * kz)
                wgt = KERNEL[i + 2] * KERNEL[j + 2] * wc * (nd * nd) * wa * wz
                w2 = wgt * wgt
                s = s + cq[..., :3] * wgt[..., None]
                sw = sw + wgt
                t = t + w2[..., None] * vq[..., :3]
        out_e = np.concatenate([s / sw[..., None], e[..., 3:4]], -1).astype(np.float32)
        out_v = np.concatenate([t / (sw * sw)[..., None], ve[..., 3:4]], -1).astype(np.float32)
    return out_e.reshape(-1, 4), out_v.reshape(-1, 4)


def join(e, albedo, beauty):
    """er_guided_join_kernel"""
    e, a, b = _f(e).reshape(-1, 4), _f(albedo).reshape(-1, 4), _f(beauty).reshape(-1, 4)
    out = np.zeros_like(e)
    for c in range(3):
        out[:, c] = e[:, c] * (a[:, c] + F(0.01))
    out[:, 3] = b[:, 3]
    return out


def sigmas(levels=0, colour_sigma=0.0, albedo_sigma=0.0, depth_sigma=0.0):
    """er_denoise_variance's defaults and its three host constants: (levels, kc, ka, kz)"""
    sc, sa, sz = F(colour_sigma or 6.0), F(albedo_sigma or 0.3), F(depth_sigma or 0.2)
    return int(levels or 5), F(1) / (sc * sc), F(1) / (sa * sa), F(1) / (sz * sz)


def denoise(beauty, samples, state, normal, albedo, depth, w, h, levels=0, colour_sigma=0.0, albedo_sigma=0.0, depth_sigma=0.0):
    """er_denoise_variance: the DENOISE plane float32[h * w][4] from BEAUTY, the counts, the state, NORMAL and the two feature planes"""
    levels, kc, ka, kz = sigmas(levels, colour_sigma, albedo_sigma, depth_sigma)
    e, ve = split(beauty, albedo, value(state, samples))
    for k in range(levels):
        e, ve = level(e, ve, normal, albedo, depth, w, h, 1 << k, kc, ka, kz)
    return join(e, albedo, beauty)
