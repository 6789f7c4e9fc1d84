"""Object transforms in numpy: csrc/er_xform.h restated operation for operation, so that what er_render_transform leaves on the device
(and er_debug_transform_apply on the host) can be held against it bit for bit.

matrices(m)        the host's derivation, in float64 with every product and sum rounded by itself: N (normals) and T (tangents)
pose(m, v, n, t)   the per-vertex arithmetic, in float32 with nothing fused: the posed vertices, normals and tangents
"""
import numpy as np

BOUND = 1e37     # er_xform_bound_ok: every row's |m_i0| Bx + |m_i1| By + |m_i2| Bz + |m_i3| stays at or below this


def matrices(m):
    """N = float32(C / max|C_ij|), C the cofactor matrix of L; T = float32(L / max|L_ij|).  ValueError for what the library refuses: an
    entry that is not finite, or det(L) not > 0."""
    m = np.asarray(m, np.float32).reshape(3, 4)
    if not np.isfinite(m).all():
        raise ValueError("a matrix entry is not finite")
    L = [np.float64(x) for x in m[:, :3].reshape(9)]
    with np.errstate(all="ignore"):
        c = [L[4] * L[8] - L[5] * L[7], L[5] * L[6] - L[3] * L[8], L[3] * L[7] - L[4] * L[6],
             L[2] * L[7] - L[1] * L[8], L[0] * L[8] - L[2] * L[6], L[1] * L[6] - L[0] * L[7],
             L[1] * L[5] - L[2] * L[4], L[2] * L[3] - L[0] * L[5], L[0] * L[4] - L[1] * L[3]]
        det = (L[0] * c[0] + L[1] * c[1]) + L[2] * c[2]
        if not det > 0:
            raise ValueError("det(L) is not > 0")
        cmax, lmax = max(abs(x) for x in c), max(abs(x) for x in L)
        N = np.array([x / cmax for x in c], np.float64).astype(np.float32).reshape(3, 3)
        T = np.array([x / lmax for x in L], np.float64).astype(np.float32).reshape(3, 3)
    return N, T


def bound_ok(m, B):
    """the overflow bound for an object whose largest rest |coordinate| per axis is B"""
    m = np.asarray(m, np.float32).reshape(3, 4).astype(np.float64)
    B = np.asarray(B, np.float32).astype(np.float64)
    a = np.abs(m)
    return all(((a[i, 0] * B[0] + a[i, 1] * B[1]) + a[i, 2] * B[2]) + a[i, 3] <= BOUND for i in range(3))


def _rows(M, x, y, z):
    return [(M[i][0] * x + M[i][1] * y) + M[i][2] * z for i in range(3)]


def _directions(M, d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    qx, qy, qz = _rows(M, x, y, z)
    length = np.sqrt((qx * qx + qy * qy) + qz * qz)
    unit = length > 0
    safe = np.where(unit, length, np.float32(1))
    return np.stack([np.where(unit, q / safe, np.float32(0)) for q in (qx, qy, qz)], 1).astype(np.float32)


def pose(m, v, n, t):
    """pose(rest, m) of [..., 3] float32 rest vertices, normals and tangents; the shapes are kept"""
    m = np.asarray(m, np.float32).reshape(3, 4)
    N, T = matrices(m)
    v, n, t = (np.ascontiguousarray(a, np.float32) for a in (v, n, t))
    with np.errstate(all="ignore"):
        p = v.reshape(-1, 3)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        pv = np.stack([(((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3]) for i in range(3)], 1).astype(np.float32)
        pn, pt = _directions(N, n.reshape(-1, 3)), _directions(T, t.reshape(-1, 3))
    return pv.reshape(v.shape), pn.reshape(n.shape), pt.reshape(t.shape)
