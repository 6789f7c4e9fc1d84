"""Linear-blend skinning in numpy: csrc/er_skin.h restated operation for operation, so that what er_render_skin leaves on the device (and
er_debug_skin_apply on the host) can be held against it bit for bit.

pose(palette, bones, weights, v, n, t)   the per-corner arithmetic, in float32 with nothing fused: the skinned vertices, normals, tangents
palette_ok(palette, B)                   er_render_skin's checks of a palette for an object whose largest rest |coordinate| per axis is B
"""
import numpy as np

from . import transform

INFLUENCES = 4           # ER_SKIN_INFLUENCES
MAX_BONES = 1024         # ER_SKIN_MAX_BONES
MAX_LINEAR = 16384.0     # ER_SKIN_MAX_LINEAR: a bone's |L_ij| stays at or below this
ENTRY_BYTES, BONE_BYTES, INFLUENCE_BYTES = 32, 48, 72      # per listed object, per listed bone; per triangle of a skinned object (once)


def palette_ok(palette, B):
    """every bone finite, det(L) > 0, within the overflow bound against B, and no linear entry beyond MAX_LINEAR"""
    P = np.asarray(palette, np.float32).reshape(-1, 3, 4)
    for m in P:
        try:
            transform.matrices(m)
        except ValueError:
            return False
        if not transform.bound_ok(m, B) or not (np.abs(m[:, :3]) <= np.float32(MAX_LINEAR)).all():
            return False
    return True


def blend(palette, bones, weights):
    """M = ((w0 P[b0] + w1 P[b1]) + w2 P[b2]) + w3 P[b3] per corner: [corners][12] float32"""
    P = np.ascontiguousarray(palette, np.float32).reshape(-1, 12)
    b = np.asarray(bones).reshape(-1, INFLUENCES).astype(np.int64)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1, INFLUENCES)
    assert b.shape == w.shape and (b.size == 0 or (0 <= b.min() and b.max() < len(P)))
    with np.errstate(all="ignore"):
        term = [w[:, k:k + 1] * P[b[:, k]] for k in range(INFLUENCES)]
        return (((term[0] + term[1]) + term[2]) + term[3]).astype(np.float32)


def _rows(M, x, y, z):
    """M: three rows of three per-corner columns"""
    return [(M[i][0] * x + M[i][1] * y) + M[i][2] * z for i in range(3)]


def _directions(M, d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    qx, qy, qz = _rows(M, x, y, z)
    length = np.sqrt((qx * qx + qy * qy) + qz * qz)
    unit = length > 0
    safe = np.where(unit, length, np.float32(1))
    return np.stack([np.where(unit, q / safe, np.float32(0)) for q in (qx, qy, qz)], 1).astype(np.float32)


def pose(palette, bones, weights, v, n, t):
    """the skinned [..., 3] float32 vertices, normals and tangents of rest arrays whose corners have [..., INFLUENCES] bones and weights;
    the shapes are kept"""
    v, n, t = (np.ascontiguousarray(a, np.float32) for a in (v, n, t))
    M = blend(palette, bones, weights)
    assert len(M) == v.size // 3
    with np.errstate(all="ignore"):
        L = [M[:, 4 * i + j] for i in range(3) for j in range(3)]
        c = [L[4] * L[8] - L[5] * L[7], L[5] * L[6] - L[3] * L[8], L[3] * L[7] - L[4] * L[6],
             L[2] * L[7] - L[1] * L[8], L[0] * L[8] - L[2] * L[6], L[1] * L[6] - L[0] * L[7],
             L[1] * L[5] - L[2] * L[4], L[2] * L[3] - L[0] * L[5], L[0] * L[4] - L[1] * L[3]]
        p = v.reshape(-1, 3)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        pv = np.stack([(((M[:, 4 * i] * x + M[:, 4 * i + 1] * y) + M[:, 4 * i + 2] * z) + M[:, 4 * i + 3]) for i in range(3)], 1).astype(np.float32)
        pn = _directions([c[0:3], c[3:6], c[6:9]], n.reshape(-1, 3))
        pt = _directions([L[0:3], L[3:6], L[6:9]], t.reshape(-1, 3))
    return pv.reshape(v.shape), pn.reshape(n.shape), pt.reshape(t.shape)
