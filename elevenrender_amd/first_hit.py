"""The cut-out rule of the first-hit camera pass (csrc/er_cutout.h) restated in numpy float32, operation for operation:
what a threshold parameter means, when a hit stops a camera ray, and the ray that goes on past a hit that does not.  `walk` composes
them into FirstHit::visible (csrc/er_first_hit.h) around two callbacks, so that a test can replay the pass from any closest-hit query."""
import numpy as np

f32 = np.float32
DEFAULT_THRESHOLD = f32(0.5)
STEP = f32(0.001)


def threshold_ok(t):
    """er_cutout_threshold_ok: 0 <= t <= 1 (False for NaN)"""
    t = f32(t)
    return bool(t >= f32(0) and t <= f32(1))


def threshold(t):
    """er_cutout_threshold: 0 means 0.5"""
    t = np.asarray(t, f32)
    return np.where(t == f32(0), DEFAULT_THRESHOLD, t).astype(f32)


def stops(opacity, thr):
    """er_cutout_stops: opacity >= threshold (False for a NaN opacity)"""
    with np.errstate(invalid="ignore"):
        return np.asarray(opacity, f32) >= np.asarray(thr, f32)


def continuation(position, d):
    """er_cutout_continue: (position + d * 0.001f, d / length(d)) -- arrays [..., 3]"""
    p, d = np.asarray(position, f32), np.asarray(d, f32)
    o = (p + (d * STEP).astype(f32)).astype(f32)
    l = np.sqrt(((d[..., 0] * d[..., 0]).astype(f32) + (d[..., 1] * d[..., 1]).astype(f32)).astype(f32) + (d[..., 2] * d[..., 2]).astype(f32)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        dn = np.where((l != 0)[..., None], (d / l[..., None]).astype(f32), d).astype(f32)
    return o, dn


def walk(origin, direction, thr, max_hits, closest, opacity_of):
    """FirstHit::visible for one ray.  closest(o, d) -> (tri, position[3], payload) with tri < 0 for a miss; opacity_of(tri, payload) ->
    float32.  Returns dict(tri, position, payload, layers, capped, through_to_miss, opacity): tri = -1 for a miss of either kind."""
    o, d = np.asarray(origin, f32), np.asarray(direction, f32)
    thr = f32(thr)
    layers = 0
    for _ in range(int(max_hits)):
        tri, pos, payload = closest(o, d)
        if tri < 0:
            return dict(tri=-1, position=None, payload=None, layers=layers, capped=False, through_to_miss=layers > 0, opacity=None)
        a = f32(opacity_of(tri, payload))
        if bool(stops(a, thr)):
            return dict(tri=int(tri), position=np.asarray(pos, f32), payload=payload, layers=layers, capped=False, through_to_miss=False, opacity=a)
        layers += 1
        o, d = continuation(pos, d)
    return dict(tri=-1, position=None, payload=None, layers=layers, capped=True, through_to_miss=False, opacity=None)
