"""A scene of layered cut-outs for the first-hit pass that sees through them (er_first_hit_set), and the numpy replay of
that pass from the oracle's entry points (a module for the tests, not a conftest).

`layers(w=44, h=28)`: a frame with partial tiles on both edges, the camera at the origin looking down +z at a wall (z = 4, a bilinear
albedo texture) that does not fill the frame, and in front of it quads given by their footprint on the wall's plane, scaled to their own
depth, so that footprints line up along the camera's rays.  Every vertex is moved by a seeded offset: no edge lies along a pixel row, a
pixel centre or a quad's own diagonal.
  (A) three stacked quads of constant opacity 0.3 with distinct albedos, staggered so that their edges leave 1, 2 and 3 layers
  (B) a quad whose opacity comes from a bilinear 2-channel 5 x 3 texture with values in about [-1.5, 2.5] (mesh_light_scenes's): the
      threshold crosses inside pixels
  (C) a 0.3 quad beside the wall: nothing behind it
  (D) six quads of opacity 0 before the wall: with max_bounces 4 a ray through them is capped
  (E) an opaque quad in front of a 0.3 cut-out
  (F) a quad of opacity exactly 0.5, the default threshold
  (G) one 0.3 quad over the wall; (H) four small opaque triangles in no object
Objects: the wall, each stack and each card is one; the triangles of (H) and the second triangle of (G) are in none.
All randomness comes from scenes.Rand."""
import ctypes as C
import functools

import numpy as np

import oracle as orc
from elevenrender_amd import abi, first_hit, scenes

f32 = np.float32
WALL_Z = 4.0
MAX_BOUNCES = 4
(M_WALL, M_A0, M_A1, M_A2, M_B, M_C, M_D, M_E_FRONT, M_E_BACK, M_F, M_G, M_H) = range(12)
# name -> (footprint x0, x1, y0, y1 on the wall's plane, [(depth, material)] front to back)
STACKS = {
    "A": ((-1.62, -0.88, 0.12, 1.02), [(2.0, M_A0), (2.4, M_A1), (2.8, M_A2)]),
    "B": ((-0.78, 0.02, 0.10, 1.00), [(3.0, M_B)]),
    "F": ((0.12, 0.70, 0.14, 0.98), [(3.2, M_F)]),
    "E": ((0.82, 1.58, 0.11, 1.01), [(2.5, M_E_FRONT), (3.0, M_E_BACK)]),
    "D": ((-1.60, -0.80, -1.00, -0.12), [(1.6 + 0.3 * k, M_D) for k in range(6)]),
    "G": ((-0.62, 0.22, -0.98, -0.14), [(3.3, M_G)]),
    "C": ((1.76, 2.02, -1.02, 0.92), [(3.0, M_C)]),
}
STAGGER = {"A": 0.09}      # each deeper layer of the stack is shifted by this much in x


def _quad(x0, x1, y0, y1, z):
    s = z / WALL_Z
    p = [[x0 * s, y0 * s, z], [x1 * s, y0 * s, z], [x1 * s, y1 * s, z], [x0 * s, y1 * s, z]]
    return [[p[0], p[1], p[2]], [p[0], p[2], p[3]]], [[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]]


@functools.lru_cache(maxsize=None)
def layers(w=44, h=28, binary=False):
    """the scene; binary=True: the copy whose opacities are only 0 and 1 (constants below 0.5 -> 0, others -> 1; the opacity texture's
    texels likewise, unfiltered), on which the rule and the render's draw agree for every u in (0, 1]"""
    r = scenes.Rand(41, 3)
    tris, uvs, mats, spans = [], [], [], {}
    t, u = _quad(-1.7, 1.7, -1.1, 1.1, WALL_Z)
    tris += t; uvs += u; mats += [M_WALL, M_WALL]
    spans["wall"] = (0, 2)
    for name, ((x0, x1, y0, y1), stack) in STACKS.items():
        first = len(tris)
        for k, (z, m) in enumerate(stack):
            dx = STAGGER.get(name, 0.0) * k
            t, u = _quad(x0 + dx, x1 + dx, y0, y1, z)
            tris += t; uvs += u; mats += [m, m]
        spans[name] = (first, len(tris))
    first = len(tris)
    for k in range(4):      # (H)
        cx, cy = 0.5 + 0.3 * k, -0.75 + 0.12 * (k % 2)
        tris.append([[cx, cy, 3.5], [cx + 0.22, cy + 0.05, 3.5], [cx + 0.08, cy + 0.3, 3.45]])
        uvs.append([[0, 0], [1, 0], [0, 1]])
        mats.append(M_H)
    spans["H"] = (first, len(tris))
    v = np.array(tris, f32)
    v[..., :2] += r.uniform(-0.011, 0.011, len(v), 3, 2)
    v[..., 2] += r.uniform(-0.004, 0.004, len(v), 3)
    for a in range(0, spans["H"][0], 2):      # the two triangles of a quad keep their shared corners
        v[a + 1, 0], v[a + 1, 1] = v[a, 0], v[a, 2]
    normals, tangents = scenes.face_frame(v)
    op = np.stack([np.resize(np.array([-1.3, 2.3, -0.7, 0.5, 1.7, -1.0, 1.4], f32), 15).reshape(3, 5) + r.uniform(-0.2, 0.2, 3, 5), r.uniform(0.0, 1.0, 3, 5)], -1)
    textures = [(abi._f32(r.uniform(0.1, 0.9, 4, 6, 3)), 6, 4, 3, 1), (abi._f32(op), 5, 3, 2, 1)]
    M = abi.default_material
    materials = [None] * 12
    materials[M_WALL] = M(albedo_tex=0)
    materials[M_A0] = M(albedo=(0.9, 0.2, 0.1), opacity=0.3)
    materials[M_A1] = M(albedo=(0.1, 0.8, 0.2), opacity=0.3)
    materials[M_A2] = M(albedo=(0.2, 0.3, 0.9), opacity=0.3)
    materials[M_B] = M(albedo=(0.8, 0.7, 0.1), opacity_tex=1)
    materials[M_C] = M(albedo=(0.6, 0.1, 0.6), opacity=0.3)
    materials[M_D] = M(albedo=(0.05, 0.05, 0.05), opacity=0.0)
    materials[M_E_FRONT] = M(albedo=(0.3, 0.9, 0.9))
    materials[M_E_BACK] = M(albedo=(0.9, 0.5, 0.0), opacity=0.3)
    materials[M_F] = M(albedo=(0.4, 0.4, 0.7), opacity=0.5)
    materials[M_G] = M(albedo=(0.7, 0.2, 0.4), opacity=0.3)
    materials[M_H] = M()
    if binary:
        for m in materials:
            m.opacity = 0.0 if m.opacity < 0.5 else 1.0
        d, tw, th, ch, _ = textures[1]
        textures[1] = (abi._f32(np.where(d < 0.5, f32(0), f32(1))), tw, th, ch, 0)
    sc = abi.SceneData(v, normals, tangents, np.array(uvs, f32), np.ones(len(v), f32), np.array(mats, np.int32), materials, textures=textures,
                       hdri=(abi._f32(0.1 + 0.3 * r.u01(8, 16, 3)), 16, 8, 3, 0), camera=abi.default_camera(), x_res=w, y_res=h)
    sc.spans = spans
    return sc


def table(sc):
    """wall, stacks and cards are different objects; (H) and the second triangle of (G) are in none"""
    sp = sc.spans
    out = [np.arange(*sp[k], dtype=np.uint32) for k in ("wall", "A", "B", "F", "E", "D", "C")]
    return out + [np.arange(sp["G"][0], sp["G"][0] + 1, dtype=np.uint32)]


def stack_rays(sc):
    """one ray per stack from the camera through the centroid of the stack's front triangle (off the quad's diagonal): (names, o, d)"""
    names = [k for k in sc.spans if k not in ("wall", "H")]
    o = np.zeros((len(names), 3), f32)
    p = np.stack([sc.vertices[sc.spans[k][0]].mean(0) for k in names]).astype(f32)
    l = np.sqrt(((p[:, 0] * p[:, 0]).astype(f32) + (p[:, 1] * p[:, 1]).astype(f32)).astype(f32) + (p[:, 2] * p[:, 2]).astype(f32)).astype(f32)
    return names, o, (p / l[:, None]).astype(f32)


# ---- the replay ----

def _fp(a):
    return np.ascontiguousarray(a, f32).ctypes.data_as(C.POINTER(C.c_float))


def camera_rays(sc, n, pinhole=False, camera=None):
    """origins, dirs [npx][n][3]: the pass's sample rays (five draws each from oracle_rng_stream), or with pinhole the key's one ray
    per pixel (r1 = r2 = 0.5, bokeh 0)"""
    L = orc.lib()
    npx = sc.x_res * sc.y_res
    cam = abi.ErCamera.from_buffer_copy(camera if camera is not None else sc.camera)
    if pinhole:
        cam.bokeh = 0
        n = 1
    origins, dirs = np.zeros((npx, n, 3), f32), np.zeros((npx, n, 3), f32)
    for idx in range(npx):
        if pinhole:
            va = [0.5, 0.5, 0.0, 0.0, 0.0]
        else:
            st, va = (C.c_uint32 * (5 * n))(), (C.c_float * (5 * n))()
            L.oracle_rng_stream(idx, 5 * n, st, va)
        for k in range(n):
            o, d = (C.c_float * 3)(), (C.c_float * 3)()
            L.oracle_camera_ray(C.byref(cam), sc.x_res, sc.y_res, idx % sc.x_res, idx // sc.x_res, (C.c_float * 5)(*va[5 * k:5 * k + 5]), orc.MATH_ER, o, d)
            origins[idx, k], dirs[idx, k] = o[:], d[:]
    return origins, dirs


def opacity_of(sc, texs, tri, rec):
    """generate_hit_data's opacity of a hit record (oracle_tri_hit's 17 floats): the constant, or .x of the filtered opacity texture"""
    m = sc.materials[int(sc.material_id[tri])]
    if m.opacity_tex < 0:
        return f32(m.opacity)
    out = np.zeros(3, f32)
    orc.lib().oracle_texture_fetch(C.byref(texs[m.opacity_tex]), float(rec[15]), float(rec[16]), 1, _fp(out))
    return f32(out[0])


def albedo_of(sc, texs, tri, rec):
    m = sc.materials[int(sc.material_id[tri])]
    assert m.albedo_shader_id == -1
    if m.albedo_tex < 0:
        return np.array([m.albedo.x, m.albedo.y, m.albedo.z], f32)
    out = np.zeros(3, f32)
    orc.lib().oracle_texture_fetch(C.byref(texs[m.albedo_tex]), float(rec[15]), float(rec[16]), 1, _fp(out))
    return out


def visible(sc, origins, dirs, threshold=0.0, max_hits=MAX_BOUNCES, cutouts=True):
    """FirstHit::visible (csrc/er_first_hit.h) for rays [n][3], layer by layer over the rays still under way: Oracle.closest_hit, then
    oracle_tri_hit for the record, first_hit.stops on the opacity, first_hit.continuation for the next segment.  cutouts=False: the
    first hit, whatever its opacity.  Returns a dict of arrays: tri (-1: a miss), rec [n][17], layers, capped, to_miss, opacity (of the
    stopping hit, NaN elsewhere), dist (from the camera ray's origin, 0 of a miss), albedo ((1, 1, 1) of a miss)."""
    L = orc.lib()
    thr = first_hit.threshold(threshold)
    o0 = np.ascontiguousarray(origins, f32).reshape(-1, 3)
    o, d = o0.copy(), np.ascontiguousarray(dirs, f32).reshape(-1, 3).copy()
    n = len(o)
    tri, rec = np.full(n, -1, np.int64), np.zeros((n, 17), f32)
    layers, capped, to_miss = np.zeros(n, np.uint32), np.zeros(n, bool), np.zeros(n, bool)
    opacity = np.full(n, np.nan, f32)
    V, N, T, UV = sc.vertices.reshape(-1, 9), sc.normals.reshape(-1, 9), sc.tangents.reshape(-1, 9), sc.uvs.reshape(-1, 6)
    texs = [abi.ErTexture(w, h, ch, flt, abi._fptr(data)) for (data, w, h, ch, flt) in sc.textures]
    orac = orc.Oracle(sc, math_mode=orc.MATH_ER, max_bounces=1)
    active = np.arange(n)
    for _ in range(int(max_hits) if cutouts else 1):
        if not len(active):
            break
        found, _pos = orac.closest_hit(o[active], d[active])
        still = []
        for i, t in zip(active, found):
            if t < 0:
                to_miss[i] = layers[i] > 0
                continue
            r = np.zeros(17, f32)
            assert L.oracle_tri_hit(_fp(V[t]), _fp(N[t]), _fp(T[t]), _fp(UV[t]), float(sc.tangent_sign[t]), _fp(o[i]), _fp(d[i]), _fp(r))
            a = opacity_of(sc, texs, int(t), r)
            if not cutouts or bool(first_hit.stops(a, thr)):
                tri[i], rec[i], opacity[i] = t, r, a
                continue
            layers[i] += 1
            o[i], d[i] = first_hit.continuation(r[0:3], d[i])
            still.append(i)
        active = np.asarray(still, np.int64)
    else:
        capped[active] = cutouts
    orac.close()
    hit = tri >= 0
    e = (rec[:, 0:3] - o0).astype(f32)
    dist = np.where(hit, np.sqrt(((e[:, 0] * e[:, 0]).astype(f32) + (e[:, 1] * e[:, 1]).astype(f32)).astype(f32) + (e[:, 2] * e[:, 2]).astype(f32)), f32(0)).astype(f32)
    albedo = np.ones((n, 3), f32)
    for i in np.nonzero(hit)[0]:
        albedo[i] = albedo_of(sc, texs, int(tri[i]), rec[i])
    return dict(tri=tri, rec=rec, layers=layers, capped=capped, to_miss=to_miss, opacity=opacity, dist=dist, albedo=albedo)


def counters(v):
    """ErFirstHitInfo's five from a replay"""
    return dict(rays=len(v["tri"]), rays_through=int((v["layers"] > 0).sum()), layers_skipped=int(v["layers"].sum()), rays_capped=int(v["capped"].sum()),
                rays_through_to_miss=int(v["to_miss"].sum()))


@functools.lru_cache(maxsize=None)
def pass_replay(n_max=4, threshold=0.0, cutouts=True, binary=False):
    """the whole-frame pass of `layers()`: visible() of its n_max sample rays per pixel, computed once and shared; arrays [npx * n_max]"""
    sc = layers(binary=binary)
    origins, dirs = camera_rays(sc, n_max)
    v = visible(sc, origins, dirs, threshold, MAX_BOUNCES, cutouts)
    v["origins"], v["dirs"] = origins.reshape(-1, 3), dirs.reshape(-1, 3)
    return v


def take(v, n, n_max=4):
    """the first n rays of every pixel of a pass_replay"""
    npx = len(v["tri"]) // n_max
    return {k: a.reshape((npx, n_max) + a.shape[1:])[:, :n].reshape((npx * n,) + a.shape[1:]) for k, a in v.items()}


def planes(sc, v, n):
    """the feature planes of the replay's first n rays per pixel, in the kernel's sum order (er_features.hip)"""
    npx = sc.x_res * sc.y_res
    w = take(v, n)
    hit = (w["tri"] >= 0).reshape(npx, n)
    alb, dist = w["albedo"].reshape(npx, n, 3), w["dist"].reshape(npx, n)
    A, D, hits = np.zeros((npx, 3), f32), np.zeros(npx, f32), np.zeros(npx, np.uint32)
    for k in range(n):
        A = (A + alb[:, k]).astype(f32)
        D = np.where(hit[:, k], (D + dist[:, k]).astype(f32), D)
        hits += hit[:, k]
    cov = (hits.astype(f32) / f32(n)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(hits > 0, (D / hits.astype(f32)).astype(f32), f32(0))
    albedo = np.concatenate([(A / f32(n)).astype(f32), cov[:, None]], 1).reshape(sc.y_res, sc.x_res, 4)
    depth = np.stack([z, z, z, cov], 1).astype(f32).reshape(sc.y_res, sc.x_res, 4)
    return albedo, depth


def key_plane(sc, objects_of, camera=None, threshold=0.0, cutouts=True):
    """the history's key plane under the mode: hit, obj, dist, P (a miss: the camera ray's direction), flat -- and the replay itself"""
    origins, dirs = camera_rays(sc, 1, pinhole=True, camera=camera)
    v = visible(sc, origins, dirs, threshold, MAX_BOUNCES, cutouts)
    hit = v["tri"] >= 0
    P = np.where(hit[:, None], v["rec"][:, 0:3], dirs.reshape(-1, 3)).astype(f32)
    obj = np.where(hit, objects_of[np.maximum(v["tri"], 0)], np.uint32(0xFFFFFFFF)).astype(np.uint32)
    return dict(hit=hit.astype(np.uint32), obj=obj, dist=v["dist"], P=P), v
