"""The scenes of tests/uv_scenes.py judged WITHOUT a GPU: the helper leaves its source alone and is seeded; the texture plan of the two
tiled scenes is what each is about (modes, fused widths and filters); and, on the oracle alone, the rays of the test frame reach what
the GPU tests of tests/test_gpu_uv.py then compare -- coordinates outside [0, 1]^2, negative ones, ones several periods out, every
material, both tangent signs -- so that a degenerate scene cannot let those tests pass."""
import ctypes as C
import functools

import numpy as np
import pytest

import uv_scenes
from elevenrender_amd import abi, scenes

f32 = np.float32


def test_varied_copies_and_is_seeded():
    sc = scenes.soup(257, 32, 24, seed=13, hdri_size=(32, 16))
    before = (sc.uvs.copy(), sc.tangent_sign.copy())
    a, b, c = uv_scenes.varied(sc, 5), uv_scenes.varied(sc, 5), uv_scenes.varied(sc, 6)
    assert (sc.uvs == before[0]).all() and (sc.tangent_sign == before[1]).all() and (sc.uvs == uv_scenes.UNIT).all()
    assert a.uvs.tobytes() == b.uvs.tobytes() and a.tangent_sign.tobytes() == b.tangent_sign.tobytes()
    assert a.uvs.tobytes() != c.uvs.tobytes() and a.tangent_sign.tobytes() != c.tangent_sign.tobytes()
    k = len(uv_scenes.SPECIAL)
    assert a.uvs[:k].tobytes() == uv_scenes.SPECIAL.tobytes() and a.vertices is sc.vertices
    assert a.uvs.dtype == f32 and a.uvs.shape == (257, 3, 2) and a.tangent_sign.shape == (257,)
    assert set(np.unique(a.tangent_sign).tolist()) == {-1.0, 1.0} and 0.4 < (a.tangent_sign < 0).mean() < 0.6
    rest = a.uvs[k:]
    assert len(np.unique(rest.reshape(len(rest), -1), axis=0)) == len(rest)                 # no two triangles share a mapping
    assert (rest < 0).any(-1).any(-1).mean() > 0.5 and np.abs(rest).max() <= 8.0
    e1, e2 = rest[:, 1] - rest[:, 0], rest[:, 2] - rest[:, 0]
    det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    assert 0.4 < (det < 0).mean() < 0.6                                                     # about half mirrored
    tiny = uv_scenes.varied(scenes.soup(3, 8, 8, seed=1, hdri_size=(8, 4)), 5)
    assert tiny.uvs.tobytes() == uv_scenes.SPECIAL[:3].tobytes()


@pytest.mark.parametrize("kind", list(uv_scenes.KINDS))
def test_texture_plan_is_what_the_scene_is_about(kind):
    sc = uv_scenes.tiled(kind)
    assert sc.tri_count == 3000 and (sc.x_res, sc.y_res) == (96, 64)
    uv_scenes.assert_plan(kind, abi.debug_texture_plan(sc))
    sides = [(w, h) for (_, w, h, _, _) in sc.textures] + [sc.hdri[1:3]]
    pow2 = all(s & (s - 1) == 0 for wh in sides for s in wh)
    assert pow2 == bool(uv_scenes.KINDS[kind]["tex_pow2"])
    if kind == "tiled-any":
        assert {(24, 20), (7, 5), (1, 1)} <= set(sides)
    else:
        assert {s for wh in sides for s in wh} == {8, 16, 32}
    assert {ch for (_, _, _, ch, _) in sc.textures} == {1, 2, 3, 4}
    m = sc.materials
    assert m[5].opacity_tex >= 0 and m[5].transmission_tex >= 0 and m[5].emission_tex >= 0 and m[6].normal_tex >= 0
    assert m[4].albedo_tex == m[4].roughness_tex >= 0
    for mat in range(uv_scenes.N_MATERIALS):                  # every material's triangles carry both signs
        s = sc.tangent_sign[sc.material_id == mat]
        assert (s > 0).sum() > 100 and (s < 0).sum() > 100, mat


@functools.lru_cache(maxsize=None)
def first_hits(kind):
    """One camera ray per pixel of the `kind` scene's frame (the first sample's: five draws of the pixel's stream), through
    Oracle.closest_hit and oracle_tri_hit: (triangle or -1, tu, tv) per pixel.  The oracle alone."""
    import oracle as orc
    sc = uv_scenes.tiled(kind)
    L = orc.lib()
    fp = lambda a: np.ascontiguousarray(a, f32).ctypes.data_as(C.POINTER(C.c_float))
    npx = sc.x_res * sc.y_res
    origins, dirs = np.zeros((npx, 3), f32), np.zeros((npx, 3), f32)
    for idx in range(npx):
        st, va = (C.c_uint32 * 5)(), (C.c_float * 5)()
        L.oracle_rng_stream(idx, 5, st, va)
        o, d = (C.c_float * 3)(), (C.c_float * 3)()
        L.oracle_camera_ray(C.byref(sc.camera), sc.x_res, sc.y_res, idx % sc.x_res, idx // sc.x_res, va, orc.MATH_ER, o, d)
        origins[idx], dirs[idx] = o[:], d[:]
    o = orc.Oracle(sc, math_mode=orc.MATH_ER, max_bounces=1)
    tri, _ = o.closest_hit(origins, dirs)
    o.close()
    V, N, T, UV = sc.vertices.reshape(-1, 9), sc.normals.reshape(-1, 9), sc.tangents.reshape(-1, 9), sc.uvs.reshape(-1, 6)
    uv = np.zeros((npx, 2), f32)
    for idx in np.nonzero(tri >= 0)[0]:
        t = int(tri[idx])
        rec = np.zeros(17, f32)
        assert L.oracle_tri_hit(fp(V[t]), fp(N[t]), fp(T[t]), fp(UV[t]), float(sc.tangent_sign[t]), fp(origins[idx]), fp(dirs[idx]), fp(rec))
        uv[idx] = rec[15:17]
    return tri, uv


@pytest.mark.parametrize("kind", list(uv_scenes.KINDS))
def test_the_frames_rays_reach_what_the_gpu_tests_compare(kind, oracle_mod):
    sc = uv_scenes.tiled(kind)
    tri, uv = first_hits(kind)
    hit = tri >= 0
    t, uv = tri[hit], uv[hit]
    outside = ((uv < 0) | (uv > 1)).any(-1)
    negative = (uv < 0).any(-1)
    far = ((uv < -1) | (uv > 2)).any(-1)                       # more than one period beyond [0, 1]
    per_material = np.bincount(sc.material_id[t], minlength=uv_scenes.N_MATERIALS)
    plus, minus = int((sc.tangent_sign[t] > 0).sum()), int((sc.tangent_sign[t] < 0).sum())
    print(f"{kind}: {hit.sum()} hits of {hit.size} rays; outside {outside.mean():.3f}, negative {negative.mean():.3f}, more than a period out "
          f"{far.mean():.3f}; per material {per_material.tolist()}; signs +{plus} -{minus}")
    assert np.isfinite(uv).all() and hit.mean() > 0.5
    assert outside.mean() >= 0.5
    assert negative.mean() >= 0.25
    assert far.mean() >= 0.1
    assert per_material.min() >= 50
    assert plus >= 500 and minus >= 500
