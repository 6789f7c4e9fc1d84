"""Scenes whose texture coordinates and tangent signs VARY (a module for the tests, not a conftest).

Every generator of elevenrender_amd/scenes.py gives each triangle the unit triangle [[0,0],[1,0],[0,1]] as uvs and +1 as tangent sign: an
interpolation by products with 0 and 1, a wrap that never sees a negative texel index, and records that any permutation leaves equal.
`varied` gives a copy of a scene per-triangle mappings (mirrored, rotated, several periods wide, half of them negative) and mirrored
tangents; `tiled` is a 3 000-triangle soup of eight textured materials under such mappings, in two forms: every side a power of two
(the wrap by mask, DevScene::tex_pow2 = 1) and sides 24 x 20, 7 x 5, 1 x 1 (the wrap by division).

Domain: every |u * width|, |v * height| these scenes produce is finite and far below 2^24 (|u|, |v| <= ~1006, sides <= 32).  What
Texture::getValueFromCoordinates does beyond the range of int (the float-to-int conversion is undefined there) and with NaN coordinates is
undefined in the reference and out of scope here.

All randomness comes from scenes.Rand, as the generators require."""
import copy

import numpy as np

from elevenrender_amd import abi, scenes

UNIT = np.array([[0, 0], [1, 0], [0, 1]], np.float32)

# the first triangles of a varied scene (as many as it has): edges of the mapping's domain
SPECIAL = np.array([
    [[0.37, -1.21], [0.37, -1.21], [0.37, -1.21]],                  # all three corners equal: every hit fetches one point
    [[0.0, 0.0], [1.0, 0.0], [0.0, -1.0]],                          # corners on texel boundaries: u * w = 0, w, -w for every w
    [[0.125, -0.25], [2.0, 0.375], [-1.5, -2.0]],                   # ... multiples of 1/8: integral for w = 8, 16, 24, 32
    [[1.0, 1.0], [-1.0, 1.0], [1.0, -1.0]],                         # u, v = +-1.0 exactly
    [[1000.0, -1000.0], [1001.5, -1000.25], [999.5, -998.0]],       # a far tile ...
    [[-1000.0, 1000.0], [-1000.75, 1002.0], [-997.0, 1000.5]],      # ... and its mirror image
    UNIT,                                                           # one triangle as every generator makes it
], np.float32)


def varied_uvs(n, seed):
    """uvs float32[n][3][2]: corner j of triangle t at c_t + A_t e_j, e_j the unit triangle's corners, c ~ U(-3, 3)^2, A 2 x 2 with
    entries ~ U(-2.5, 2.5); SPECIAL over the first triangles.  tangent_sign float32[n]: +1 or -1, a seeded draw, about half each."""
    r = scenes.Rand(seed, 11)
    c = r.uniform(-3.0, 3.0, n, 2)
    A = r.uniform(-2.5, 2.5, n, 2, 2)
    uv = np.stack([c, (c + A[:, :, 0]).astype(np.float32), (c + A[:, :, 1]).astype(np.float32)], axis=1).astype(np.float32)
    k = min(n, len(SPECIAL))
    uv[:k] = SPECIAL[:k]
    sign = np.where(r.u01(n) < np.float32(0.5), np.float32(1.0), np.float32(-1.0)).astype(np.float32)
    return np.ascontiguousarray(uv), sign


def varied(sc, seed):
    """a copy of `sc` (which stays as it is) with per-triangle uvs and tangent signs (varied_uvs)"""
    out = copy.copy(sc)
    out._desc = None
    out.uvs, out.tangent_sign = varied_uvs(sc.tri_count, seed)
    assert np.isfinite(out.uvs).all() and np.abs(out.uvs).max() * 32 < 2 ** 24
    return out


def _tex(r, w, h, ch, flt, lo=0.0, hi=1.0):
    """(data [h][w][ch], w, h, ch, filter) of seeded values in [lo, hi)"""
    return (abi._f32(r.uniform(lo, hi, h, w, ch)), w, h, ch, flt)


def _normal_map(r, w, h):
    """a normal map: x, y in [0.2, 0.8), z in [0.75, 1) -- local normals tilted up to ~50 degrees, so the tangent and the bitangent count"""
    xy = r.uniform(0.2, 0.8, h, w, 2)
    z = r.uniform(0.75, 1.0, h, w, 1)
    return (abi._f32(np.concatenate([xy, z], -1)), w, h, 3, 0)


# Per scene kind: (big, mid, small) sides as (w, h), the HDRI's, and what debug_texture_plan must say (tests/test_uv_scenes_cpu.py).
# Texture list, the same for both kinds but for the sides (ch = channels, f = filter: 1 bilinear):
#    0  big   3ch f0   albedo of material 0                      1  big   3ch f0   roughness of 0        2  big   1ch f0   metallic of 0
#    3  small 4ch f1   albedo of 1                               4  small 2ch f1   roughness of 1        5  small 1ch f1   metallic of 1
#    6  mid   3ch f0   albedo of 2                               7  mid   1ch f0   roughness of 2        8  mid   2ch f0   metallic of 2
#    9  big   3ch f1   albedo of 3                              10  small 3ch f0   roughness of 3       11  mid   2ch f1   metallic of 3
#   12  small 3ch f1   albedo AND roughness of 4 (kept whole)
#   13  small 2ch f1   opacity of 5                             14  big   3ch f0   transmission of 5    15  small 3ch f1   emission of 5
#   16  big   3ch f0   normal map of 6
# Materials: 0 fused unfiltered, 1 fused bilinear, 2 fused with a one-channel roughness texture, 3 not fused (three sizes), 4 one texture
# as colour and scalar, 5 opacity + transmission + emission textures, 6 a normal map under an anisotropic lobe, 7 anisotropic + clearcoat
# constants (the bitangent's sign reaches the lobes).  Triangle t has material t % 8 and a sign drawn independently: every material's
# triangles carry both signs.
KINDS = {
    "tiled-pow2": dict(sides=((32, 32), (16, 16), (8, 8)), hdri=(32, 16), tex_pow2=1),
    "tiled-any": dict(sides=((24, 20), (1, 1), (7, 5)), hdri=(24, 12), tex_pow2=0),
}
# er_texplan.h: mode 1 = first channel alone (scalar uses only, > 1 channel), 2 = that to the power 2.2 (roughness / metallic only,
# unfiltered); a texture with a colour use, an unused one, or a one-channel one that is not powered stays as it came (0)
PLAN_MODES = [0, 2, 2, 0, 1, 0, 0, 2, 2, 0, 2, 1, 0, 1, 1, 0, 0]
PLAN_FUSED = [("big", 2), ("small", 1), ("mid", 2), None, None, None, None, None]      # per material: (side, DevFused.filter) or not fused
N_MATERIALS = 8


def tiled(kind, x_res=96, y_res=64, n_tris=3000, seed=41):
    """the `kind` scene of KINDS: scenes.soup geometry with jittered (smooth) normals, the materials and textures listed above, varied
    uvs and signs"""
    k = KINDS[kind]
    big, mid, small = k["sides"]
    hw, hh = k["hdri"]
    sc = scenes.soup(n_tris, x_res, y_res, seed=seed, hdri_size=(64, 32))
    r = scenes.Rand(seed, 13)
    sc.hdri = (abi._f32(0.15 + 1.5 * r.u01(hh, hw, 3)), hw, hh, 3, 0)
    sc.normals = scenes._normalize(sc.normals + r.uniform(-0.35, 0.35, n_tris, 3, 3))
    T = [_tex(r, *big, 3, 0), _tex(r, *big, 3, 0), _tex(r, *big, 1, 0),
         _tex(r, *small, 4, 1), _tex(r, *small, 2, 1), _tex(r, *small, 1, 1),
         _tex(r, *mid, 3, 0), _tex(r, *mid, 1, 0), _tex(r, *mid, 2, 0),
         _tex(r, *big, 3, 1), _tex(r, *small, 3, 0), _tex(r, *mid, 2, 1),
         _tex(r, *small, 3, 1),
         _tex(r, *small, 2, 1, 0.25, 1.0), _tex(r, *big, 3, 0, 0.0, 0.7), _tex(r, *small, 3, 1, 0.0, 0.8),
         _normal_map(r, *big)]
    M = abi.default_material
    sc.materials = [
        M(albedo_tex=0, roughness_tex=1, metallic_tex=2, sheen=0.5),
        M(albedo_tex=3, roughness_tex=4, metallic_tex=5, clearcoat=0.7, clearcoat_gloss=0.4),
        M(albedo_tex=6, roughness_tex=7, metallic_tex=8, anisotropic=0.6),
        M(albedo_tex=9, roughness_tex=10, metallic_tex=11),
        M(albedo_tex=12, roughness_tex=12, metallic=0.3, anisotropic=0.4),
        M(albedo=(0.7, 0.6, 0.5), opacity_tex=13, transmission_tex=14, emission_tex=15, roughness=0.5),
        M(albedo=(0.6, 0.7, 0.8), normal_tex=16, roughness=0.35, metallic=0.6, anisotropic=0.8),
        M(albedo=(0.8, 0.5, 0.3), roughness=0.3, metallic=0.8, anisotropic=0.9, clearcoat=1.0, clearcoat_gloss=0.6),
    ]
    assert len(sc.materials) == N_MATERIALS and len(T) == len(PLAN_MODES)
    sc.textures = [(abi._f32(d), w, h, ch, flt) for (d, w, h, ch, flt) in T]
    sc.material_id = (np.arange(n_tris, dtype=np.int64) % N_MATERIALS).astype(np.int32)
    sc._desc = None
    return varied(sc, seed + 1)


def assert_plan(kind, plan):
    """the texture plan (abi.debug_texture_plan) is what the `kind` scene is about: nothing here passes because nothing was fused or compacted"""
    sides = dict(zip(("big", "mid", "small"), KINDS[kind]["sides"]))
    assert plan["modes"].tolist() == PLAN_MODES, plan["modes"].tolist()
    assert plan["fused_any"] == 1
    for m, want in enumerate(PLAN_FUSED):
        f = plan["fused"][m]
        if want is None:
            assert f["width"] == 0, (m, f)
        else:
            assert (int(f["width"]), int(f["height"]), int(f["filter"])) == sides[want[0]] + (want[1],), (m, f)
    # the table: compacted entries have one channel, pre-powered ones filter 2
    for i, mode in enumerate(PLAN_MODES):
        e = plan["table"][i]
        if mode:
            assert e["channels"] == 1 and (e["filter"] == 2) == (mode == 2), (i, e)
