"""ER_FLAG_MESH_LIGHTS on the GPU: next-event estimation of emissive triangles (rules: csrc/er_shade.h; table: csrc/er_lights.hip).

The oracle mirrors this extension statement for statement, and tests/test_gpu_mesh_light_parity.py holds the kernels to it on bits.  Here:
the emitter table against a numpy float32 replay of the float order csrc/er_lights.hip documents, bit for bit, at sizes that leave the
first wave, workgroup and CDF chunk (tests/mesh_light_scenes.py), and against float64 sums with a derived bound; equality across the
schedules, ranks, checkpoints and adaptive tiles; a replay of the RNG draws; and statistics that share no formula with the mirror:
the estimator's mean against the render without the flag -- also on a scene with cut-outs between bounce and emitter and emitters of
textured emission and partial opacity -- and its noise.

Left out: er_lights_scan_kernel with chunk >= 2 needs more than 1 048 576 triangles, which is outside a test of a few seconds."""
import ctypes as C

import numpy as np
import pytest

import mesh_light_scenes as mls
from elevenrender_amd import abi, client, render, scenes

from test_gpu_parity import gpu_render
from test_host_server import Server, session_scene

pytestmark = pytest.mark.gpu

PLANES = ("beauty", "normal", "tangent", "bitangent", "denoise")
SCHEDULES = (abi.FLAG_STREAM, abi.FLAG_WAVEFRONT, abi.FLAG_MEGAKERNEL)
MESH = abi.FLAG_MESH_LIGHTS


def lum(rgb):
    rgb = np.asarray(rgb, np.float64)
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def dim_cornell(x_res=64, y_res=64):
    """scenes.cornell_dim: C1 lit by its emitter (light at y = 0.7, emission 0.3, HDRI 0.002), chosen so that no path reaches the
    clamp at 10: a sample adds the emission 0.3 at most once per vertex, weighted by MIS weights <= 1 and by a throughput that does
    not grow with these diffuse materials (albedo <= 0.8), so it stays far below 10; the unbiasedness test also checks its chunk means."""
    return scenes.cornell_dim(x_res, y_res)


def textured_scene(x_res=48, y_res=48):
    """C1 plus: the light textured (a 4 x 4 emission map, bilinear), a floor triangle of constant emission, and an emissive triangle of
    zero area (no entry)."""
    sc = scenes.cornell(x_res, y_res)
    rng = np.random.default_rng(7)
    tex = (rng.random((4, 4, 3)) * 6.0).astype(np.float32)
    v = np.concatenate([sc.vertices, np.array([[[0.2, -0.99, 2.5], [0.6, -0.99, 2.5], [0.2, -0.99, 2.9]],
                                               [[0.0, 0.0, 3.0], [0.0, 0.0, 3.0], [0.5, 0.5, 3.0]]], np.float32)])
    normals, tangents = scenes.face_frame(v)
    uvs = np.tile(np.array([[0, 0], [1, 0], [0, 1]], np.float32), (len(v), 1, 1))
    mats = list(sc.materials)
    mats[3] = abi.default_material(emission=(1.0, 1.0, 1.0))
    mats[3].emission_tex = 0
    mats.append(abi.default_material(emission=(0.5, 1.5, 0.25)))
    mid = np.concatenate([sc.material_id, np.array([4, 4], np.int32)])
    return abi.SceneData(v, normals, tangents, uvs, np.ones(len(v), np.float32), mid, mats, textures=[(tex, 4, 4, 3, 1)],
                         camera=sc.camera, x_res=x_res, y_res=y_res)


def numpy_table(sc):
    """(input triangle indices, P) of the emitter table, in float64 (csrc/er_shade.h rule 1)."""
    v = np.asarray(sc.vertices, np.float32).astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    w = np.zeros(len(v))
    for t in range(len(v)):
        m = sc.materials[int(sc.material_id[t])]
        if m.emission_tex >= 0:
            data, tw, th, ch, _ = sc.textures[m.emission_tex]
            l = lum(np.asarray(data, np.float32).reshape(th * tw, ch)[:, :3]).mean()
        else:
            l = lum((m.emission.x, m.emission.y, m.emission.z))
            if not l > 0:
                continue
        w[t] = area[t] * l
    ids = np.nonzero(w > 0)[0]
    return ids, w[ids] / w[ids].sum()


def run(sc, spp, flags=0, chunks=None, **kw):
    rm = render.RenderingManager(render.RenderParameters(flags=flags, **kw))
    rm.start_rendering(sc)
    for n in (chunks or [spp]):
        if n:
            rm.render(n)
    out = {p: rm.get_pass(p) for p in PLANES}
    out["samples"] = rm.read_samples()
    out["rng"] = rm.read_rng()
    out["lights"] = rm.light_info()
    out["table"] = rm.debug_light_table()
    rm.close()
    return out


def same(a, b, what, mask=None):
    for p in PLANES + ("samples", "rng"):
        x, y = np.asarray(a[p]), np.asarray(b[p])
        if p in PLANES:
            x, y = x.view(np.uint32), y.view(np.uint32)
        if mask is not None:
            x, y = x.reshape(mask.shape + (-1,))[mask], y.reshape(mask.shape + (-1,))[mask]
        assert (x == y).all(), f"{what}: {p} differs"


@pytest.mark.parametrize("builder", [abi.FLAG_HOST_BUILD, abi.FLAG_GPU_BUILD])
@pytest.mark.parametrize("make", [scenes.cornell, textured_scene])
def test_light_table_matches_numpy(make, builder):
    sc = make(16, 16)
    ids, prob = numpy_table(sc)
    r = run(sc, 0, flags=MESH | builder)
    tri, cdf = r["table"]
    assert r["lights"]["emitters"] == len(ids)
    # in slot order: the same set as numpy, each input triangle once
    assert sorted(tri.tolist()) == ids.tolist()
    p_dev = np.diff(np.concatenate([[0.0], cdf.astype(np.float64)]))
    order = {t: i for i, t in enumerate(ids)}
    p_ref = np.array([prob[order[t]] for t in tri])
    assert np.allclose(p_dev, p_ref, rtol=1e-6, atol=0), (p_dev, p_ref)
    assert abs(float(cdf[-1]) - 1.0) <= 1e-6


@pytest.mark.parametrize("builder", [abi.FLAG_HOST_BUILD, abi.FLAG_GPU_BUILD], ids=["host-build", "gpu-build"])
@pytest.mark.parametrize("n_tris,share", mls.CASES, ids=mls.CASE_IDS)
def test_light_table_bit_for_bit(n_tris, share, builder):
    """The device's table -- CDF, P at every emitter's slot, W -- equals the numpy float32 replay of the documented order of operations
    (mesh_light_scenes.replay_table) as bits, at the sizes of mesh_light_scenes.CASES: a second wave, a full and a partial workgroup, a
    second workgroup, CDF chunks of 2 and 3 entries with trailing threads that own nothing, waves and workgroups without an emitter, a
    single entry, none.  The emitter order is the device's own; it must be the ascending slot order of the triangle records, and the
    set numpy's.  Beside it the float64 sums with the bound derived in mesh_light_scenes.float64_cdf."""
    sc = mls.emitters(n_tris, share)
    want = mls.emitter_count(n_tris, share)
    rm = render.RenderingManager(render.RenderParameters(flags=MESH | builder))
    rm.start_rendering(sc)
    info = rm.light_info()
    tri, cdf, prob = rm.debug_light_table(prob=True)
    isect = rm.debug_read_accel()["isect"][:sc.tri_count]
    rm.close()
    assert info["emitters"] == want == len(tri)
    # the order: ascending slot of the triangle records; the set: numpy's, by the float32 weights and by the rule in float64
    slot_of = np.empty(sc.tri_count, np.int64)
    slot_of[isect["tri_id"]] = np.arange(sc.tri_count)
    assert sorted(isect["tri_id"].tolist()) == list(range(sc.tri_count))
    assert (np.diff(slot_of[tri]) > 0).all()
    rep = mls.replay_table(sc, tri)
    assert sorted(tri.tolist()) == rep["emitters"].tolist() == mls.numpy_emitters64(sc).tolist()
    if builder == abi.FLAG_HOST_BUILD:
        assert (tri == mls.host_order(sc)).all()
    if want == 0:
        assert info["total_weight"] == 0.0
        return
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert (bits(cdf) == bits(rep["cdf"])).all(), int((bits(cdf) != bits(rep["cdf"])).sum())
    assert (bits(prob) == bits(rep["prob"])).all(), int((bits(prob) != bits(rep["prob"])).sum())
    assert bits(np.float32(info["total_weight"])) == bits(rep["total"])
    cdf64, bound, total64 = mls.float64_cdf(rep["weight"], info["total_weight"])
    err = np.abs(cdf.astype(np.float64) - cdf64) / cdf64
    k = -(-want // 1024) + 1024
    print(f"{n_tris} x {share}: {want} emitters; max relative CDF error {err.max():.3e}, bound {bound:.3e}")
    assert (err <= bound).all()
    assert abs(info["total_weight"] - total64) / total64 <= k * mls.U / (1 - k * mls.U)


def test_empty_table_changes_nothing():
    sc = scenes.soup(3000, 40, 32, hdri_size=(64, 32))
    a, b = run(sc, 4), run(sc, 4, flags=MESH)
    assert b["lights"]["emitters"] == 0
    same(a, b, "soup with and without the flag")


@pytest.mark.parametrize("mis", [0, abi.FLAG_MIS])
@pytest.mark.parametrize("make", [scenes.cornell, textured_scene])
def test_schedules_give_the_same_bits(make, mis):
    sc = make(40, 32)
    outs = [run(sc, 6, flags=MESH | mis | s) for s in SCHEDULES]
    assert outs[0]["lights"]["emitters"] > 0
    for o, s in zip(outs[1:], SCHEDULES[1:]):
        same(outs[0], o, f"schedule {s} against the streaming one")
    plain = run(sc, 6, flags=mis)
    assert not (plain["beauty"].view(np.uint32) == outs[0]["beauty"].view(np.uint32)).all()    # the flag does something


def test_three_ranks_equal_one():
    sc = scenes.cornell(40, 32)
    one = run(sc, 4, flags=MESH)
    tiles_x, tiles_y = 5, 4
    for r in range(3):
        part = run(sc, 4, flags=MESH, rank=r, world=3)
        own = np.array([[(tx + ty) % 3 == r for tx in range(tiles_x)] for ty in range(tiles_y)])
        mask = np.repeat(np.repeat(own, 8, 0), 8, 1)[:32, :40]
        same(one, part, f"rank {r} of 3", mask=mask)


def test_export_import_continue():
    sc = textured_scene(32, 32)
    whole = run(sc, 6, flags=MESH | abi.FLAG_MIS)
    rm = render.RenderingManager(render.RenderParameters(flags=MESH | abi.FLAG_MIS))
    rm.start_rendering(sc)
    rm.render(2)
    blob = rm.state_export()
    rm.close()
    rm = render.RenderingManager(render.RenderParameters(flags=MESH | abi.FLAG_MIS))
    rm.start_rendering(sc)
    rm.state_import(blob)
    rm.render(4)
    out = {p: rm.get_pass(p) for p in PLANES}
    out["samples"], out["rng"] = rm.read_samples(), rm.read_rng()
    rm.close()
    same(whole, out, "export, import and continue")


def test_adaptive_tile_equals_uniform():
    sc = scenes.cornell(40, 32)
    rm = render.RenderingManager(render.RenderParameters(flags=MESH))
    rm.start_rendering(sc)
    rm.set_adaptive(0.08, 4, 2)
    rm.render(10)
    beauty, samples = rm.get_pass("beauty"), rm.read_samples().reshape(32, 40)
    rng = rm.read_rng().reshape(32, 40)
    rm.close()
    for k in np.unique(samples):
        u = run(sc, int(k) - 1, flags=MESH)
        m = samples == k
        assert (beauty.view(np.uint32)[m] == u["beauty"].view(np.uint32)[m]).all(), k
        assert (rng[m] == u["rng"].reshape(32, 40)[m]).all(), k


def xorshift(s, n):
    s = int(s)
    for _ in range(n):
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
    return s


def test_draw_count():
    """Every hit of this scene is opaque: a sample draws 5 (camera) + per hit 1 (opacity) + 7 (HDRI cell, BRDF, emitter pick and
    point), whether or not the emitter sample is then skipped."""
    sc = scenes.cornell(16, 16)
    rm = render.RenderingManager(render.RenderParameters(flags=MESH))
    rm.start_rendering(sc)
    rng0 = rm.read_rng().copy()
    rm.render(1)
    rng1 = rm.read_rng().copy()
    rm.close()
    rm = render.RenderingManager(render.RenderParameters(flags=MESH))
    rm.start_rendering(sc)
    checked = 0
    for idx in range(0, 256, 7):
        recs = rm.debug_trace_pixel(idx)
        hits = [r for r in recs if r.tri >= 0]
        assert all(r.opaque == 1 for r in hits)
        assert rng1[idx] == xorshift(rng0[idx], 5 + 8 * len(hits)), idx
        checked += len(hits) > 0
    rm.close()
    assert checked > 10


def chunk_means(sc, flags, chunks, **kw):
    """Per chunk of samples, each pixel's mean beauty over that chunk's samples (the planes hold sum / (n + 1))."""
    rm = render.RenderingManager(render.RenderParameters(flags=flags, **kw))
    rm.start_rendering(sc)
    prev, prev_sum, out = None, 0.0, []
    for n in chunks:
        rm.render(n)
        spp = rm.read_samples().reshape(sc.y_res, sc.x_res).astype(np.float64)
        s = rm.get_pass("beauty")[..., :3].astype(np.float64) * spp[..., None]
        out.append((s - prev_sum) / ((spp - (prev if prev is not None else 1.0))[..., None]))
        prev, prev_sum = spp, s
    rm.close()
    return np.stack(out)


def test_unbiased_against_the_render_without_it():
    sc = dim_cornell(64, 64)
    chunks = [256] * 8
    a, b = chunk_means(sc, 0, chunks), chunk_means(sc, MESH, chunks)
    assert a.max() < 10 and b.max() < 10            # far from the clamp (see dim_cornell)
    def blocks(x):      # per 16 x 16 block: mean over the chunks of the rgb sum, and its standard error
        s = x.sum(-1).reshape(x.shape[0], 4, 16, 4, 16).mean((2, 4))
        return s.mean(0), s.std(0, ddof=1) / np.sqrt(s.shape[0])
    ma, sa = blocks(a)
    mb, sb = blocks(b)
    z = np.abs(ma - mb) / np.sqrt(sa ** 2 + sb ** 2)
    print("block z max", z.max(), "image means", a.mean(), b.mean())
    assert (z < 4).all(), z
    assert abs(b.mean() / a.mean() - 1.0) < 0.005, (a.mean(), b.mean())


def test_unbiased_with_cutouts_and_textured_partial_emitters():
    """The same check on mesh_light_scenes.lit_soup at 64 x 64: cut-outs of opacity 0.3 lie between bounces and emitters (rule 7's
    summed distance), emission comes from textures at the sampled point's uv, and emitters have an opacity of 0.5 and a textured one
    beyond [0, 1] (rule 4).  The oracle's mirror is written from the same rules as the kernel, so a wrong rule would be mirrored; the
    render without the flag shares none of them.  Per 16 x 16 block the chunk means agree within 4 standard errors of their difference,
    and so do the image means; the standard errors come from the 8 chunk means of both renders.  No fixed percentage."""
    sc = mls.lit_soup(x_res=64, y_res=64)
    chunks = [256] * 8
    kw = dict(max_bounces=mls.LIT_MAX_BOUNCES)
    a, b = chunk_means(sc, 0, chunks, **kw), chunk_means(sc, MESH, chunks, **kw)
    assert a.max() < 10 and b.max() < 10            # far from the clamp (emission < 1, HDRI < 0.1: see lit_soup)
    def blocks(x):
        s = x.sum(-1).reshape(x.shape[0], 4, 16, 4, 16).mean((2, 4))
        return s.mean(0), s.std(0, ddof=1) / np.sqrt(s.shape[0])
    ma, sa = blocks(a)
    mb, sb = blocks(b)
    z = np.abs(ma - mb) / np.sqrt(sa ** 2 + sb ** 2)
    ia, ib = a.sum(-1).mean((1, 2)), b.sum(-1).mean((1, 2))          # the 8 chunk means of the whole image
    zi = abs(ia.mean() - ib.mean()) / np.sqrt(ia.var(ddof=1) / len(ia) + ib.var(ddof=1) / len(ib))
    print("lit_soup: block z max", z.max(), "image means", ia.mean(), ib.mean(), "image z", zi,
          "chunk-mean std without / with", ia.std(ddof=1), ib.std(ddof=1))
    assert (z < 4).all(), z
    assert zi < 4, (ia.mean(), ib.mean(), zi)


def test_variance_reduction():
    sc = dim_cornell(64, 64)
    ref = gpu_render(sc, 4096, flags=MESH)["beauty"][..., :3].astype(np.float64)
    plain = gpu_render(sc, 16)["beauty"][..., :3]
    nee = gpu_render(sc, 16, flags=MESH)["beauty"][..., :3]
    e_plain = np.sqrt(((plain - ref) ** 2).mean())
    e_nee = np.sqrt(((nee - ref) ** 2).mean())
    print("rmse without / with", e_plain, e_nee, "ratio", e_nee / e_plain)
    assert e_nee <= 0.5 * e_plain, (e_plain, e_nee)


def test_both_light_kinds_conflict():
    sc = scenes.cornell(16, 16)
    sc.point_lights = [abi.ErPointLight(abi.ErVec3(0.0, 0.5, 3.0), abi.ErVec3(1.0, 1.0, 1.0))]
    lib = abi.load()
    h = C.c_void_p()
    assert lib.er_scene_create(C.byref(sc.desc()), C.byref(h)) == abi.ER_OK
    try:
        p = abi.ErRenderParams()
        p.flags = abi.FLAG_POINT_LIGHTS | MESH
        assert lib.er_render_begin(h, C.byref(p)) == abi.ER_ERR_INVALID_ARG
        assert b"ER_FLAG_MESH_LIGHTS" in lib.er_last_error()
        p.flags = MESH          # either alone is fine
        assert lib.er_render_begin(h, C.byref(p)) == abi.ER_OK
    finally:
        lib.er_scene_destroy(h)


def test_host_session_with_the_mesh_lights_key(tmp_path):
    a = client.cornell_session_assets(32, 32)
    s = Server()
    c = client.Client(port=s.port)
    img = client.play_cornell_session(c, a, sample_target=6, mesh_lights=True)
    info = c.get_info()
    c.close()
    assert s.finish() == 0
    sc = session_scene(a, tmp_path)
    direct = gpu_render(sc, 6, flags=MESH)["beauty"]
    assert info["mesh_lights"] is True and info["emitters"] > 0
    assert (img.view(np.uint32) == direct.view(np.uint32)).all()
