"""The scenes and the table replay of tests/mesh_light_scenes.py judged WITHOUT a GPU (the precedent: tests/test_uv_scenes_cpu.py).

  * The float32 replay of the emitter table against the oracle's own table (C++, built from the same documented order: two independent
    statements of it must give the same bits) and against the float64 sums with their derived bound, for every case of
    mesh_light_scenes.CASES.
  * mesh_pick of the oracle as a known answer.
  * The oracle alone over the traced pixels of tests/test_gpu_mesh_light_parity.py: lit_soup exercises what it is for -- every class of
    mesh_light_scenes.CLASSES at least 20 times -- and no traced sample reaches the clamp at 10.  Otherwise a passing GPU test says
    nothing.  The emitter order here is the host builder's (no device needed); the GPU test asserts that a render begun with
    ER_FLAG_HOST_BUILD has exactly this order."""
import functools

import numpy as np
import pytest

import mesh_light_scenes as mls
from elevenrender_amd import abi

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def permuted_order(sc, seed=1):
    """numpy's emitter set in a seeded order (the replay and the oracle take any order: the device's is known only on the GPU)"""
    ids = np.nonzero(mls.weights32(sc) > 0)[0]
    return np.random.default_rng(seed).permutation(ids).astype(np.int32)


@pytest.mark.parametrize("n_tris,share", mls.CASES, ids=mls.CASE_IDS)
def test_replay_equals_the_oracles_table_and_meets_the_float64_bound(oracle_mod, n_tris, share):
    sc = mls.emitters(n_tris, share)
    want = mls.emitter_count(n_tris, share)
    for order in (mls.host_order(sc), permuted_order(sc)):
        assert len(order) == want and sorted(order.tolist()) == mls.numpy_emitters64(sc).tolist()
        rep = mls.replay_table(sc, order)
        orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, flags=abi.FLAG_MESH_LIGHTS)
        orc.set_emitters(order)
        tab = orc.emitters()
        orc.close()
        assert (tab["tri"] == order).all()
        for k in ("weight", "cdf", "prob"):
            assert (bits(tab[k]) == bits(rep[k])).all(), (k, int((bits(tab[k]) != bits(rep[k])).sum()))
        assert bits(tab["total"]) == bits(rep["total"])
        if want == 0:
            continue
        cdf64, bound, total64 = mls.float64_cdf(rep["weight"], rep["total"])
        err = np.abs(rep["cdf"].astype(np.float64) - cdf64) / cdf64
        k = -(-want // 1024) + 1024
        print(f"{n_tris} x {share}: {want} emitters, max relative CDF error {err.max():.3e} (bound {bound:.3e}), W error "
              f"{abs(float(rep['total']) - total64) / total64:.3e}")
        assert (err <= bound).all()
        assert abs(float(rep["total"]) - total64) / total64 <= k * mls.U / (1 - k * mls.U)
        # (the last entry may round to either side of 1: its sum is associated by chunks, W's by threads; mesh_pick clamps for that)
        assert (np.diff(rep["cdf"]) >= 0).all() and abs(float(rep["cdf"][-1]) - 1.0) <= bound
        assert np.allclose(rep["prob"].astype(np.float64).sum(), 1.0, rtol=0, atol=want * 2 * mls.U + k * mls.U)


def test_texture_means_replay_equals_the_oracles(oracle_mod):
    sc = mls.emitters(65, "all")
    assert [(w, h, ch, flt) for (_, w, h, ch, flt) in sc.textures] == mls.EMISSION_TEXTURES
    assert {ch for (_, _, _, ch, _) in sc.textures} == {1, 2, 3, 4}
    d = sc.desc()
    for i, tex in enumerate(sc.textures):
        got = f32(oracle_mod.lib().oracle_texture_mean_luminance(d.textures[i]))
        assert bits(got) == bits(mls.texture_mean32(tex)), i
        data, w, h, ch, _ = tex
        rgb = np.zeros((h * w, 3))
        px = np.asarray(data, np.float64).reshape(h * w, ch)
        rgb[:] = px[:, :1] if ch == 1 else np.concatenate([px[:, :2], np.zeros((h * w, 1))], 1) if ch == 2 else px[:, :3]
        ref = (0.2126 * rgb[:, 0] + 0.7152 * rgb[:, 1] + 0.0722 * rgb[:, 2]).mean()
        # 5 roundings per luminance, at most ceil(texels / 256) + 8 additions per term, one division
        m = 5 + -(-h * w // 256) + 8 + 1
        assert abs(float(got) - ref) <= ref * m * mls.U / (1 - m * mls.U), i


def test_the_oracle_refuses_a_list_that_is_not_its_emitters(oracle_mod):
    sc = mls.emitters(65, 1 / 2)
    order = mls.host_order(sc)
    orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, flags=abi.FLAG_MESH_LIGHTS)
    plain = int(np.nonzero(sc.material_id == 0)[0][0])
    for bad in (order[:-1], np.concatenate([order, [plain]]), np.concatenate([order[:-1], order[:1]]), np.concatenate([order[:-1], [plain]])):
        with pytest.raises(ValueError):
            orc.set_emitters(bad.astype(np.int32))
        assert len(orc.emitters()["tri"]) == 0
    orc.set_emitters(order)
    assert (orc.emitters()["tri"] == order).all()
    orc.close()


def pick_inputs(cdf, seed=11):
    """r values of the mesh_pick known-answer test: every CDF entry, its neighbours in both directions, 0, 1.0, values above the last
    entry when it is below 1, and 2 000 uniform draws"""
    cdf = np.asarray(cdf, f32)
    r = [cdf, np.nextafter(cdf, f32(-1)), np.nextafter(cdf, f32(2)), f32([0.0, 1.0])]
    if cdf[-1] < 1:
        r.append(np.linspace(cdf[-1], 1.0, 7, dtype=f32))
    r.append(np.random.default_rng(seed).random(2000, dtype=f32))
    return np.concatenate(r).astype(f32)


def pick_reference(cdf, r):
    return np.minimum(np.searchsorted(np.asarray(cdf, f32), r, side="right"), len(cdf) - 1)


@pytest.mark.parametrize("n_tris,share", [(1, "all"), (2049, "all"), (3000, 1 / 97)])
def test_oracle_mesh_pick_is_the_first_entry_above_r(oracle_mod, n_tris, share):
    sc = mls.emitters(n_tris, share)
    orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, flags=abi.FLAG_MESH_LIGHTS)
    orc.set_emitters(mls.host_order(sc))
    cdf = orc.emitters()["cdf"]
    r = pick_inputs(cdf)
    got = np.array([orc.mesh_pick(x) for x in r])
    orc.close()
    assert (got == pick_reference(cdf, r)).all()


@functools.lru_cache(maxsize=None)
def lit_traces():
    import oracle as orc_mod
    sc = mls.lit_soup()
    order = mls.host_order(sc)
    pixels = mls.traced_pixels(sc)
    runs = {}
    for flags, mb in mls.TRACE_CONFIGS:
        orc, tr = mls.oracle_traces(orc_mod, sc, order, flags, mb, pixels)
        orc.close()
        runs[(flags, mb)] = tr
    return sc, order, runs


def test_lit_soup_is_the_scene_the_issue_describes():
    sc = mls.lit_soup()
    assert sc.tri_count >= 1000 and sc.x_res * sc.y_res <= 48 * 36      # (ER_STREAM_SPEC_MIN_TRIS: speculative samples can start)
    a, b = mls.lit_soup(), mls.lit_soup(seed=20)
    assert a.vertices.tobytes() == sc.vertices.tobytes() and a.uvs.tobytes() == sc.uvs.tobytes() and b.vertices.tobytes() != sc.vertices.tobytes()
    order = mls.host_order(sc)
    em = np.isin(sc.material_id, mls.LIT_EMISSIVE)
    assert em[mls.LIT_ZERO_AREA] and mls.LIT_ZERO_AREA not in order.tolist()
    assert sorted(order.tolist()) == [t for t in np.nonzero(em)[0].tolist() if t != mls.LIT_ZERO_AREA] == mls.numpy_emitters64(sc).tolist()
    uv = sc.uvs[sc.material_id == mls.TEX_RGB]
    assert (uv < 0).any() and (np.abs(uv) > 1).any()                    # tiled and negative on the textured emitters
    op = np.asarray(sc.textures[mls.LIT_TEX_OPACITY][0])
    assert op.min() < 0 and op.max() > 1
    assert (sc.material_id == mls.CUTOUT).mean() > 0.3
    w, h = sc.textures[mls.LIT_TEX_ONE][1:3]
    assert w & (w - 1) and h & (h - 1) and sc.textures[mls.LIT_TEX_ONE][3] == 1 and sc.textures[mls.LIT_TEX_ONE][4] == 0
    assert not (np.cross(sc.vertices[:, 1] - sc.vertices[:, 0], sc.normals[:, 0]) == 0).all()      # normals are not the face normals


def test_the_traced_samples_exercise_every_class(oracle_mod):
    sc, order, runs = lit_traces()
    for key, tr in runs.items():
        print(f"flags {key[0]} max_bounces {key[1]}: {sum(len(r) for _, _, r in tr)} records; {mls.class_counts(tr)}")
    # ER_FLAG_MIS changes no draw and no hit: its runs walk the same paths, so only the two runs without it are counted
    assert all(mls.class_counts(runs[(abi.FLAG_MIS, mb)]) == mls.class_counts(runs[(0, mb)]) for mb in (8, 2))
    distinct = mls.class_counts(runs[(0, 8)] + runs[(0, 2)])
    print("the runs without ER_FLAG_MIS:", distinct)
    for k, v in distinct.items():
        assert v >= 20, (k, v)


def test_no_traced_sample_reaches_the_clamp(oracle_mod):
    _, _, runs = lit_traces()
    for key, tr in runs.items():
        m = mls.max_unclamped(tr)
        print(f"flags {key[0]} max_bounces {key[1]}: largest unclamped component {m:.4f}")
        assert m < 10.0, (key, m)
