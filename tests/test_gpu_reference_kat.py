"""The HIP path against vectors recorded from the REFERENCE's own code (tests/golden/reference_*.npz, `*_er`: the reference's
sources compiled on the host with er_math.h's six functions under the sycl:: math names -- tests/golden/make_golden_reference.py).

Reads tests/golden/ only: neither the oracle nor oracle/_ref/ is involved, so a misreading of the reference that the oracle and
the kernels share cannot hide here.  Bit for bit, NaN matching NaN, no tolerances:
  * er_debug_eval for every device function of tests/test_gpu_function_kat.py's FN on the recorded inputs (ER_FN_MATH excepted:
    the six functions are not the reference's code; their GPU and CPU builds are compared in test_transcendentals);
  * er_debug_trace_rays (the production traversal) and er_debug_closest_hit (the exact routine) against the recorded throwRay
    hits: the same triangle, the same Hit.position (7 box-corner rays, where the reference's own tree drops the nearest triangle,
    are kept apart and compared with the reference's Tri::hit over every triangle: DESIGN.md 1);
  * whole renders of the two golden scenes in the three schedules: every plane, the sample counts, the RNG states."""
import os

import numpy as np
import pytest

from elevenrender_amd import abi, render
from golden_util import GOLDEN_DIR, load, scene_from
from test_gpu_function_kat import FN, ibits, same

pytestmark = pytest.mark.gpu

TRACE_SCENE = "torture_300tri_32x24_4spp"      # the closest-hit rays were recorded on this golden's scene


def first_bad(ok):
    return np.argwhere(~np.asarray(ok))[:5].tolist()


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN_DIR, "reference_functions.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def rm(fx):
    sc, _, _ = scene_from(fx, "rig_")
    # known-answer tests of the fetch on the textures as they came: the scalar-channel compaction off (see test_gpu_function_kat.py)
    before = os.environ.get("ER_TEX_COMPACT")
    os.environ["ER_TEX_COMPACT"] = "0"
    try:
        m = render.RenderingManager(render.RenderParameters(max_bounces=5))
        m.start_rendering(sc)
    finally:
        if before is None:
            del os.environ["ER_TEX_COMPACT"]
        else:
            os.environ["ER_TEX_COMPACT"] = before
    yield m
    m.close()


def test_rng_streams(rm, fx):
    out = rm.debug_eval(FN["RNG"], ibits(fx["rng_idx"].astype(np.int32)).reshape(-1, 1), 32)
    assert same(out[:, :16], fx["rng_values_er"]).all()
    assert (out[:, 16:].view(np.uint32) == fx["rng_states_er"]).all()


def test_camera_rays(rm, fx):
    ok = same(rm.debug_eval(FN["CAMERA_RAY"], fx["cam_items"], 6), fx["cam_rays_er"]).all(1)
    assert ok.all(), first_bad(ok)


def test_tri_hit_records(rm, fx):
    out = rm.debug_eval(FN["TRI_HIT"], fx["trihit_items"], 18)
    hit = fx["trihit_ok_er"] == 1
    assert ((out[:, 0] == 1.0) == hit).all(), first_bad((out[:, 0] == 1.0) == hit)
    ok = same(out[hit, 1:], fx["trihit_rec_er"][hit]).all(1)
    assert ok.all(), first_bad(ok)


def test_tri_hit_records_with_varied_uvs_and_signs():
    """reference_trihit_uv.npz: the reference's Tri::hit on per-triangle uvs (mirrored, several periods wide, negative) and tangent
    signs of both kinds -- full_hit's uv interpolation and its signed bitangent (csrc/er_device.h) against src/Tri.h:76,136 itself"""
    import copy
    z = np.load(os.path.join(GOLDEN_DIR, "reference_trihit_uv.npz"), allow_pickle=False)
    sc = copy.copy(load(TRACE_SCENE)[0])
    sc._desc = None
    for k in ("vertices", "normals", "tangents", "uvs", "tangent_sign"):
        a = np.ascontiguousarray(z["rig_" + k])
        assert a.shape == getattr(sc, k).shape, k
        setattr(sc, k, a)
    m = render.RenderingManager(render.RenderParameters(max_bounces=5))
    m.start_rendering(sc)
    try:
        out = m.debug_eval(FN["TRI_HIT"], z["trihit_items"], 18)
    finally:
        m.close()
    hit = z["trihit_ok_er"] == 1
    assert ((out[:, 0] == 1.0) == hit).all(), first_bad((out[:, 0] == 1.0) == hit)
    ok = same(out[hit, 1:], z["trihit_rec_er"][hit]).all(1)
    assert ok.all(), (first_bad(ok), out[hit][~ok][:2], z["trihit_rec_er"][hit][~ok][:2])
    assert hit.sum() > len(hit) // 2


def test_disney_eval_pdf_sample(rm, fx):
    it = fx["disney_items"]
    for kind, items, ref in (("DISNEY_EVAL", it, fx["disney_eval_er"]), ("DISNEY_PDF", it, fx["disney_pdf_er"].reshape(-1, 1)),
                             ("DISNEY_SAMPLE", np.concatenate([it[:, :26], fx["disney_rs"]], 1), fx["disney_sample_er"])):
        ok = same(rm.debug_eval(FN[kind], items, ref.shape[1]), ref).all(1)
        assert ok.all(), (kind, first_bad(ok))


def test_spherical_mappings(rm, fx):
    ok = same(rm.debug_eval(FN["SPHERICAL"], fx["sph_p"], 2), fx["sph_uv_er"]).all(1)
    assert ok.all(), first_bad(ok)
    ok = same(rm.debug_eval(FN["REV_SPHERICAL"], fx["rev_uv"], 3), fx["rev_p_er"]).all(1)
    assert ok.all(), first_bad(ok)


def test_texture_fetches(rm, fx):
    ok = same(rm.debug_eval(FN["TEXTURE"], fx["texfetch_items"], 3), fx["texfetch_er"]).all(1)
    assert ok.all(), first_bad(ok)


def test_hdri_search_and_pdf(rm, fx):
    got = rm.debug_eval(FN["HDRI_SEARCH"], fx["hdri_search_vals"].reshape(-1, 1), 1).view(np.int32).reshape(-1)
    assert (got == fx["hdri_search_er"]).all(), first_bad(got == fx["hdri_search_er"])
    got = rm.debug_eval(FN["HDRI_PDF"], ibits(fx["hdri_pdf_xy"]), 1).reshape(-1)
    ok = same(got, fx["hdri_pdf_er"])
    assert ok.all(), first_bad(ok)


def test_closest_hits_of_throw_ray(fx):
    sc, _, _, _ = load(TRACE_SCENE)
    m = render.RenderingManager(render.RenderParameters(max_bounces=5))
    m.start_rendering(sc)
    try:
        o, d = fx["closest_o"], fx["closest_d"]
        tri, slot, pos, dist, info = m.debug_trace_rays(o, d)
        tri2, pos2, dist2 = m.debug_closest_hit(o, d)
        gtri, _, gpos, _, _ = m.debug_trace_rays(fx["graze_o"], fx["graze_d"])
    finally:
        m.close()
    for what, t, p in (("production traversal", tri, pos), ("exact routine", tri2, pos2)):
        print(f"{what}: {int((t >= 0).sum())} hits, {int((t != fx['closest_tri_er']).sum())} other triangles, "
              f"{int((~same(p, fx['closest_pos_er']).all(1)).sum())} other positions")
        assert (t == fx["closest_tri_er"]).all(), (what, first_bad(t == fx["closest_tri_er"]))
        hit = t >= 0
        ok = same(p[hit], fx["closest_pos_er"][hit]).all(1)
        assert ok.all(), (what, first_bad(ok))
    # The box-corner rays (items graze_index of the first recording): the reference's own tree drops the nearest
    # triangle on the rounding of its slab test, which no other tree can reproduce; the HIP path gives what the reference's Tri::hit
    # over every triangle gives.
    assert (gtri == fx["graze_alltri_er"]).all() and same(gpos, fx["graze_allpos_er"]).all(), (gtri, fx["graze_alltri_er"])


@pytest.mark.parametrize("flags", [0, abi.FLAG_WAVEFRONT, abi.FLAG_MEGAKERNEL], ids=["streaming", "wavefront", "megakernel"])
@pytest.mark.parametrize("name", ["cornell_32x32", "torture_300tri_32x24"])
def test_whole_path_render(name, flags):
    sc, _, _, _ = load(name + "_4spp")
    z = np.load(os.path.join(GOLDEN_DIR, f"reference_{name}.npz"), allow_pickle=False)
    m = render.RenderingManager(render.RenderParameters(max_bounces=int(z["max_bounces"][0]), flags=flags))
    m.start_rendering(sc)
    try:
        m.render(int(z["spp"][0]))
        planes = {p: m.get_pass(p) for p in abi.PASS_NAMES}
        samples, rng = m.read_samples(), m.read_rng()
    finally:
        m.close()
    for p, got in planes.items():
        ok = same(got, z[f"pass_{p}_er"]).all(-1)
        print(f"{name} {p}: {int((~ok).sum())} of {ok.size} pixels differ")
        assert ok.all(), (p, int((~ok).sum()), first_bad(ok))
    assert (samples == z["samples_er"]).all() and (rng == z["rng_er"]).all()
