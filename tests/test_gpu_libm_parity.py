"""The header-independent parity check, widened.

In `er` mode the oracle and the kernel share csrc/er_math.h (six transcendentals + f2i), so a polynomial that is wrong on both
sides would pass every bit-exact test.  Here the GPU is compared with the oracle in LIBM mode -- glibc's sinf/cosf/acosf/
atan2f/powf/logf, i.e. what a CPU build of the reference computes -- under the image tolerance of SURVEY 8(c):

    per channel |d| <= 1e-3 + 1e-3 |ref| for >= 99.5 % of the pixels, image mean within 1e-4 relative.

A 1-ulp difference in one transcendental can send a path into another HDRI texel or past a triangle edge, after which that
pixel's sample is a different (equally valid) sample: such pixels are the < 0.5 % the tolerance allows, and the deeper the paths
the more of them there are.  (The reference's own vectors are in tests/test_gpu_reference_kat.py, at fixture size.)  What this adds is independence from the
shared header on every scene family of the suite, not only on the 128x128 Cornell frame.
"""
import numpy as np
import pytest

from elevenrender_amd import abi, scenes
from test_gpu_parity import gpu_render, oracle_render

pytestmark = pytest.mark.gpu


def _lit_soup():
    sc = scenes.soup(3000, 72, 56, seed=17, hdri_size=(64, 32))
    sc.point_lights = scenes.point_lights(7, seed=5)
    sc._desc = None
    return sc


CASES = {
    # name: (scene factory, spp, max_bounces, render flags)
    "soup": (lambda: scenes.soup(2000, 96, 72, seed=7, hdri_size=(64, 32)), 16, 8, 0),
    "textured16": (lambda: scenes.torture(4000, 80, 60, seed=5, n_materials=16, tex_size=32, hdri_size=(128, 64)), 16, 16, 0),
    "blobs": (lambda: scenes.blob_instances(n_instances=60, tris_per_blob=300, x_res=96, y_res=64, grid=(5, 4, 3), spacing=0.45), 16, 8, 0),
    "lit": (_lit_soup, 16, 8, abi.FLAG_POINT_LIGHTS | abi.FLAG_MIS),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_against_the_libm_oracle_within_the_image_tolerance(oracle_mod, name):
    factory, spp, mb, flags = CASES[name]
    sc = factory()
    g = gpu_render(sc, spp, max_bounces=mb, flags=flags)
    o = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_LIBM, max_bounces=mb, threads=8, flags=flags)
    o.render(spp)
    ref = o.read_pass(0)
    o.close()
    img = g["beauty"]
    d = np.abs(img - ref)
    tol = 1e-3 + 1e-3 * np.abs(ref)
    within = (d <= tol).all(-1).mean()
    exact = (img.view(np.uint32) == ref.view(np.uint32)).all(-1).mean()
    gm, om = img[..., :3].mean((0, 1)), ref[..., :3].mean((0, 1))
    rel = np.abs(gm - om) / np.maximum(np.abs(om), 1e-12)
    print(f"{name} vs libm oracle: {exact:.4f} of pixels bit-identical, {within:.4f} within 1e-3 + 1e-3|ref|, max|d| {d.max():.3e}, mean rel diff {rel.max():.2e}")
    assert np.isfinite(img).all()
    assert within >= 0.995, f"{name}: only {within:.4f} of the pixels within the image tolerance"
    # per-channel image mean: 1e-4 relative widened by the Monte-Carlo noise of the few diverged samples:
    # a diverged pixel differs by up to its clamp range (10) / (spp + 1); bound = share of such pixels * that, relative to the mean
    bound = 1e-4 + (1.0 - within) * 10.0 / (spp + 1) / max(float(om.mean()), 1e-6)
    assert (rel <= bound).all(), f"{name}: image mean {gm} vs {om}"
