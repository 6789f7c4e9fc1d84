"""The variance plane and the denoise guided by it on the GPU (er_variance_fold / er_variance_info / er_read_variance /
er_denoise_variance: csrc/er_variance.hip and csrc/er_variance.h).

(1) the plane and the two pixel counts word for word against a numpy replay (elevenrender_amd/variance.py) fed the BEAUTY and the counts
read after every call, with and without adaptive sampling; (2) DENOISE word for word against the replay of split, levels with the
propagated variance and join; (3) a render with all of it in between equals the render without, in every schedule; (4) what resets the
moments; (5) what is refused; (6) the filtered frame is nearer the converged one than the unfiltered frame."""
import ctypes as C
import functools

import numpy as np
import pytest

from elevenrender_amd import abi, render, scenes, variance
from test_gpu_adaptive import replay_errors
from test_gpu_update import PLANES, SCHEDULES

pytestmark = pytest.mark.gpu
f32 = np.float32
INV, STATE = abi.ER_ERR_INVALID_ARG, abi.ER_ERR_STATE
bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)
CALLS = (1, 2, 3, 2)
AD_MIN, AD_INTERVAL = 4, 2


def manager(sc, flags=0, max_bounces=4, **kw):
    rm = render.RenderingManager(render.RenderParameters(max_bounces=max_bounces, flags=flags, **kw))
    rm.start_rendering(sc)
    return rm


def assert_words(got, want, what):
    bad = int((bits(got).reshape(-1, 4) != bits(want).reshape(-1, 4)).any(1).sum())
    assert bad == 0, f"{what}: {bad} pixels differ from the replay"


def fold_and_check(rm, st, calls, what):
    """`calls` samples at a time, a fold after each; the plane and the counts against the replay after every fold.  Returns the replay's
    state."""
    for i, n in enumerate(calls):
        rm.render(n)
        beauty, samples = rm.get_pass("beauty"), rm.read_samples()
        rm.variance_fold()
        st, folded = variance.fold(st, beauty, samples)
        assert_words(rm.get_variance(), variance.value(st, samples), f"{what}, fold {i}")
        info = rm.variance_info()
        K = st.view(np.uint32)[:, 11]
        assert (info["pixels_folded"], info["pixels_known"]) == (int(folded.sum()), int((K >= 2).sum())), (what, i, info)
        assert info["fold_ms"] > 0
    return st


def filter_and_check(rm, st, sc, what, **par):
    """er_denoise_variance against the replay from the planes as they are read now"""
    rm.render_features()
    rm.denoise_variance(**par)
    got = rm.get_pass("denoise")
    beauty, samples, normal = rm.get_pass("beauty"), rm.read_samples(), rm.get_pass("normal")
    want = variance.denoise(beauty, samples, st, normal, rm.get_feature("albedo"), rm.get_feature("depth"), sc.x_res, sc.y_res, **par)
    assert_words(got, want, what)
    assert np.isfinite(got).all() and (got[..., 3] == beauty[..., 3]).all() and (bits(got) != bits(beauty)).any()
    assert rm.variance_info()["filter_ms"] > 0
    return got


# ---- (1) ----

def test_fold_equals_the_replay():
    sc = scenes.cornell_textured(44, 28)          # neither side a multiple of 8 or 16: partial tiles, partial 16 x 16 blocks, 5 workgroups of 256
    npx = sc.x_res * sc.y_res
    rm = manager(sc)
    try:
        assert rm.variance_info() == dict(folds=0, pixels_folded=0, pixels_known=0, fold_ms=0.0, filter_ms=0.0)
        assert (rm.get_variance() == 0).all()                                                # no fold yet: K = 0 everywhere
        st = fold_and_check(rm, variance.start(npx), CALLS, "uniform")
        K = st.view(np.uint32)[:, 11]
        assert rm.variance_info()["folds"] == len(CALLS) and (K == len(CALLS)).all()
        v = rm.get_variance()
        assert (v[..., 3] == len(CALLS)).all() and (v[..., :3] >= 0).all() and (v[..., :3] > 0).any()
        # samples after the last fold change M, not the moments
        rm.render(3)
        samples = rm.read_samples()
        assert_words(rm.get_variance(), variance.value(st, samples), "three samples after the last fold")
        assert rm.variance_info()["folds"] == len(CALLS)
    finally:
        rm.close()


def adaptive_threshold(sc):
    """The adaptive metric alone, replayed in numpy from the planes of a plain render at the snapshot (2 samples) and the first test (4):
    the median of the tiles' errors stops about half of them there."""
    rm = manager(sc)
    try:
        state = lambda: {"beauty": rm.get_pass("beauty"), "samples": rm.read_samples().reshape(sc.y_res, sc.x_res)}
        rm.render(AD_MIN - AD_INTERVAL)
        snap = state()
        rm.render(AD_INTERVAL)
        tiles = np.arange(((sc.x_res + 7) // 8) * ((sc.y_res + 7) // 8))
        e = replay_errors(sc, tiles, snap, state())
    finally:
        rm.close()
    return float(np.median(e[e >= 0]))


@functools.lru_cache(maxsize=None)
def adaptive_frame_threshold():
    return adaptive_threshold(scenes.cornell_textured(44, 28))


def test_fold_and_filter_equal_the_replay_under_adaptive_sampling():
    """min_samples 4, interval 2, calls of 1, 2, 3, 2: the test at 4 samples stops some tiles, which then have n = 1 in the third fold and
    n = 0 in the fourth -- their words stay and their K is one behind."""
    sc = scenes.cornell_textured(44, 28)
    npx = sc.x_res * sc.y_res
    rm = manager(sc)
    try:
        rm.set_adaptive(adaptive_frame_threshold(), AD_MIN, AD_INTERVAL)
        st = fold_and_check(rm, variance.start(npx), CALLS, "adaptive")
        _, spp = rm.tile_state()
        stopped, active = int((spp < sum(CALLS)).sum()), int((spp == sum(CALLS)).sum())
        assert stopped > 0 and active > 0, f"the threshold left {stopped} stopped and {active} active tiles"
        K = st.view(np.uint32)[:, 11]
        info = rm.variance_info()
        assert len(set(K.tolist())) >= 2 and 0 < info["pixels_folded"] < npx and info["pixels_known"] == npx
        filter_and_check(rm, st, sc, "adaptive frame, 5 levels")
    finally:
        rm.close()


def test_centres_without_a_variance_take_no_colour_stop():
    """calls of 4, 2, 2 under the same sampler: a tile stopped at the first test has one batch (K = 1) however many folds follow, so
    the filter runs with K < 2 centres beside known ones"""
    sc = scenes.cornell_textured(44, 28)
    npx = sc.x_res * sc.y_res
    rm = manager(sc)
    try:
        rm.set_adaptive(adaptive_frame_threshold(), AD_MIN, AD_INTERVAL)
        st = fold_and_check(rm, variance.start(npx), (4, 2, 2), "adaptive, late folds")
        K = st.view(np.uint32)[:, 11]
        assert (K == 1).any() and (K >= 2).any() and rm.variance_info()["pixels_known"] == int((K >= 2).sum())
        v = rm.get_variance().reshape(-1, 4)
        assert (v[K == 1, :3] == 0).all()
        filter_and_check(rm, st, sc, "K < 2 centres", levels=3)
    finally:
        rm.close()


# ---- (2) ----

@pytest.fixture(scope="module")
def folded_frame():
    sc = scenes.cornell_textured(48, 40)          # at level 5 the step-16 taps reach 32 pixels: they clamp on both axes
    rm = manager(sc)
    st = fold_and_check(rm, variance.start(sc.x_res * sc.y_res), CALLS, "48 x 40")
    yield rm, st, sc
    rm.close()


@pytest.mark.parametrize("levels,sigmas", [(1, (0.0, 0.0, 0.0)), (3, (2.0, 0.1, 0.05)), (5, (0.0, 0.0, 0.0))])
def test_filter_equals_the_replay(folded_frame, levels, sigmas):
    rm, st, sc = folded_frame
    got = filter_and_check(rm, st, sc, f"{levels} levels", levels=levels, colour_sigma=sigmas[0], albedo_sigma=sigmas[1], depth_sigma=sigmas[2])
    if levels == 5 and sigmas == (0.0, 0.0, 0.0):                                            # 0 names the defaults
        rm.denoise_variance()
        assert (bits(rm.get_pass("denoise")) == bits(got)).all()
        rm.denoise_variance(5, 6.0, 0.3, 0.2)
        assert (bits(rm.get_pass("denoise")) == bits(got)).all()
    # the other two filters are what they were: they do not read the variance
    rm.denoise_guided()
    a = rm.get_pass("denoise")
    rm.variance_fold()
    rm.denoise_guided()
    assert (bits(a) == bits(rm.get_pass("denoise"))).all()


# ---- (3) ----

def render_outputs(rm):
    out = {p: rm.get_pass(p).view(np.uint32) for p in PLANES if p != "denoise"}
    out["samples"], out["rng"] = rm.read_samples(), rm.read_rng()
    return out, rm.counters(), rm.get_render_info().samples


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_variance_leaves_the_render_alone(sched):
    sc = scenes.cornell_textured(44, 28)
    got = []
    for with_variance in (True, False):
        rm = manager(sc, SCHEDULES[sched])
        try:
            if with_variance:
                rm.render_features()
                for n in (3, 2, 3):
                    rm.render(n)
                    rm.variance_fold()
                    rm.get_variance()
                    if rm.variance_info()["folds"] >= 2:
                        rm.denoise_variance()
            else:
                rm.render_features()
                rm.render(8)
            got.append(render_outputs(rm))
        finally:
            rm.close()
    for k in got[0][0]:
        assert (got[0][0][k] == got[1][0][k]).all(), f"{sched}: {k} differs"
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2]


# ---- (4) ----

def test_what_resets_the_moments():
    sc = scenes.cornell_textured(44, 28)
    npx = sc.x_res * sc.y_res
    lib = abi.load()
    cam = abi.ErCamera.from_buffer_copy(sc.camera)
    cam.position = abi.ErVec3(sc.camera.position.x + 0.02, sc.camera.position.y, sc.camera.position.z - 0.03)
    V = sc.vertices.reshape(-1, 3, 3)
    mats = [abi.ErMaterial.from_buffer_copy(m) for m in sc.materials]
    identity = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(f32)
    moved = identity.copy()
    moved[0, 3] = 0.01
    rm = manager(sc)
    try:
        rm.set_objects([np.arange(0, 4, dtype=np.uint32)])

        def armed():
            """at least two folds and a filtered frame, whatever went before"""
            for n in (2, 1):
                rm.render(n)
                rm.variance_fold()
            rm.render_features()
            rm.denoise_variance()
            assert rm.variance_info()["folds"] >= 2 and rm.variance_info()["pixels_known"] == npx

        def after_reset(what, st):
            info = rm.variance_info()
            assert (info["folds"], info["pixels_folded"], info["pixels_known"]) == (0, 0, 0), (what, info)
            assert (rm.get_variance() == 0).all(), what
            rm.render_features()                                                             # (an edit drops the features too: the refusal below is the folds')
            assert lib.er_denoise_variance(rm.handle, C.byref(abi.ErDenoiseVariance(0, 0.0, 0.0, 0.0))) == STATE, what
            assert b"folds" in lib.er_last_error(), what
            st = fold_and_check(rm, st, (2,), what)
            assert lib.er_denoise_variance(rm.handle, C.byref(abi.ErDenoiseVariance(0, 0.0, 0.0, 0.0))) == STATE, what      # one fold only
            st = fold_and_check(rm, st, (1,), what)
            rm.denoise_variance()

        resets = {
            "update camera": lambda: rm.update(camera=cam),
            "update vertices": lambda: rm.update(vertices=V),
            "update sparse": lambda: rm.update(tri_ids=np.array([3, 4], np.uint32), vertices=V[[3, 4]]),
            "edit materials": lambda: rm.edit(materials=mats),
            "transform": lambda: rm.transform({0: moved}),
            "topology": lambda: rm.topology(remove=np.array([sc.tri_count - 1], np.uint32)),
        }
        for what, call in resets.items():
            armed()
            call()
            after_reset(what, variance.start(npx))
        armed()
        rm.start_rendering(sc)                                                               # er_render_begin
        after_reset("start_rendering", variance.start(npx))
        # er_state_import: the first batch is measured from the imported planes
        rm.render(3)
        blob = rm.state_export()
        beauty3, samples3 = rm.get_pass("beauty"), rm.read_samples()
        armed()
        rm.state_import(blob)
        assert (bits(rm.get_pass("beauty")) == bits(beauty3)).all()
        after_reset("state_import", variance.mark(beauty3, samples3))
        # samples, features, ids and the history calls leave the state alone
        rm.history_capture()
        rm.update(camera=cam, keep_history=False)                                           # (this one resets ...)
        assert rm.variance_info()["folds"] == 0
        st = fold_and_check(rm, variance.start(npx), (2, 2), "after the camera")
        rm.history_resolve()
        rm.get_blended()
        rm.render_features()
        rm.render_ids()
        assert rm.variance_info()["folds"] == 2                                              # (... and these do not)
        assert_words(rm.get_variance(), variance.value(st, rm.read_samples()), "after features, ids and history")
    finally:
        rm.close()


# ---- (5) ----

def test_refusals():
    sc = scenes.cornell_textured(44, 28)
    lib = abi.load()
    par = abi.ErDenoiseVariance(0, 0.0, 0.0, 0.0)
    rm = manager(sc)
    try:
        rm.render(2)
        rm.variance_fold()
        rm.render(2)
        rm.variance_fold()
        assert lib.er_denoise_variance(rm.handle, C.byref(par)) == STATE                     # no features
        assert b"feature" in lib.er_last_error()
        rm.render_features()
        rm.denoise_variance()
        for bad in ((9, 0.0, 0.0, 0.0), (0, -1.0, 0.0, 0.0), (0, 0.0, -0.5, 0.0), (0, 0.0, 0.0, -0.1), (0, float("nan"), 0.0, 0.0), (0, 0.0, float("nan"), 0.0),
                    (0, 0.0, 0.0, float("nan"))):
            assert lib.er_denoise_variance(rm.handle, C.byref(abi.ErDenoiseVariance(*bad))) == INV, bad
        rm.denoise_variance(8, 1.0, 1.0, 1.0)                                                # the most levels
        rm.start_rendering(sc)
        rm.render_features()
        rm.render(2)
        rm.variance_fold()
        assert lib.er_denoise_variance(rm.handle, C.byref(par)) == STATE                     # one fold only
        assert b"folds" in lib.er_last_error()
    finally:
        rm.close()
    rm = manager(sc, max_bounces=1, rank=0, world=2)
    try:
        plane = np.zeros(sc.y_res * sc.x_res * 4, f32)
        info = abi.ErVarianceInfo()
        assert lib.er_variance_fold(rm.handle) == STATE
        assert b"sharded" in lib.er_last_error()
        assert lib.er_variance_info(rm.handle, C.byref(info)) == STATE
        assert lib.er_read_variance(rm.handle, plane.ctypes.data_as(C.POINTER(C.c_float))) == STATE
        assert lib.er_denoise_variance(rm.handle, C.byref(par)) == STATE
    finally:
        rm.close()


# ---- (6) ----

def test_the_variance_guided_frame_is_nearer_the_converged_one_than_the_unfiltered():
    """cornell_textured 96 x 96: 16 spp in folds of 2 against 1 024 spp, every image scaled by samples / (samples - 1) (the setup sample).
    Asserted: the mean absolute error of er_denoise_variance at its defaults is below the unfiltered frame's.  Printed, not asserted: its
    ratio to er_denoise_guided at defaults and at the best colour_sigma of a sweep."""
    sc = scenes.cornell_textured(96, 96)
    rm = manager(sc, max_bounces=5)
    try:
        rm.render(16, fold_every=2)
        assert rm.variance_info()["folds"] == 8
        rm.render_features()
        scale = f32(17.0 / 16.0)
        image = lambda: rm.get_pass("denoise")[..., :3].astype(np.float64) * scale
        plain = rm.get_pass("beauty")[..., :3].astype(np.float64) * scale
        rm.denoise_variance()
        by_variance = image()
        swept = {}
        for s in (2.0, 3.0, 4.0):
            rm.denoise_variance(colour_sigma=s)
            swept[s] = image()
        rm.denoise_guided()
        guided = image()
        sweep = {}
        for s in (0.5, 1.0, 2.0, 4.0, 8.0, 16.0):
            rm.denoise_guided(colour_sigma=s)
            sweep[s] = image()
        rm.render(1024 - 16)
        truth = rm.get_pass("beauty")[..., :3].astype(np.float64) * (1025.0 / 1024.0)
    finally:
        rm.close()
    err = lambda a: float(np.abs(a - truth).mean())
    e_plain, e_var, e_guided = err(plain), err(by_variance), err(guided)
    best = min(sweep, key=lambda s: err(sweep[s]))
    print(f"mean absolute error against 1024 spp: unfiltered {e_plain:.5f}, er_denoise_variance {e_var:.5f} (x{e_var / e_plain:.3f}), "
          f"er_denoise_guided defaults {e_guided:.5f} (variance / guided {e_var / e_guided:.3f}), best guided colour_sigma {best}: {err(sweep[best]):.5f} "
          f"(variance / best guided {e_var / err(sweep[best]):.3f}); er_denoise_variance at colour_sigma " + ", ".join(f"{s}: {err(a):.5f}" for s, a in swept.items()))
    assert e_var < e_plain
