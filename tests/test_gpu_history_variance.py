"""The variance carried through the history on the GPU (er_history_capture / er_history_resolve with a folded scene, er_read_history_variance,
er_read_blended_variance, er_denoise_blended, er_history_variance_info: csrc/er_history_variance.hip and csrc/er_history_variance.h).

(1) the carried plane, the blend's variance and DENOISE word for word against the numpy replay (tests/history_variance_replay.py), fed the
BEAUTY and sample counts read at every fold point and before the capture, for a moved camera, posed objects, both, and the same camera
again; (2) three edits with 2 samples each, the carried plane surviving them, the known counts and ErHistoryVarianceInfo against the
replay's; (3) the history, the blend and the render are the same bits with and without all of it; (4) a capture with a pending restart
carries nothing; (5) states and arguments; (6) the denoised blend is nearer the converged frame than the blend."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_history as gh
from elevenrender_amd import abi, history, render, scenes
from history_variance_replay import Replay, steps
from test_gpu_update import PLANES, SCHEDULES

pytestmark = pytest.mark.gpu
f32 = np.float32
INV, STATE = abi.ER_ERR_INVALID_ARG, abi.ER_ERR_STATE
bits = gh.bits
assert_words = gh.assert_words


def read(rm):
    return rm.get_pass("beauty"), rm.read_samples()


def first_frame(rm, rp, folds=4, per=2):
    """`folds` batches of `per` samples, the replay fed at every fold point; returns the last read"""
    for _ in range(folds):
        rm.render(per)
        beauty, samples = read(rm)
        rm.variance_fold()
        rp.fold(beauty, samples)
    return beauty, samples


def move(rm, rp, camera, poses):
    """capture, edit, resolve on the handle and in the replay; returns the objects the replay saw move"""
    beauty, samples = read(rm)
    rm.history_capture(max_weight=rp.max_weight)
    rp.capture(beauty, samples)
    gh.edit(rm, camera, poses)
    rp.edit(camera, poses)
    rm.history_resolve()
    return rp.resolve()


def check_info(rm, rp, blended=None):
    info = rm.history_variance_info()
    known_sv, known_hv = rp.known()
    want = dict(captured=int(rp.sv is not None), resolved=int(rp.hv is not None), pixels_known_captured=known_sv, pixels_known_history=known_hv)
    assert {k: info[k] for k in want} == want, (info, want)
    if blended is not None:
        assert info["pixels_known_blended"] == blended, (info, blended)
    return info


# ---- (1) ----

@pytest.mark.parametrize("name", gh.NAMES)
def test_carried_variance_blend_variance_and_denoise_equal_the_replay(name):
    sc = gh.scene(name)
    for case in ("camera", "objects", "both", "same"):
        rm = gh.history_manager(sc)
        rp = Replay(name)
        try:
            first_frame(rm, rp)
            moved = move(rm, rp, *gh.moves(name, case))
            what = f"{name} {case}"
            assert_words(rm.get_history(), rp.hist, what + " history")                      # the colour is what it was
            assert_words(rm.get_history_variance(), rp.hv, what + " history variance")
            assert rm.history_info()["moved_objects"] == moved
            check_info(rm, rp, blended=0)
            rm.render(2)
            beauty, samples = read(rm)
            want_vb = rp.blended_variance(samples)
            assert_words(rm.get_blended_variance(), want_vb, what + " blended variance")
            assert_words(rm.get_history_variance(), rp.hv, what + " history variance after two samples")
            info = check_info(rm, rp, blended=int((want_vb[:, 3] != 0).sum()))
            assert 0 < info["pixels_known_history"] < rp.npx or case == "same"
            rm.render_features()
            normal, albedo, depth = rm.get_pass("normal"), rm.get_feature("albedo"), rm.get_feature("depth")
            for par in (dict(levels=1), dict(), dict(levels=2, colour_sigma=3.0, albedo_sigma=0.5, depth_sigma=0.1)):
                rm.denoise_blended(**par)
                got = rm.get_pass("denoise")
                assert_words(got, rp.denoise(beauty, samples, normal, albedo, depth, **par), f"{what} denoise {par}")
                assert (got[..., 3] == 1).all()
            info = rm.history_variance_info()
            assert info["filter_ms"] > 0 and info["pixels_known_blended"] == int((want_vb[:, 3] != 0).sum())
            assert_words(rm.get_blended(), history.blend(beauty, samples, rp.hist), what + " blend")      # and so is the blend
        finally:
            rm.close()


# ---- (2) ----

def test_the_carried_plane_survives_three_edits():
    """`large`: 8 samples in folds of 2, then three edits with 2 samples and one fold each, so the current K < 2 after the first frame and
    everything the blend knows of its variance came through the history.  tests/test_history_variance_cpu.py checks on the CPU that the
    last resolve holds at least 20 pixels of every way the variance can arrive."""
    name = "large"
    rm = gh.history_manager(gh.scene(name))
    rp = Replay(name)
    try:
        first_frame(rm, rp)
        known = []
        for k, (camera, poses) in enumerate(steps(name)):
            move(rm, rp, camera, poses)
            assert_words(rm.get_history(), rp.hist, f"edit {k} history")
            assert_words(rm.get_history_variance(), rp.hv, f"edit {k} history variance")
            check_info(rm, rp)
            known.append(rp.known())
            first_frame(rm, rp, folds=1)                                                     # one fold: K = 1, nothing known of the current frame
            assert rm.variance_info()["pixels_known"] == 0
            beauty, samples = read(rm)
            want_vb = rp.blended_variance(samples)
            assert_words(rm.get_blended_variance(), want_vb, f"edit {k} blended variance")
            assert (bits(want_vb[:, 3]) == bits(rp.hv[:, 3])).all()                          # known exactly where the history is
            check_info(rm, rp, blended=int((want_vb[:, 3] != 0).sum()))
        print("known pixels (captured, history) per edit:", known, "coverage of the last resolve:", rp.coverage())
        assert known[0][0] == rp.npx and all(0 < h <= c for c, h in known) and known[2][1] >= 0.3 * rp.npx
        cov = rp.coverage()
        assert all(cov[k] >= 20 for k in cov), cov
        rm.render_features()
        rm.denoise_blended()
        assert_words(rm.get_pass("denoise"), rp.denoise(beauty, samples, rm.get_pass("normal"), rm.get_feature("albedo"), rm.get_feature("depth")), "denoise after three edits")
    finally:
        rm.close()


# ---- (3) ----

def render_outputs(rm):
    out = {p: rm.get_pass(p).view(np.uint32) for p in PLANES if p != "denoise"}
    out["samples"], out["rng"] = rm.read_samples(), rm.read_rng()
    return out, rm.counters(), rm.get_render_info().samples


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_nothing_else_moves(sched):
    """the same sequence on a handle that folded, on one that never did, and on one with none of these calls"""
    sc = gh.scene("large")
    camera, poses = gh.moves("large", "both")
    seen, got = {}, {}
    for mode in ("folded", "never folded", "plain"):
        rm = gh.history_manager(sc, SCHEDULES[sched], max_bounces=4)
        try:
            for _ in range(2):
                rm.render(2)
                if mode == "folded":
                    rm.variance_fold()
            if mode != "plain":
                rm.history_capture()
            gh.edit(rm, camera, poses)
            if mode != "plain":
                rm.history_resolve()
                hv = rm.get_history_variance()
            rm.render(2)
            if mode != "plain":
                rm.render_features()
                rm.denoise_blended()
                info = rm.history_info()
                seen[mode] = dict(history=rm.get_history(), blended=rm.get_blended(), classes={k: info["pixels_" + k] for k in history.CLASS_NAMES}, hv=hv,
                                  vb=rm.get_blended_variance(), info=rm.history_variance_info())
            got[mode] = render_outputs(rm)
        finally:
            rm.close()
    a, b = seen["folded"], seen["never folded"]
    assert (bits(a["history"]) == bits(b["history"])).all() and (bits(a["blended"]) == bits(b["blended"])).all() and a["classes"] == b["classes"]
    assert (a["info"]["captured"], a["info"]["resolved"]) == (1, 1) and a["info"]["pixels_known_history"] > 0 and (a["hv"][..., 3] == 1).any()
    assert (b["info"]["captured"], b["info"]["resolved"]) == (0, 0) and b["info"]["pixels_known_history"] == b["info"]["pixels_known_blended"] == 0
    assert not bits(b["hv"]).any() and not bits(b["vb"]).any()
    for mode in ("folded", "never folded"):
        gh.assert_same_outputs(got[mode][0], got["plain"][0], f"{sched} {mode}")
        assert got[mode][1] == got["plain"][1] and got[mode][2] == got["plain"][2]


# ---- (4) ----

def test_a_capture_with_a_pending_restart_carries_nothing():
    name = "small"
    sc = gh.scene(name)
    rm = gh.history_manager(sc)
    rp = Replay(name)
    cam = gh.camera_of(sc, (0.02, 0.0, -0.03))
    try:
        first_frame(rm, rp)
        assert rm.variance_info()["pixels_known"] == rp.npx
        rm.update(camera=cam)                                    # the moments are now the previous frame's; no fold follows
        rp.edit(cam, {})
        rm.render(2)
        move(rm, rp, gh.camera_of(sc, (0.04, 0.0, -0.05)), {})
        info = check_info(rm, rp)
        assert (info["captured"], info["resolved"], info["pixels_known_captured"], info["pixels_known_history"]) == (1, 1, 0, 0)      # carried, and nothing known in it
        hv = rm.get_history_variance()
        assert not bits(hv).any() and rm.get_history()[..., 3].max() > 0
        rm.render(2)
        assert not bits(rm.get_blended_variance()).any()
        # the same capture after one fold of the new frame carries nothing either (K = 1), after two it does
        first_frame(rm, rp, folds=1)
        move(rm, rp, gh.camera_of(sc, (0.02, 0.0, -0.03)), {})
        assert check_info(rm, rp)["pixels_known_history"] == 0
        first_frame(rm, rp, folds=2)
        move(rm, rp, gh.camera_of(sc, (0.04, 0.0, -0.05)), {})
        assert check_info(rm, rp)["pixels_known_history"] > 0
        assert_words(rm.get_history_variance(), rp.hv, "after two folds")
    finally:
        rm.close()


# ---- (5) ----

def refused(rm, sc, par=None):
    lib = abi.load()
    plane = np.zeros(sc.y_res * sc.x_res * 4, f32)
    fp = plane.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.er_read_history_variance(rm.handle, fp) == STATE
    assert b"resolve" in lib.er_last_error()
    assert lib.er_read_blended_variance(rm.handle, fp) == STATE
    assert lib.er_denoise_blended(rm.handle, C.byref(par or abi.ErDenoiseVariance(0, 0.0, 0.0, 0.0))) == STATE
    info = rm.history_variance_info()
    assert (info["captured"], info["resolved"], info["pixels_known_captured"], info["pixels_known_history"], info["pixels_known_blended"]) == (0, 0, 0, 0, 0)


def test_states_and_arguments():
    sc = gh.scene("small")
    objects = gh.table(sc)
    lib = abi.load()
    cam = gh.camera_of(sc, (0.02, 0.0, -0.03))
    V = sc.vertices.reshape(-1, 3, 3)
    mats = [abi.ErMaterial.from_buffer_copy(m) for m in sc.materials]
    rm = gh.history_manager(sc)
    plane = np.zeros(sc.y_res * sc.x_res * 4, f32)
    fp = plane.ctypes.data_as(C.POINTER(C.c_float))
    try:
        refused(rm, sc)                                                                      # begun, nothing captured
        rm.render(2)
        rm.variance_fold()
        rm.render(2)
        rm.variance_fold()
        rm.history_capture()
        info = rm.history_variance_info()
        assert (info["captured"], info["resolved"], info["pixels_known_captured"]) == (1, 0, sc.x_res * sc.y_res)
        assert lib.er_read_history_variance(rm.handle, fp) == STATE and lib.er_denoise_blended(rm.handle, C.byref(abi.ErDenoiseVariance(0, 0.0, 0.0, 0.0))) == STATE      # captured, not resolved
        rm.update(camera=cam)
        rm.history_resolve()
        rm.render(1)
        assert lib.er_denoise_blended(rm.handle, C.byref(abi.ErDenoiseVariance(0, 0.0, 0.0, 0.0))) == STATE      # no features of this scene state
        assert b"feature" in lib.er_last_error()
        rm.get_history_variance(), rm.get_blended_variance()
        rm.render_features()
        rm.denoise_blended()
        # arguments
        assert lib.er_denoise_blended(rm.handle, None) == INV and lib.er_read_history_variance(rm.handle, None) == INV and lib.er_read_blended_variance(rm.handle, None) == INV
        assert lib.er_history_variance_info(rm.handle, None) == INV
        assert lib.er_denoise_blended(rm.handle, C.byref(abi.ErDenoiseVariance(9, 0.0, 0.0, 0.0))) == INV
        for bad in ((-1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0), (float("nan"), 0.0, 0.0), (0.0, float("nan"), 0.0), (0.0, 0.0, float("nan"))):
            assert lib.er_denoise_blended(rm.handle, C.byref(abi.ErDenoiseVariance(0, *bad))) == INV, bad
        rm.denoise_blended(levels=8)

        def armed():
            rm.render(2)
            rm.variance_fold()
            rm.render(2)
            rm.variance_fold()
            rm.history_capture()
            rm.update(camera=cam)
            rm.history_resolve()
            rm.history_capture()                                 # (a capture of an unfolded frame that carries the history's variance on)
            info = rm.history_variance_info()
            assert info["captured"] == 1 and info["pixels_known_captured"] > 0

        # everything that drops a capture drops the carried planes
        drops = {
            "update": lambda: rm.update(vertices=V),
            "update_sparse": lambda: rm.update(tri_ids=np.array([3, 4], np.uint32), vertices=V[[3, 4]]),
            "edit geometry": lambda: rm.edit(vertices=V),
            "edit materials": lambda: rm.edit(materials=mats),
            "edit textures": lambda: rm.edit(textures=[None] * len(sc.textures)),
            "edit hdri": lambda: rm.edit(hdri=sc.hdri),
            "objects_set": lambda: rm.set_objects(objects),
            "topology": lambda: rm.topology(remove=np.array([sc.tri_count - 1], np.uint32)),
            "state_import": lambda: rm.state_import(rm.state_export()),
        }
        for what, call in drops.items():
            armed()
            call()
            refused(rm, sc)
            if what == "topology":                                                           # (back to the scene the other calls know)
                rm.start_rendering(sc)
                rm.set_objects(objects)
        armed()
        rm.start_rendering(sc)                                                               # er_render_begin
        refused(rm, sc)
    finally:
        rm.close()
    # a sharded frame
    rm = render.RenderingManager(render.RenderParameters(max_bounces=1, rank=0, world=2))
    rm.start_rendering(sc)
    try:
        assert lib.er_history_variance_info(rm.handle, C.byref(abi.ErHistoryVarianceInfo())) == STATE
        assert b"sharded" in lib.er_last_error()
        assert lib.er_read_history_variance(rm.handle, fp) == STATE and lib.er_read_blended_variance(rm.handle, fp) == STATE
        assert lib.er_denoise_blended(rm.handle, C.byref(abi.ErDenoiseVariance(0, 0.0, 0.0, 0.0))) == STATE
    finally:
        rm.close()


# ---- (6) ----

def test_the_denoised_blend_is_nearer_the_converged_frame_than_the_blend():
    """cornell_textured 96 x 96: 64 spp in folds of 2, capture, the history test's small camera move, resolve, 4 spp, features,
    er_denoise_blended.  Asserted: the mean absolute error against 1 024 spp of the new frame is below the unfiltered blend's.  Printed,
    not asserted: the ratio, and the same for er_denoise_guided of the plain 4 spp.  No margin is claimed."""
    sc = scenes.cornell_textured(96, 96)
    cam = gh.camera_of(sc, (0.02, 0.01, 0.0), (0.0, 1.0, 0.0))
    zero = np.zeros((96 * 96, 4), f32)
    mean = lambda: history.blend(rm.get_pass("beauty"), rm.read_samples(), zero).reshape(96, 96, 4)[..., :3].astype(np.float64)      # (without the setup sample)
    rm = render.RenderingManager(render.RenderParameters())
    rm.start_rendering(sc)
    try:
        rm.render(64, fold_every=2)
        assert rm.variance_info()["folds"] == 32
        rm.update(camera=cam, keep_history=True)
        rm.render(4)
        rm.render_features()
        rm.denoise_blended()
        denoised = rm.get_pass("denoise")[..., :3].astype(np.float64)
        info = rm.history_variance_info()
        blended = rm.get_blended()[..., :3].astype(np.float64)
        plain = mean()
        rm.denoise_guided()
        guided = rm.get_pass("denoise")[..., :3].astype(np.float64) * (5.0 / 4.0)
        rm.update(camera=cam)
        rm.render(1024)
        truth = mean()
    finally:
        rm.close()
    err = lambda a: float(np.abs(a - truth).mean())
    e_blend, e_den, e_plain, e_guided = err(blended), err(denoised), err(plain), err(guided)
    print(f"mean absolute error against 1024 spp: blend {e_blend:.5f}, er_denoise_blended {e_den:.5f} (x{e_den / e_blend:.3f} of the blend), plain 4 spp {e_plain:.5f}, "
          f"er_denoise_guided of it {e_guided:.5f} (x{e_guided / e_plain:.3f} of the plain; denoised blend / guided {e_den / e_guided:.3f}); {info}")
    assert info["resolved"] == 1 and info["pixels_known_blended"] > 0.5 * 96 * 96
    assert e_den < e_blend
