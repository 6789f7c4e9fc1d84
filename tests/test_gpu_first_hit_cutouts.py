"""The first-hit pass that sees through cut-outs (er_first_hit_set) on the GPU, against the numpy replay of
tests/cutout_scenes.py, every word compared and no pixel excluded.

(1) mode on, both builders, 1 and 4 rays: albedo, depth, the six id planes, the history across a camera move (its key planes), er_pick
along two rows and the five counters; (2) er_debug_first_hit_rays through every stack, and over a real tree; (3) mode off after on, and
a scene never set: today's planes, counters 0; (4) the render is the same with and without the mode; (5) what a set invalidates; (6) two
ranks on one GPU; (7) the host session."""
import ctypes as C
import functools

import numpy as np
import pytest

import cutout_scenes as cs
import mesh_light_scenes
from elevenrender_amd import abi, client, history, ids, render
from test_gpu_features import planes_numpy, scene as feature_scene
from test_gpu_update import assert_same_outputs, outputs
from test_host_server import Server, session_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
BUILDERS = {"host": abi.FLAG_HOST_BUILD, "device": abi.FLAG_GPU_BUILD}
SCHEDULES = {"stream": abi.FLAG_STREAM, "wavefront": abi.FLAG_WAVEFRONT, "megakernel": abi.FLAG_MEGAKERNEL}
KINDS = ("triangle", "object", "material")
COUNTERS = ("rays", "rays_through", "layers_skipped", "rays_capped", "rays_through_to_miss")
bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)


def differing(a, b):
    return int((bits(a) != bits(b)).any(-1).sum())


def manager(sc, flags=0, objects=True, cutouts=None, **kw):
    rm = render.RenderingManager(render.RenderParameters(max_bounces=cs.MAX_BOUNCES, flags=flags, **kw))
    rm.start_rendering(sc)
    if objects:
        rm.set_objects(cs.table(sc))
    if cutouts is not None:
        rm.set_first_hit(cutouts)
    return rm


def counts_of(rm):
    info = rm.first_hit_info()
    return {k: info[k] for k in COUNTERS}


def moved_camera(sc):
    cam = abi.ErCamera.from_buffer_copy(sc.camera)
    cam.position = abi.ErVec3(sc.camera.position.x + 0.12, sc.camera.position.y - 0.07, sc.camera.position.z - 0.15)
    cam.rotation = abi.ErVec3(1.0, -2.0, 0.5)
    return cam


@functools.lru_cache(maxsize=None)
def want_ids(n, kind, cutouts=True):
    sc = cs.layers()
    tri = cs.take(cs.pass_replay(4, cutouts=cutouts), n)["tri"].reshape(-1, n)
    t = np.maximum(tri, 0)
    k = {"triangle": t.astype(np.uint32), "object": ids.object_of(sc.tri_count, cs.table(sc))[t], "material": sc.material_id.astype(np.uint32)[t]}[kind]
    i, c, over = ids.planes(k, tri >= 0)
    return i.reshape(sc.y_res, sc.x_res, 4), c.reshape(sc.y_res, sc.x_res, 4), over


@functools.lru_cache(maxsize=None)
def keys(cutouts=True):
    """the key planes before and after the camera move, with their replays"""
    sc = cs.layers()
    of = ids.object_of(sc.tri_count, cs.table(sc))
    return cs.key_plane(sc, of, cutouts=cutouts), cs.key_plane(sc, of, camera=moved_camera(sc), cutouts=cutouts)


def assert_feature_and_id_planes(rm, n, cutouts=True, what=""):
    sc = cs.layers()
    v = cs.pass_replay(4, cutouts=cutouts)
    rm.render_features(n)
    want_a, want_d = cs.planes(sc, v, n)
    da, dd = differing(rm.get_feature("albedo"), want_a), differing(rm.get_feature("depth"), want_d)
    print(what, "n", n, "albedo pixels differing", da, "depth", dd)
    assert da == 0 and dd == 0, (what, n, da, dd)
    if cutouts:
        assert counts_of(rm) == cs.counters(cs.take(v, n)), (what, n, "features")
    rm.render_ids(n)
    for kind in KINDS:
        gi, gc = rm.get_ids(kind)
        wi, wc, over = want_ids(n, kind, cutouts)
        assert (gi == wi).all() and (gc == wc).all(), (what, n, kind, int((gi != wi).any(-1).sum()), int((gc != wc).any(-1).sum()))
        assert rm.id_info()["overflow_pixels"][KINDS.index(kind)] == over
    if cutouts:
        assert counts_of(rm) == cs.counters(cs.take(v, n)), (what, n, "ids")


# ---- (1) ----

@pytest.mark.parametrize("builder", list(BUILDERS))
def test_every_consumer_equals_the_replay_with_the_mode_on(builder):
    sc = cs.layers()
    npx = sc.x_res * sc.y_res
    v = cs.pass_replay(4)
    rm = manager(sc, BUILDERS[builder])
    try:
        assert rm.accel_info()["builder"] == (1 if builder == "device" else 0)
        assert rm.first_hit_info() == dict(cutouts=0, opacity_threshold=0.5, rays=0, rays_through=0, layers_skipped=0, rays_capped=0, rays_through_to_miss=0)
        rm.set_first_hit(True)
        info = rm.first_hit_info()
        assert (info["cutouts"], info["opacity_threshold"]) == (1, 0.5) and all(info[k] == 0 for k in COUNTERS)
        for n in (1, 4):
            assert_feature_and_id_planes(rm, n, what=builder)
        # the mode changes every plane on this scene
        off_a, _ = cs.planes(sc, cs.pass_replay(4, cutouts=False), 4)
        assert differing(rm.get_feature("albedo"), off_a) > 200
        # er_pick: ray 0 of every pixel of two rows, through both rows of cards
        r0 = cs.take(v, 1)
        of = ids.object_of(sc.tri_count, cs.table(sc))
        seen = set()
        for y in (7, 21):
            for x in range(sc.x_res):
                i = y * sc.x_res + x
                p = rm.pick(x, y)
                t = int(r0["tri"][i])
                if t < 0:
                    assert (p["hit"], p["triangle"], p["object"], p["material"]) == (0, abi.ID_NONE, abi.ID_NONE, abi.ID_NONE), (x, y, p)
                    assert p["distance"] == 0 and (p["position"] == 0).all() and (p["uv"] == 0).all()
                else:
                    assert (p["hit"], p["triangle"], p["object"], p["material"]) == (1, t, int(of[t]), int(sc.material_id[t])), (x, y, p, t)
                    assert (bits(p["distance"]) == bits(r0["dist"][i])).all() and (bits(p["position"]) == bits(r0["rec"][i, 0:3])).all(), (x, y)
                    assert (bits(p["uv"]) == bits(r0["rec"][i, 15:17])).all(), (x, y)
                seen.add((t >= 0, int(r0["layers"][i]), bool(r0["capped"][i]), bool(r0["to_miss"][i])))
        assert {(True, 0, False, False), (True, 1, False, False), (True, 3, False, False), (False, 0, False, False), (False, cs.MAX_BOUNCES, True, False),
                (False, 1, False, True)} <= seen, seen
        assert counts_of(rm) == cs.counters(cs.take(v, 4))          # a pick counts nothing: still the id pass's
        # the key plane, through the history: a capture, a camera move, a resolve -- against history.py fed the replayed keys
        rm.render(2)
        beauty, samples = rm.get_pass("beauty"), rm.read_samples()
        rm.history_capture()
        (old, old_v), (new, new_v) = keys()
        assert counts_of(rm) == cs.counters(old_v)
        rm.update(camera=moved_camera(sc))
        rm.history_resolve()
        got = rm.get_history()
        cw = history.capture(beauty, samples, None, 32.0)
        zeros12, zeros = np.zeros((npx, 12), f32), np.zeros(npx, np.uint32)
        want, state, cls = history.resolve(abi.debug_history_camera(sc.camera), sc.x_res, sc.y_res, f32(0.02), new["hit"], new["obj"], new["P"], zeros, zeros12,
                                           old["hit"], old["obj"], old["dist"], cw)
        bad = differing(got.reshape(-1, 4), want)
        print(builder, "history pixels differing", bad, history.class_counts(cls))
        assert bad == 0, bad
        hi = rm.history_info()
        assert {k: hi["pixels_" + k] for k in history.CLASS_NAMES} == history.class_counts(cls)
        assert counts_of(rm) == cs.counters(new_v)
        # under the other rule the same capture resolves differently: the keys matter
        (old0, _), (new0, _) = keys(False)
        other, _, _ = history.resolve(abi.debug_history_camera(sc.camera), sc.x_res, sc.y_res, f32(0.02), new0["hit"], new0["obj"], new0["P"], zeros, zeros12,
                                      old0["hit"], old0["obj"], old0["dist"], cw)
        assert differing(other, want) > 50
    finally:
        rm.close()


# ---- (2) ----

def assert_rays(rm, sc, o, d, max_hits, threshold=0.0):
    tri, layers, dist, pos = rm.debug_first_hit_rays(o, d, threshold)
    v = cs.visible(sc, o, d, threshold, max_hits)
    assert (tri == v["tri"]).all(), int((tri != v["tri"]).sum())
    assert (layers == v["layers"]).all()
    hit = tri >= 0
    assert (bits(pos[hit]) == bits(v["rec"][hit, 0:3])).all() and (pos[~hit] == 0).all()
    assert (bits(dist) == bits(v["dist"])).all()
    return v


def test_rays_through_every_stack_equal_the_replay():
    sc = cs.layers()
    rm = manager(sc)                                                               # (the hook runs the walk whatever the scene's mode)
    try:
        names, o, d = cs.stack_rays(sc)
        v = assert_rays(rm, sc, o, d, cs.MAX_BOUNCES)
        got = {k: (int(sc.material_id[t]) if t >= 0 else -1, int(l)) for k, t, l in zip(names, v["tri"], v["layers"])}
        assert got == {"A": (cs.M_WALL, 3), "B": got["B"], "F": (cs.M_F, 0), "E": (cs.M_E_FRONT, 0), "D": (-1, cs.MAX_BOUNCES), "G": (cs.M_WALL, 1), "C": (-1, 1)}, got
        # a threshold of 0.25 stops every 0.3 card; one of 1 passes the 0.5 card too
        low = assert_rays(rm, sc, o, d, cs.MAX_BOUNCES, 0.25)
        assert (low["layers"][[names.index(k) for k in ("A", "G", "C")]] == 0).all()
        high = assert_rays(rm, sc, o, d, cs.MAX_BOUNCES, 1.0)
        assert high["layers"][names.index("F")] == 1
        # 65 and 129 rays: a second and a third workgroup, partial ones
        for n in (65, 129):
            oo, dd = cs.pass_replay(4)["origins"][:n], cs.pass_replay(4)["dirs"][:n]
            assert_rays(rm, sc, oo, dd, cs.MAX_BOUNCES)
    finally:
        rm.close()


def test_rays_over_a_real_tree_equal_the_replay():
    """mesh_light_scenes.lit_soup: 3 000 triangles, 6 of 16 of them cut-outs of 0.3, textured and half opacities between them"""
    sc = mesh_light_scenes.lit_soup()
    o, d = cs.camera_rays(sc, 1)
    rm = render.RenderingManager(render.RenderParameters(max_bounces=mesh_light_scenes.LIT_MAX_BOUNCES))
    rm.start_rendering(sc)
    try:
        v = assert_rays(rm, sc, o.reshape(-1, 3), d.reshape(-1, 3), mesh_light_scenes.LIT_MAX_BOUNCES)
        c = cs.counters(v)
        print(c)
        assert c["rays_through"] > 300 and (v["layers"] >= 3).sum() > 20 and c["rays_through_to_miss"] > 5
    finally:
        rm.close()


# ---- (3) ----

def test_mode_off_after_on_and_a_scene_never_set_give_todays_planes():
    sc = cs.layers()
    for was_on in (True, False):
        rm = manager(sc)
        try:
            if was_on:
                rm.set_first_hit(True)
                rm.render_features(4)
                rm.render_ids(4)
                assert rm.first_hit_info()["rays"] > 0
                rm.set_first_hit(False)
            assert_feature_and_id_planes(rm, 4, cutouts=False, what=f"off, was on {was_on}")
            info = rm.first_hit_info()
            assert info["cutouts"] == 0 and all(info[k] == 0 for k in COUNTERS)
        finally:
            rm.close()
    # ... and on the feature test's own scene against its own replay
    name = "torture-600"
    fs = feature_scene(name)
    rm = render.RenderingManager(render.RenderParameters(max_bounces=1))
    rm.start_rendering(fs)
    try:
        rm.set_first_hit(True)
        rm.render_features(4)
        rm.set_first_hit(False)
        rm.render_features(4)
        want_a, want_d, _ = planes_numpy(name, 4)
        assert differing(rm.get_feature("albedo"), want_a) == 0 and differing(rm.get_feature("depth"), want_d) == 0
    finally:
        rm.close()


# ---- (4) ----

@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_the_render_is_the_same_with_and_without_the_mode(sched):
    sc = cs.layers()
    got = []
    for with_mode in (True, False):
        rm = manager(sc, SCHEDULES[sched])
        if with_mode:
            rm.set_first_hit(True)
            rm.render_features(4)
            rm.render_ids(2)
        rm.render(4)
        if with_mode:
            rm.render_features(2)
            rm.pick(3, 9)
            rm.history_capture()
        got.append((outputs(rm), rm.counters(), rm.get_render_info().samples))
        rm.close()
    assert_same_outputs(got[0][0], got[1][0], sched)
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2] == 5


# ---- (5) ----

def test_a_set_that_changes_something_invalidates_and_one_that_does_not_does_not():
    sc = cs.layers()
    rm = manager(sc)
    valid = lambda: (rm.feature_info()["valid"], rm.id_info()["valid"], rm.history_info()["captured"])

    def fill():
        rm.render_features(1)
        rm.render_ids(1)
        rm.history_capture()
        assert valid() == (1, 1, 1)

    try:
        rm.render(1)
        fill()
        rm.set_first_hit(False)                                                    # off -> off, whatever the threshold's spelling
        rm.set_first_hit(False, 0.5)
        assert valid() == (1, 1, 1)
        rm.set_first_hit(True)                                                     # the mode changes
        assert valid() == (0, 0, 0)
        assert abi.load().er_history_resolve(rm.handle) == abi.ER_ERR_STATE         # the capture is gone
        fill()
        before = counts_of(rm)
        rm.set_first_hit(True, 0.0)                                                # the same values: 0 is 0.5
        rm.set_first_hit(True, 0.5)
        assert valid() == (1, 1, 1) and counts_of(rm) == before
        rm.set_first_hit(True, 0.25)                                               # the threshold changes
        assert valid() == (0, 0, 0) and rm.first_hit_info()["opacity_threshold"] == 0.25 and counts_of(rm)["rays"] == 0
        fill()
        with pytest.raises(abi.ErError):
            rm.set_first_hit(True, float("nan"))                                   # a refusal leaves the scene untouched
        assert valid() == (1, 1, 1) and rm.first_hit_info()["opacity_threshold"] == 0.25
        # the setting survives a second er_render_begin and an update
        p = abi.ErRenderParams(rm.pars.sampleTarget, rm.pars.block_size, 2, 0, 0, 1, 0)
        abi.check(rm.lib.er_render_begin(rm.handle, C.byref(p)))
        info = rm.first_hit_info()
        assert (info["cutouts"], info["opacity_threshold"]) == (1, 0.25) and all(info[k] == 0 for k in COUNTERS) and valid() == (0, 0, 0)
        rm.render_features(1)                                                      # ... with max_bounces 2 now: a ray examines two hits
        after = counts_of(rm)
        want = cs.counters(cs.visible(sc, *cs.camera_rays(sc, 1), threshold=0.25, max_hits=2))
        assert after == want and after["rays_capped"] > 0 and after["layers_skipped"] < before["layers_skipped"]
        rm.update(camera=moved_camera(sc))
        info = rm.first_hit_info()
        assert (info["cutouts"], info["opacity_threshold"]) == (1, 0.25) and rm.feature_info()["valid"] == 0
    finally:
        rm.close()


# ---- (6) ----

def test_two_ranks_on_one_gpu_gathered_equal_the_one_rank_planes():
    lib = abi.load()
    sc = cs.layers()
    world, root = 2, 0
    comms = (C.c_void_p * world)()
    abi.check(lib.er_comm_create_local(world, comms))
    rms = [manager(sc, cutouts=True, rank=r, world=world) for r in range(world)]
    try:
        for rm in rms:
            rm.render_features(4)
        per_rank = [counts_of(rm) for rm in rms]
        want = cs.counters(cs.pass_replay(4))
        assert all(c["rays"] > 0 for c in per_rank) and {k: sum(c[k] for c in per_rank) for k in COUNTERS} == want          # each rank counts its own rays
        for rm in rms:
            rm.render_ids(4)
        for f in (abi.FEATURE_ALBEDO, abi.FEATURE_DEPTH):
            for r in (1, 0):
                abi.check(lib.er_gather_feature(rms[r].handle, f, comms[r], root))
        for kind in range(abi.ID_KIND_COUNT):
            for r in (1, 0):
                abi.check(lib.er_gather_ids(rms[r].handle, kind, comms[r], root))
        want_a, want_d = cs.planes(sc, cs.pass_replay(4), 4)
        assert differing(rms[root].get_feature("albedo"), want_a) == 0 and differing(rms[root].get_feature("depth"), want_d) == 0
        for kind in KINDS:
            gi, gc = rms[root].get_ids(kind)
            wi, wc, _ = want_ids(4, kind)
            assert (gi == wi).all() and (gc == wc).all(), kind
    finally:
        for rm in rms:
            rm.close()
        for c in comms:
            lib.er_comm_destroy(c)


# ---- what the mode buys the guided denoise ----

def test_guided_denoise_is_nearer_the_converged_frame_with_the_mode_on():
    """scenes.cornell_cards(192, 192): a card of binary opacity in front of the textured back wall.  Mean absolute error of
    er_denoise_guided (defaults) against 1 024 spp, images scaled by (n + 1) / n as tests/test_gpu_features.py does.  Measured
    (tools/first_hit_bench.py, profiles/first_hit_cutouts.log): 4 spp 0.02042 with the mode on against 0.02351 with it off (0.87),
    16 spp 0.01829 against 0.02063 (0.89).  Asserted: on < off at both."""
    from elevenrender_amd import scenes
    sc = scenes.cornell_cards(192, 192)
    out, ref = {}, None
    for on in (True, False):
        rm = render.RenderingManager(render.RenderParameters(max_bounces=5))
        rm.start_rendering(sc)
        rm.set_first_hit(on)
        rm.render_features()
        done = 0
        for n in (4, 16):
            rm.render(n - done)
            done = n
            rm.denoise_guided()
            out[on, n] = rm.get_pass("denoise")[..., :3] * f32((n + 1) / n)
        if ref is None:
            assert rm.first_hit_info()["rays_through"] > 1000
            rm.render(1024 - done)
            ref = rm.get_pass("beauty")[..., :3] * f32(1025 / 1024)
        rm.close()
    for n in (4, 16):
        e_on, e_off = float(np.abs(out[True, n] - ref).mean()), float(np.abs(out[False, n] - ref).mean())
        print(f"{n} spp: mean abs error vs 1024 spp, guided denoise, mode on {e_on:.5f}, mode off {e_off:.5f}")
        assert e_on < e_off, (n, e_on, e_off)


# ---- (7) ----

def test_host_session_with_cutouts_serves_the_direct_planes(tmp_path):
    """the Cornell session with its red wall made a cut-out of opacity 0.3: with "cutouts": true the albedo plane shows what lies behind it"""
    a = client.cornell_session_assets(100, 76)                                      # partial tiles on both edges
    a["materials"][1] = dict(a["materials"][1], opacity=0.3)
    sc = session_scene(a, tmp_path)
    assert sc.materials[2].albedo.x == f32(0.8)
    sc.materials[2].opacity = 0.3
    sc._desc = None
    direct = {}
    for on in (True, False):
        rm = render.RenderingManager(render.RenderParameters())
        rm.start_rendering(sc)
        if on:
            rm.set_first_hit(True)
        rm.render_features(2)
        direct[on] = (rm.get_feature("albedo"), rm.get_feature("depth"), rm.first_hit_info())
        rm.close()
    assert differing(direct[True][0], direct[False][0]) > 100 and direct[True][2]["rays_through"] > 100
    for gpus in (1, 3):
        s = Server()
        c = client.Client(port=s.port)
        extra = dict(gpus=3, devices=[0, 0, 0], transport="local") if gpus == 3 else {}
        client.play_cornell_session(c, a, sample_target=3, cutouts=True, feature_samples=2, **extra)
        albedo, depth = c.get_pass("albedo", 100, 76), c.get_pass("depth", 100, 76)
        info = c.get_info()
        c.close()
        assert s.finish() == 0
        assert differing(albedo, direct[True][0]) == 0 and differing(depth, direct[True][1]) == 0, gpus
        assert info["cutouts"] is True and info["cutout_threshold"] == 0.5
        assert {k: info["cutout_" + k] for k in COUNTERS} == {k: direct[True][2][k] for k in COUNTERS}, (gpus, info)
    # a session without the key answers as before
    s = Server()
    c = client.Client(port=s.port)
    client.play_cornell_session(c, a, sample_target=3, feature_samples=2)
    albedo = c.get_pass("albedo", 100, 76)
    info = c.get_info()
    c.close()
    assert s.finish() == 0
    assert differing(albedo, direct[False][0]) == 0 and not any(k.startswith("cutout") for k in info)
