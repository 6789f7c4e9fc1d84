"""Every wide traversal beyond the stack levels it keeps in LDS, against the oracle.

The first WF_LDS_STACK (8) entries of a lane's traversal stack live in LDS, the deeper ones in an HBM spill area (csrc/er_trav.h,
trav_choose) whose per-wave base each kernel computes for itself: er_wf_trace (csrc/er_wavefront.hip), the streaming tracer waves and
their counting instances (csrc/er_stream.hip), the first-hit walker behind features, ids, pick and history keys (csrc/er_first_hit.h,
csrc/er_ids.hip) and the debug hooks (csrc/er_debug.hip).  Ordinary scenes never leave the LDS levels; the self-similar scene of
tests/deep_tree_scenes.py does on nearly every camera ray (tests/test_deep_tree_scenes_cpu.py proves it without a GPU), at 648
triangles, so every comparison here is bit for bit with the oracle and takes seconds.

Which test covers which base computation (a lane, wave or workgroup term off by one makes lanes or waves share stack entries; the test
runs that kernel with many spilling waves at once, and a shared entry sends a ray down another ray's subtree):
  er_wavefront.hip `W.spill + blockIdx.x * (ER_STACK8 * 64) + lane`    test_images_equal_the_oracle[*-wavefront-*], 160 x 120
  er_stream.hip    `W.spill + (blockIdx.x * 16 + wave) * ER_SPILL_PER_WAVE + lane`, the tracer waves
                                                                        test_images_equal_the_oracle[*-stream-*] and [*-auto-*], 160 x 120
  er_stream.hip    the 32-bit re-formed pointer of the COUNT instances  test_images_equal_the_oracle[*-stream+counters-*], 160 x 120
  er_first_hit.h / er_ids.hip  `spill_base + blockIdx.x * ER_FIRST_HIT_SPILL_PER_BLOCK + lane`
                                                                        test_first_hit_passes_equal_their_replays (features, keys, pick / ids)
  er_debug.hip     er_debug_trace_kernel `spill_base + blockIdx.x * (ER_STACK8 * 64) + threadIdx.x`
                                                                        test_rays_through_the_spill_levels (322 blocks; the hook reads the area back)
  er_debug.hip     er_debug_pixel_kernel, the exact routine's stack behind the spill levels
                                                                        test_pixel_trace_through_the_spill_levels

What these tests cannot see: each region holds ER_STACK8 = 32 levels and the deepest rays here use 6 of them (the builders pad every box
by 1e-6 of the scene's extent, which ends the chain: no scene of a few hundred triangles gets much deeper than 15 wide levels), so a
region stride wrong by fewer than the unused levels moves no entry onto another wave's.  A wrong lane, wave or workgroup term does.

Measured on an MI355X: test_rays_through_the_spill_levels; the whole file takes 8.5 s, its slowest test 2.8 s."""
import functools

import numpy as np
import pytest

import accel_check
import deep_tree_scenes as dts
from elevenrender_amd import abi, history, ids, render, scenes
from test_gpu_function_level import _rec_tuple
from test_gpu_update import with_arrays

pytestmark = pytest.mark.gpu
f32 = np.float32
bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)
BUILDERS = {"host": abi.FLAG_HOST_BUILD, "device": abi.FLAG_GPU_BUILD}
SCHEDULES = {"wavefront": abi.FLAG_WAVEFRONT, "stream": abi.FLAG_STREAM, "stream+counters": abi.FLAG_STREAM | abi.FLAG_COUNTERS, "auto": 0,
             "megakernel": abi.FLAG_MEGAKERNEL}      # (the megakernel never touches the spill area: the control)
PLANES = ("beauty", "denoise", "normal", "tangent", "bitangent")
LDS, STACK8 = dts.WF_LDS_STACK, dts.ER_STACK8
SPP, MAX_BOUNCES = 4, 8
SMALL, LARGE = (24, 16), (160, 120)


@functools.lru_cache(maxsize=None)
def scene(name, frame):
    sc = dts.nested_shells(*frame)
    return {"shells": lambda s: s, "scaled": dts.scaled, "posed": dts.posed}[name](sc)


@functools.lru_cache(maxsize=None)
def centre_rays(frame):
    return dts.pixel_centre_rays(scene("shells", frame))


@functools.lru_cache(maxsize=None)
def oracle_frame(name, frame, spp=SPP):
    """the oracle's planes, sample counts, RNG and counters of a description: computed once, shared, never changed"""
    import oracle as orc
    o = orc.Oracle(scene(name, frame), math_mode=orc.MATH_ER, max_bounces=MAX_BOUNCES, threads=8)
    o.render(spp)
    out = {n: o.read_pass(p) for n, p in abi.PASS_NAMES.items()}
    out["samples"], out["rng"], out["counters"] = o.read_samples(), o.read_rng(), o.counters()
    o.close()
    return out


def manager(sc, flags=0, rank=0, world=1, max_bounces=MAX_BOUNCES):
    rm = render.RenderingManager(render.RenderParameters(max_bounces=max_bounces, flags=flags, rank=rank, world=world))
    rm.start_rendering(sc)
    return rm


def outputs(rm):
    out = {p: rm.get_pass(p) for p in PLANES}
    out["samples"], out["rng"], out["counters"] = rm.read_samples(), rm.read_rng(), rm.counters()
    return out


def assert_bit_equal(g, o, what, mask=None):
    shape = g["beauty"].shape[:2]
    m = np.ones(shape, bool) if mask is None else mask
    for p in PLANES:
        bad = (bits(g[p]) != bits(o[p])).any(-1) & m
        assert not bad.any(), f"{what}: {p} differs in {int(bad.sum())} pixels, first {np.argwhere(bad)[:3].tolist()}"
    for k in ("samples", "rng"):
        bad = (g[k].reshape(shape) != o[k].reshape(shape)) & m
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} pixels"
    if mask is None:
        assert g["counters"]["bounce_samples"] == o["counters"]["bounce_samples"], what
        assert g["counters"]["paths"] == o["counters"]["paths"], what


def assert_deep(sc, rm, builder, what, frame=SMALL):
    """the conditions of tests/test_deep_tree_scenes_cpu.py on the tree as it lies in device memory, whichever builder made it"""
    d, info = rm.debug_read_accel(), rm.accel_info()
    rep = accel_check.check(sc, d, accel_depth=info["max_depth"])
    assert rep.ok, f"{what}: {rep.message()}"
    o, dr = centre_rays(frame)
    entries, marginal = dts.first_descent_entries(d, o, dr)
    keep = ~marginal
    print(f"{what} ({builder} builder): wide depth {d['max_depth8']}, binary depth {d['max_depth']}, marginal {marginal.mean():.4f}, "
          f"first-descent entries {dts.distribution(entries, keep)}")
    assert LDS + 6 <= d["max_depth8"] <= STACK8, what
    assert marginal.mean() <= 0.02 and (entries[keep] >= LDS + 4).mean() >= 0.5 and entries[keep].max() >= LDS + 6, what
    return d, entries, marginal


# ---- function level ----

def probe_rays(sc, hit_pos):
    """origins, dirs and what they are: the pixel-centre rays of both frames, rays leaving the hit points, axis-parallel rays, rays from
    outside the scene towards the origin"""
    rnd = scenes.Rand(77, 3)
    co, cd = centre_rays(LARGE)
    so, sd = centre_rays(SMALL)
    nd = rnd.uniform(-1, 1, len(hit_pos), 3)
    nd = (nd / np.maximum(np.linalg.norm(nd, axis=1, keepdims=True), 1e-6)).astype(f32)
    lo = (hit_pos + nd * f32(0.001)).astype(f32)
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(f32)
    cam = np.array([sc.camera.position.x, sc.camera.position.y, sc.camera.position.z], f32)
    ad = np.tile(axes, (41, 1))
    ao = (np.concatenate([np.tile(cam, (6, 1)), np.repeat(hit_pos[:40], 6, 0)]) + ad * f32(0.001)).astype(f32)      # (off the surface, as the kernels' rays)
    oo = rnd.uniform(-1, 1, 500, 3)
    oo = (10.0 * oo / np.maximum(np.linalg.norm(oo, axis=1, keepdims=True), 1e-6)).astype(f32)
    od = (-oo / np.linalg.norm(oo, axis=1, keepdims=True)).astype(f32)
    parts = [("camera 160 x 120", co, cd), ("camera 24 x 16", so, sd), ("leaving hit points", lo, nd), ("axis-parallel", ao, ad), ("towards the origin", oo, od)]
    kind = np.concatenate([np.full(len(o), i) for i, (_, o, _) in enumerate(parts)])
    return np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), kind, [p[0] for p in parts]


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_rays_through_the_spill_levels(oracle_mod, builder):
    """er_debug_trace_rays_levels: closest hits bit for bit with the oracle's throwRay, the spill levels each ray wrote at least what the
    replay of its first descent says, shadow verdicts as the oracle's closest hits imply.

    Measured on an MI355X, the same under either builder (both trees: binary depth 20, wide depth 15).  Spill levels {levels: rays} of the
    19 200 camera rays of the 160 x 120 frame: {2: 71, 3: 94, 4: 128, 5: 499, 6: 18 408}, the replay's entries minus 8 on all but a
    hundred marginal rays ({10: 70, 11: 93, 12: 127, 13: 494, 14: 18 305}); of the 24 x 16 frame {2: 1, 3: 2, 4: 1, 5: 8, 6: 372}; of the 500
    rays towards the origin {0: 449, 1: 2, 2: 3, 3: 3, 4: 2, 5: 3, 6: 38}; the rays leaving hit points and the axis-parallel ones stay
    within the LDS levels.  Shadow queries prune the groups beyond their limit before they are pushed, exactly as the replay with that
    limit says on the four fifths of the camera rays it does not call marginal ({10: 5 203, 11: 1 238, 12: 601, 13: 988, 14: 7 388}): leaving the hit triangle
    {2: 9 066, 3: 1 468, 4: 605, 5: 995, 6: 7 450}, 1 % beyond the hit (11 735 occluded) {0: 507, 2: 8 799, 3: 1 324, 4: 568, 5: 955, 6: 7 431}."""
    sc = scene("shells", SMALL)
    orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, max_bounces=MAX_BOUNCES, threads=8)
    rm = manager(sc, BUILDERS[builder])
    try:
        assert rm.accel_info()["builder"] == (1 if builder == "device" else 0)
        d, _, _ = assert_deep(sc, rm, builder, "function level")
        ht, hp = orc.closest_hit(*centre_rays(SMALL))
        o, dr, kind, names = probe_rays(sc, hp[ht >= 0])
        assert len(o) % 64 != 0 and len(o) > 300 * 64                                 # many blocks and a partial last one
        tri, slot, pos, dist, info, lv = rm.debug_trace_rays(o, dr, levels=True)
        assert (lv["lds_levels"], lv["stack_levels"]) == (LDS, STACK8)                 # what the tests state is what was compiled
        spill = lv["spill_levels"].astype(np.int64)
        otri, opos = orc.closest_hit(o, dr)
        bad = (bits(pos) != bits(opos)).any(-1) | (tri != otri)
        assert not bad.any(), f"{int(bad.sum())} rays differ from the oracle, first {np.nonzero(bad)[0][:5].tolist()} of kinds {kind[bad][:5].tolist()}"
        entries, marginal = dts.first_descent_entries(d, o, dr)
        for i, name in enumerate(names):
            k = kind == i
            print(f"{builder} builder, {name}: {int(k.sum())} rays, {int((tri[k] >= 0).sum())} hit, spill levels {{levels: rays}} {dts.distribution(spill, k)}, "
                  f"replay entries {dts.distribution(entries, k & ~marginal)}")
        short = ~marginal & (spill + LDS < entries)
        assert not short.any(), f"{int(short.sum())} rays wrote fewer spill levels than their first descent leaves, first {np.nonzero(short)[0][:5].tolist()}"
        cam = kind <= 1
        assert (spill[cam] >= 4).mean() >= 0.5
        assert spill.max() < d["max_depth8"] - LDS
        # shadow queries whose verdict the oracle's closest hits imply.  (a) the camera ray again, leaving out the triangle it hits, up to
        # that hit: nothing else is nearer; (b) no triangle left out, up to 1 % beyond the hit: occluded, 1 % short of it: not;
        # (c) a ray that misses, with no limit to speak of: not occluded
        hit = tri >= 0
        odist = np.sqrt(((opos - o).astype(np.float64) ** 2).sum(-1)).astype(f32)
        n = len(o)
        clear = ~hit | (odist > f32(1e-3))            # (1 % of a hit at the ray's own origin is no margin)
        assert clear.mean() > 0.99
        cases = [("leaving the hit triangle", np.where(hit, slot, -1).astype(np.int32), np.where(hit, dist, f32(1e30)).astype(f32), np.zeros(n, bool)),
                 ("1 % beyond the hit", np.full(n, -1, np.int32), np.where(hit, odist * f32(1.01), f32(1e30)).astype(f32), hit),
                 ("1 % short of the hit", np.full(n, -1, np.int32), np.where(hit, odist * f32(0.99), f32(1e30)).astype(f32), np.zeros(n, bool))]
        for what, self_slots, limits, want in cases:
            occ, sinfo, slv = rm.debug_trace_rays(o, dr, self_slots=self_slots, limits=limits, levels=True)
            wrong = (occ != want) & clear
            assert not wrong.any(), f"shadow queries {what}: {int(wrong.sum())} verdicts differ, first {np.nonzero(wrong)[0][:5].tolist()}"
            s = slv["spill_levels"].astype(np.int64)
            print(f"{builder} builder, shadow queries {what}: {int(occ.sum())} occluded, camera rays' spill levels {dts.distribution(s, cam)}")
            # a query without a limit that finds nothing is the closest-hit query step for step
            assert (s[~hit] == spill[~hit]).all(), what
            if what == "1 % beyond the hit":
                # a query that an occluder may end has no bound of this kind: its triangles are tested on the way down, and a replay
                # that stops at the first node with a hit leaf slot keeps 8 entries or fewer on every camera ray
                continue
            # a query that finds no occluder runs its first descent to the end, pruning only what lies beyond its limit: the replay
            # with that limit is a lower bound ray by ray, and by it at least half of the camera rays write 2 levels or more
            lentries, lmarginal = dts.first_descent_entries(d, o, dr, limits=limits)
            print(f"   replay with the limit: marginal {lmarginal[cam].mean():.3f} of the camera rays, entries {dts.distribution(lentries, cam & ~lmarginal)}")
            short = ~lmarginal & (s + LDS < lentries)
            assert not short.any(), f"shadow queries {what}: {int(short.sum())} rays wrote fewer spill levels than their limited first descent leaves"
            assert (lentries[cam & ~lmarginal] >= LDS + 2).sum() >= 0.5 * cam.sum(), what
            assert (s[cam] >= 2).mean() >= 0.5, what
    finally:
        rm.close()
        orc.close()


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_pixel_trace_through_the_spill_levels(oracle_mod, builder):
    """er_debug_trace_pixel, whose scratch holds the spill levels and, behind them, the exact routine's stack: record by record against
    the oracle's trace, on pixels whose centre ray leaves 12 entries or more"""
    sc = scene("shells", SMALL)
    orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, max_bounces=MAX_BOUNCES, threads=1)
    rm = manager(sc, BUILDERS[builder])
    try:
        entries, marginal = dts.first_descent_entries(rm.debug_read_accel(), *centre_rays(SMALL))
        deep = np.nonzero((entries >= LDS + 4) & ~marginal)[0]
        assert len(deep) >= 100
        rm.render(2)
        orc.render(2)
        n_rec = n_long = 0
        for idx in deep[:: len(deep) // 24][:24]:
            for _ in range(2):
                g, o = rm.debug_trace_pixel(int(idx), max_recs=16), orc.trace_pixel(int(idx), max_recs=16)
                assert len(g) == len(o), (int(idx), len(g), len(o))
                n_long += len(g) > 2
                for a, b in zip(g, o):
                    n_rec += 1
                    traced = a.shadow_occ >= 0
                    assert _rec_tuple(a, traced) == _rec_tuple(b, traced), (int(idx), a.bounce)
        print(f"{builder} builder: {n_rec} bounce records equal, {n_long} of 48 samples ran more than two iterations")
        assert n_long >= 5
        same = (bits(rm.get_pass("beauty")) == bits(orc.read_pass(0))).all() and (rm.read_samples() == orc.read_samples()).all()
        assert same, "the traced samples did not advance the pixels as rendered samples do"
    finally:
        rm.close()
        orc.close()


# ---- images against the oracle, bit for bit ----

def rank_mask(sc, rank, world):
    tiles_x, tiles_y = -(-sc.x_res // 8), -(-sc.y_res // 8)
    own = np.array([[(tx + ty) % world == rank for tx in range(tiles_x)] for ty in range(tiles_y)])
    return np.repeat(np.repeat(own, 8, 0), 8, 1)[:sc.y_res, :sc.x_res]


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("case", ["24x16", "24x16 in chunks 1+2+1", "160x120", "160x120 rank 1 of 3"])
def test_images_equal_the_oracle(case, schedule, builder):
    """every plane, the RNG, the sample counts and bounce_samples.  At 160 x 120 several hundred waves spill at the same time: two
    regions that overlap show as wrong pixels."""
    frame = SMALL if case.startswith("24") else LARGE
    sc = scene("shells", frame)
    rank, world = (1, 3) if "rank" in case else (0, 1)
    rm = manager(sc, SCHEDULES[schedule] | BUILDERS[builder], rank, world)
    try:
        for n in ([1, 2, 1] if "chunks" in case else [SPP]):
            rm.render(n)
        g = outputs(rm)
        if schedule == "stream+counters":
            assert g["counters"]["node_visits"] > 0       # (the counting instances ran)
    finally:
        rm.close()
    assert_bit_equal(g, oracle_frame("shells", frame), f"{case} {schedule} {builder}", mask=rank_mask(sc, rank, world) if world > 1 else None)


# ---- the first-hit passes ----

@pytest.mark.parametrize("builder", list(BUILDERS))
def test_first_hit_passes_equal_their_replays(builder, monkeypatch):
    """feature planes, id planes, er_pick at a spilling pixel and the history of a camera stepped back against the replays the tests of those passes
    hold (imported, not copied), on the 160 x 120 frame: 300 tiles of spilling rays.  Measured: the history's classes after the step back
    are 8 348 valid, 3 018 partial, 17 rejected and 7 817 sky pixels, under either builder."""
    import test_gpu_features as tf
    import test_gpu_history as th
    import test_gpu_ids as ti
    sc = scene("shells", LARGE)
    objects = [dts.inner_object(sc), np.arange(0, 64, dtype=np.uint32)]
    monkeypatch.setattr(tf, "scene", lambda name: sc)
    n = 2
    want_a, want_d, hits = tf.planes_numpy("deep-tree-shells", n)
    tri, _, _ = traced_ids(n)
    rm = manager(sc, BUILDERS[builder], max_bounces=2)
    try:
        rm.set_objects(objects)
        _, entries, marginal = assert_deep(sc, rm, builder, "first-hit passes", LARGE)
        rm.render_features(n)
        assert 0 < (hits > 0).sum() < hits.size
        assert tf.differing(rm.get_feature("albedo"), want_a) == 0 and tf.differing(rm.get_feature("depth"), want_d) == 0
        rm.render_ids(n)
        for kind in ti.KINDS:
            gi, gc = rm.get_ids(kind)
            wi, wc, _ = ids.planes(ti.kind_ids(sc, tri, kind, objects), tri >= 0)
            bad = int(((gi.reshape(wi.shape) != wi) | (gc.reshape(wc.shape) != wc)).any(-1).sum())
            assert bad == 0, f"{kind}: {bad} pixels differ from the replay"
        # er_pick: ray 0 of a pixel whose centre ray spills and hits -- slot 0 of a one-ray id pass, the distance of a one-ray depth plane
        rm.render_ids(1)
        rm.render_features(1)
        planes, depth = {k: rm.get_ids(k) for k in ti.KINDS}, rm.get_feature("depth")
        spilling = np.nonzero((entries >= LDS + 4) & ~marginal & (tri[:, 0] >= 0))[0]
        assert len(spilling) > 1000
        for idx in spilling[:: len(spilling) // 8][:8]:
            x, y = int(idx % sc.x_res), int(idx // sc.x_res)
            p = rm.pick(x, y)
            assert p["hit"] == 1 and p["triangle"] == int(tri[idx, 0]), (x, y)
            for k in ti.KINDS:
                assert p[k] == int(planes[k][0][y, x, 0]), (x, y, k)
            assert bits(p["distance"]) == bits(depth[y, x, 0]), (x, y)
        # the key plane: a capture, the camera stepped back by 1e-5 along its axis (its rays still spill: asserted), a resolve.  The
        # nearest shells shift by up to half a pixel, so the taps are real bilinear ones and some pixels are partial or rejected
        cam = dts.stepped_back_camera(sc)
        unit = np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(f32).reshape(12), (len(objects), 1))
        old = dict(key=key_plane_of_the_large_frame(False), cam=abi.debug_history_camera(sc.camera), poses=unit)
        new = dict(key=key_plane_of_the_large_frame(True), cam=abi.debug_history_camera(cam), poses=unit)
        e2, m2 = dts.first_descent_entries(rm.debug_read_accel(), *dts.pixel_centre_rays(with_arrays(sc, camera=cam)))
        assert m2.mean() <= 0.02 and (e2[~m2] >= LDS + 4).mean() >= 0.5
        rm.render(2)
        beauty, samples = rm.get_pass("beauty"), rm.read_samples()
        rm.history_capture()
        rm.update(camera=cam)
        rm.history_resolve()
        want_hist, _, cls, moved = th.resolve(old, new, history.capture(beauty, samples, None, 32.0), sc.x_res, sc.y_res)
        th.assert_words(rm.get_history(), want_hist, f"{builder}: history")
        info, c = rm.history_info(), history.class_counts(cls)
        print(f"{builder} builder: history classes {c}")
        assert {k: info["pixels_" + k] for k in history.CLASS_NAMES} == c and sum(c.values()) == sc.x_res * sc.y_res, (info, c)
        assert c["valid"] > 1000 and c["partial"] > 1000 and c["sky"] > 1000       # (by the replay alone: the move is no identity)
    finally:
        rm.close()


@functools.lru_cache(maxsize=None)
def key_plane_of_the_large_frame(stepped_back):
    import test_gpu_history as th
    sc = scene("shells", LARGE)
    seen = with_arrays(sc, camera=dts.stepped_back_camera(sc)) if stepped_back else sc
    return th.key_plane(seen, [dts.inner_object(sc), np.arange(0, 64, dtype=np.uint32)])


@functools.lru_cache(maxsize=None)
def traced_ids(n):
    import test_gpu_ids as ti
    return ti.traced(scene("shells", LARGE), n)


# ---- after an edit ----

@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("edit", ["scaled", "posed"])
def test_after_an_edit_the_tree_is_as_deep_and_the_image_the_oracles(edit, builder):
    """er_render_update scaling every vertex by 1.5 about the origin / er_render_transform of the inner shells: after the refit, and after
    a rebuild in the call (ER_REBUILD_ALWAYS), the structure checks clean, is as deep as before, and the image is a fresh scene's and
    the oracle's"""
    sc, sc_new = scene("shells", SMALL), scene(edit, SMALL)
    want = oracle_frame(edit, SMALL)
    fresh = manager(sc_new, BUILDERS[builder] | abi.FLAG_WAVEFRONT)
    try:
        fresh.render(SPP)
        assert_bit_equal(outputs(fresh), want, f"{edit} {builder}: a fresh scene")
    finally:
        fresh.close()
    rm = manager(sc, BUILDERS[builder] | abi.FLAG_WAVEFRONT)
    try:
        depth8 = rm.debug_read_accel()["max_depth8"]
        if edit == "posed":
            rm.set_objects([dts.inner_object(sc)])
        for policy in (abi.REBUILD_NEVER, abi.REBUILD_ALWAYS):
            rm.set_update_policy(policy)
            rm.render(1)                                              # (some state for the edit to start over from)
            if edit == "scaled":
                rm.update(vertices=sc_new.vertices)
            else:
                rm.transform({0: dts.inner_pose()})
            what = f"{edit} {builder} {'refit' if policy == abi.REBUILD_NEVER else 'rebuild'}"
            d, _, _ = assert_deep(sc_new, rm, builder, what)
            if policy == abi.REBUILD_NEVER:
                assert d["max_depth8"] == depth8, what                # a refit keeps the topology
            else:
                assert rm.rebuild_info()["rebuilds"] >= 1, rm.rebuild_info()
            rm.render(SPP)
            assert_bit_equal(outputs(rm), want, what)
    finally:
        rm.close()
