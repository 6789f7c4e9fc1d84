"""The feature pass (er_render_features: first-hit albedo and depth through the production traversal, csrc/er_features.hip) and the
denoise guided by its planes (er_denoise_guided) on the GPU.

(a) both planes against a numpy float32 replay composed from the oracle's function-level entry points, every pixel bit-equal;
(b) coverage against the NORMAL plane of the path; (c) a feature pass leaves the render's state alone, in every schedule;
(d) er_render_update invalidates the planes and a new pass equals a fresh scene's; (e) sharded: gathered planes and the guided
denoise equal the one-rank ones; (f) the filter against a numpy replay, bit for bit; (g) its error on textured content against the
plain filter's; (h) the planes and the guided denoise through the host server."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as orc
import uv_scenes
from elevenrender_amd import abi, client, render, scenes
from test_gpu_denoise import atrous_numpy
from test_gpu_update import assert_same_outputs, edit_J, moved_camera, outputs, with_arrays
from test_host_server import Server, session_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
BUILDERS = {"host": abi.FLAG_HOST_BUILD, "device": abi.FLAG_GPU_BUILD}
SCHEDULES = {"stream": abi.FLAG_STREAM, "wavefront": abi.FLAG_WAVEFRONT, "megakernel": abi.FLAG_MEGAKERNEL}


def same(a, b):
    return (np.ascontiguousarray(a, f32).view(np.uint32) == np.ascontiguousarray(b, f32).view(np.uint32)).all()


def differing(a, b):
    return int((np.ascontiguousarray(a, f32).view(np.uint32) != np.ascontiguousarray(b, f32).view(np.uint32)).any(-1).sum())


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "torture-600":
        return scenes.torture(600, 32, 24, seed=7, n_materials=8, tex_size=32, hdri_size=(64, 32), n_lights=4)
    if name == "torture-4000":      # 70 x 45: partial tiles on both edges; one bilinear albedo texture, one constant albedo
        sc = scenes.torture(4000, 70, 45, seed=7, n_materials=8, tex_size=32, hdri_size=(64, 32), n_lights=4)
        d, w, h, ch, _ = sc.textures[0]
        sc.textures[0] = (d, w, h, ch, 1)
        sc.materials[1] = abi.default_material(albedo=(0.3, 0.6, 0.2), roughness_tex=4, metallic_tex=5)
        sc._desc = None
        return sc
    if name in uv_scenes.KINDS:     # varied, tiled and negative uvs on a frame of 48 x 32: the fused and the plain albedo fetch outside [0, 1]^2
        return uv_scenes.tiled(name, 48, 32)
    if name == "torture-filter":
        return scenes.torture(4000, 70, 45, n_materials=8, tex_size=32)
    raise KeyError(name)


# ---- (a) the planes, replayed from the oracle's entry points ----

@functools.lru_cache(maxsize=None)
def oracle_samples(name, n_max=4):
    """Per pixel and sample k < n_max: (hit, albedo a_k, distance d_k), from oracle_rng_stream (five draws per sample), oracle_camera_ray,
    Oracle.closest_hit, oracle_tri_hit and oracle_texture_fetch.  Computed once per scene and shared."""
    sc = scene(name)
    L = orc.lib()
    fp = lambda a: np.ascontiguousarray(a, f32).ctypes.data_as(C.POINTER(C.c_float))
    npx = sc.x_res * sc.y_res
    origins, dirs = np.zeros((npx, n_max, 3), f32), np.zeros((npx, n_max, 3), f32)
    for idx in range(npx):
        st, va = (C.c_uint32 * (5 * n_max))(), (C.c_float * (5 * n_max))()
        L.oracle_rng_stream(idx, 5 * n_max, st, va)
        for k in range(n_max):
            o, d = (C.c_float * 3)(), (C.c_float * 3)()
            L.oracle_camera_ray(C.byref(sc.camera), sc.x_res, sc.y_res, idx % sc.x_res, idx // sc.x_res, (C.c_float * 5)(*va[5 * k:5 * k + 5]), orc.MATH_ER, o, d)
            origins[idx, k], dirs[idx, k] = o[:], d[:]
    o = orc.Oracle(sc, math_mode=orc.MATH_ER, max_bounces=1)
    tri, _ = o.closest_hit(origins.reshape(-1, 3), dirs.reshape(-1, 3))
    o.close()
    tri = tri.reshape(npx, n_max)
    hit = tri >= 0
    alb, dist = np.ones((npx, n_max, 3), f32), np.zeros((npx, n_max), f32)
    V, N, T, UV = sc.vertices.reshape(-1, 9), sc.normals.reshape(-1, 9), sc.tangents.reshape(-1, 9), sc.uvs.reshape(-1, 6)
    texs = [abi.ErTexture(w, h, ch, flt, abi._fptr(data)) for (data, w, h, ch, flt) in sc.textures]
    branches = set()
    for idx, k in zip(*np.nonzero(hit)):
        t = int(tri[idx, k])
        rec = np.zeros(17, f32)
        assert L.oracle_tri_hit(fp(V[t]), fp(N[t]), fp(T[t]), fp(UV[t]), float(sc.tangent_sign[t]), fp(origins[idx, k]), fp(dirs[idx, k]), fp(rec))
        p = (rec[0:3] - origins[idx, k]).astype(f32)
        dist[idx, k] = np.sqrt(f32(f32(p[0] * p[0]) + f32(p[1] * p[1])) + f32(p[2] * p[2]))
        m = sc.materials[int(sc.material_id[t])]
        assert m.albedo_shader_id == -1
        if m.albedo_tex < 0:
            alb[idx, k] = (m.albedo.x, m.albedo.y, m.albedo.z)
            branches.add("constant")
        else:
            out = np.zeros(3, f32)
            L.oracle_texture_fetch(C.byref(texs[m.albedo_tex]), float(rec[15]), float(rec[16]), 1, fp(out))      # (filtered: by the texture's own filter)
            alb[idx, k] = out
            branches.add("bilinear" if sc.textures[m.albedo_tex][4] == 1 else "unfiltered")
    return hit, alb, dist, branches


def planes_numpy(name, n):
    """the stated sum order: A += a_k and D += d_k for k = 0 .. n - 1, then A / (float)n, D / (float)hits, hits / (float)n"""
    sc = scene(name)
    hit, alb, dist, _ = oracle_samples(name)
    npx = sc.x_res * sc.y_res
    A, D, hits = np.zeros((npx, 3), f32), np.zeros(npx, f32), np.zeros(npx, np.uint32)
    for k in range(n):
        A = (A + alb[:, k]).astype(f32)
        D = np.where(hit[:, k], (D + dist[:, k]).astype(f32), D)
        hits += hit[:, k]
    cov = (hits.astype(f32) / f32(n)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(hits > 0, (D / hits.astype(f32)).astype(f32), f32(0))
    albedo = np.concatenate([(A / f32(n)).astype(f32), cov[:, None]], 1).reshape(sc.y_res, sc.x_res, 4)
    depth = np.stack([z, z, z, cov], 1).astype(f32).reshape(sc.y_res, sc.x_res, 4)
    return albedo, depth, hits.reshape(sc.y_res, sc.x_res)


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", ["torture-600", "torture-4000"] + list(uv_scenes.KINDS))
def test_planes_equal_the_replay_from_the_oracles_entry_points(name, builder):
    sc = scene(name)
    if name == "torture-4000" or name in uv_scenes.KINDS:
        assert oracle_samples(name)[3] == {"constant", "bilinear", "unfiltered"}
    rm = render.RenderingManager(render.RenderParameters(max_bounces=1, flags=BUILDERS[builder]))
    rm.start_rendering(sc)
    assert rm.accel_info()["builder"] == (1 if builder == "device" else 0)
    assert rm.feature_info() == dict(valid=0, samples=0, rays=0, ms=0.0)
    try:
        for n in (1, 4):
            rm.render_features(n)
            albedo, depth = rm.get_feature("albedo"), rm.get_feature("depth")
            want_a, want_d, hits = planes_numpy(name, n)
            assert 0 < (hits > 0).sum() < hits.size and (hits == n).any()          # hits, misses and -- at n = 4 -- partly covered pixels
            assert differing(albedo, want_a) == 0 and differing(depth, want_d) == 0, (n, differing(albedo, want_a), differing(depth, want_d))
            info = rm.feature_info()
            assert (info["valid"], info["samples"], info["rays"]) == (1, n, n * sc.x_res * sc.y_res) and info["ms"] > 0
        assert (planes_numpy(name, 4)[2] % 4 != 0).any()
        rm.render_features(0)                                                       # 0 means 4
        assert rm.feature_info()["samples"] == 4 and same(rm.get_feature("albedo"), albedo)
    finally:
        rm.close()


# ---- (b) ----

def test_coverage_is_where_the_path_found_its_first_hit():
    sc = scenes.soup(4000, 70, 45, seed=3, hdri_size=(64, 32))
    rm = render.RenderingManager(render.RenderParameters(max_bounces=1))
    rm.start_rendering(sc)
    rm.render_features(1)
    rm.render(1)
    normal, albedo, depth = rm.get_pass("normal"), rm.get_feature("albedo"), rm.get_feature("depth")
    rm.close()
    hit = (normal[..., :3] != 0).any(-1)
    assert 0 < hit.sum() < hit.size
    assert (albedo[..., 3][hit] == 1).all() and (albedo[..., 3][~hit] == 0).all() and same(albedo[..., 3], depth[..., 3])
    assert (depth[..., 0][hit] > 0).all() and (depth[..., :3][~hit] == 0).all() and (albedo[..., :3][~hit] == 1).all()
    assert (albedo[..., :3][hit] == f32(0.5)).all()                                 # the one default material


# ---- (c) ----

@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_a_feature_pass_leaves_the_render_alone(sched):
    sc = scene("torture-4000")
    got = []
    for with_features in (True, False):
        rm = render.RenderingManager(render.RenderParameters(max_bounces=4, flags=SCHEDULES[sched]))
        rm.start_rendering(sc)
        if with_features:
            rm.render_features(4)
        rm.render(4)
        if with_features:
            rm.render_features(2)                                                   # ... nor does one after the samples
        got.append((outputs(rm), rm.counters(), rm.get_render_info().samples))
        rm.close()
    assert_same_outputs(got[0][0], got[1][0], sched)
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2] == 5


# ---- (d) ----

def test_an_update_invalidates_the_planes_and_a_new_pass_equals_a_fresh_scenes():
    lib = abi.load()
    sc = scene("torture-4000")
    comm = (C.c_void_p * 1)()
    abi.check(lib.er_comm_create_local(1, comm))
    rm = render.RenderingManager(render.RenderParameters(max_bounces=4))
    rm.start_rendering(sc)
    buf = np.zeros((sc.y_res, sc.x_res, 4), f32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    guided = abi.ErDenoiseGuided(0, 0.0, 0.0, 0.0)

    def refused():
        assert rm.feature_info()["valid"] == 0
        for f in (abi.FEATURE_ALBEDO, abi.FEATURE_DEPTH):
            assert lib.er_read_feature(rm.handle, f, fp) == abi.ER_ERR_STATE
            assert b"er_render_features" in lib.er_last_error()
            assert lib.er_gather_feature(rm.handle, f, comm[0], 0) == abi.ER_ERR_STATE
        assert lib.er_denoise_guided(rm.handle, C.byref(guided)) == abi.ER_ERR_STATE

    try:
        refused()                                                                   # begun, no pass yet
        rm.render_features(4)
        before = rm.get_feature("albedo")
        edits = [("camera", dict(camera=moved_camera(sc))), ("geometry", edit_J(sc))]
        edited = sc
        for what, kw in edits:
            rm.update(**kw)
            refused()
            rm.render_features(4)
            edited = with_arrays(edited, **kw)
            fresh = render.RenderingManager(render.RenderParameters(max_bounces=4))
            fresh.start_rendering(edited)
            fresh.render_features(4)
            for name in ("albedo", "depth"):
                assert same(rm.get_feature(name), fresh.get_feature(name)), (what, name)
            fresh.close()
            assert not same(rm.get_feature("albedo"), before), what
            before = rm.get_feature("albedo")
    finally:
        rm.close()
        lib.er_comm_destroy(comm[0])


# ---- the filter's replay (f), shared with (e) ----

def guided_numpy(beauty, normal, albedo, depth, levels=0, sc=0.0, sa=0.0, sz=0.0):
    levels, sc, sa, sz = levels or 5, f32(sc or 4.0), f32(sa or 0.3), f32(sz or 0.2)
    h, w = beauty.shape[:2]
    kern = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], f32)
    one = f32(1.0)
    ap = (albedo[..., :3] + f32(0.01)).astype(f32)
    src = beauty.copy()
    src[..., :3] = beauty[..., :3] / ap
    ys, xs = np.mgrid[0:h, 0:w]
    none = (normal[..., :3] == 0).all(-1)
    a, z = albedo[..., :3], depth[..., 0]
    ka, kz = f32(one / f32(sa * sa)), f32(one / f32(sz * sz))
    for k in range(levels):
        step = 1 << k
        kc = f32(f32(one / f32(sc * sc)) * f32(1 << k))
        acc, sw = np.zeros((h, w, 3), f32), np.zeros((h, w), f32)
        c = src[..., :3]
        for j in range(-2, 3):
            for i in range(-2, 3):
                qx, qy = np.clip(xs + i * step, 0, w - 1), np.clip(ys + j * step, 0, h - 1)
                cq, nq, aq, zq = src[qy, qx, :3], normal[qy, qx, :3], a[qy, qx], z[qy, qx]
                d = (c - cq).astype(f32)
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(f32) + d[..., 2] * d[..., 2]
                wc = one / (one + kc * d2)
                nd = (normal[..., 0] * nq[..., 0] + normal[..., 1] * nq[..., 1]).astype(f32) + normal[..., 2] * nq[..., 2]
                nd = np.where(none & none[qy, qx], one, np.where(nd < 0, f32(0.0), nd)).astype(f32)
                da = (a - aq).astype(f32)
                a2 = (da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]).astype(f32) + da[..., 2] * da[..., 2]
                wa = one / (one + a2 * ka)
                r = ((z - zq) / (np.maximum(z, zq) + f32(1e-6))).astype(f32)
                wz = one / (one + (r * r).astype(f32) * kz)
                wgt = ((((kern[i + 2] * kern[j + 2]) * wc).astype(f32) * (nd * nd).astype(f32)).astype(f32) * wa).astype(f32) * wz
                acc = acc + cq * wgt[..., None]
                sw = sw + wgt
        out = src.copy()
        out[..., :3] = acc / sw[..., None]
        src = out
    res = beauty.copy()
    res[..., :3] = src[..., :3] * ap
    assert res.dtype == f32
    return res


@pytest.mark.parametrize("levels,sc,sa,sz", [(1, 4.0, 0.3, 0.2), (3, 2.0, 0.1, 0.05), (5, 0.0, 0.0, 0.0)])
def test_guided_denoise_matches_numpy_replay(levels, sc, sa, sz):
    scn = scene("torture-filter")
    rm = render.RenderingManager(render.RenderParameters(max_bounces=8))
    rm.start_rendering(scn)
    rm.render(4)
    rm.render_features()
    rm.denoise_guided(levels, sc, sa, sz)
    got = rm.get_pass("denoise")
    beauty, normal, albedo, depth = rm.get_pass("beauty"), rm.get_pass("normal"), rm.get_feature("albedo"), rm.get_feature("depth")
    want = guided_numpy(beauty, normal, albedo, depth, levels, sc, sa, sz)
    assert differing(got, want) == 0, (differing(got, want), np.abs(got - want).max())
    assert np.isfinite(got).all() and (got[..., 3] == beauty[..., 3]).all()
    assert not same(got, beauty)
    # ... and the plain filter is what it was
    rm.denoise(3, 0.5)
    plain = rm.get_pass("denoise")
    rm.close()
    assert same(plain, atrous_numpy(beauty, normal, 3, 0.5))


# ---- (e) ----

def test_sharded_features_and_guided_denoise_equal_the_one_rank_ones():
    lib = abi.load()
    sc = scene("torture-4000")
    one = render.RenderingManager(render.RenderParameters(max_bounces=4))
    one.start_rendering(sc)
    one.render(4)
    one.render_features(4)
    one.denoise_guided()
    want = {n: one.get_feature(n) for n in ("albedo", "depth")}
    want_denoised = one.get_pass("denoise")
    one.close()
    world, root = 3, 1
    comms = (C.c_void_p * world)()
    abi.check(lib.er_comm_create_local(world, comms))
    rms = []
    for r in range(world):
        rm = render.RenderingManager(render.RenderParameters(max_bounces=4, rank=r, world=world))
        rm.start_rendering(sc)
        rm.render(4, blocking=False)
        rm.render_features(4)
        rms.append(rm)
    order = [x for x in range(world) if x != root] + [root]
    g = abi.ErDenoiseGuided(0, 0.0, 0.0, 0.0)
    try:
        info = [rm.feature_info() for rm in rms]
        assert sum(i["rays"] for i in info) == 4 * sc.x_res * sc.y_res and all(i["rays"] > 0 for i in info)
        own = rms[root].get_feature("albedo")                                       # before the gather: this rank's pixels, zero elsewhere
        ys, xs = np.mgrid[0:sc.y_res, 0:sc.x_res]
        mine = (xs // 8 + ys // 8) % world == root
        assert same(own[mine], want["albedo"][mine]) and (own[~mine] == 0).all()
        assert lib.er_denoise_guided(rms[root].handle, C.byref(g)) == abi.ER_ERR_STATE
        for word in (b"BEAUTY", b"NORMAL", b"ALBEDO", b"DEPTH"):
            assert word in lib.er_last_error()
        for p in (abi.PASS_BEAUTY, abi.PASS_NORMAL):
            for r in order:
                abi.check(lib.er_gather_pass(rms[r].handle, p, comms[r], root))
        assert lib.er_denoise_guided(rms[root].handle, C.byref(g)) == abi.ER_ERR_STATE          # the features are still sharded
        msg = lib.er_last_error()
        assert b"ALBEDO" in msg and b"DEPTH" in msg and b"BEAUTY" not in msg
        for f in (abi.FEATURE_ALBEDO, abi.FEATURE_DEPTH):
            for r in order:
                abi.check(lib.er_gather_feature(rms[r].handle, f, comms[r], root))
        for n in ("albedo", "depth"):
            assert same(rms[root].get_feature(n), want[n]), n
        rms[root].denoise_guided()
        assert same(rms[root].get_pass("denoise"), want_denoised)
        assert lib.er_denoise_guided(rms[0].handle, C.byref(g)) == abi.ER_ERR_STATE             # a rank that nothing was gathered to
        assert lib.er_gather_feature(rms[0].handle, 0, comms[2], root) == abi.ER_ERR_INVALID_ARG
        # a new pass on the root makes its gathered pixels stale again
        rms[root].render_features(4)
        assert lib.er_denoise_guided(rms[root].handle, C.byref(g)) == abi.ER_ERR_STATE
    finally:
        for rm in rms:
            rm.close()
        for c in comms:
            lib.er_comm_destroy(c)


# ---- (g) ----

def test_guided_denoise_beats_the_plain_filter_on_textured_content():
    """cornell_textured(96, 96), 4 spp against 1 024 spp, both scaled by (n + 1) / n as tests/test_gpu_denoise.py does.  A float64
    numpy replay on the oracle's images gave 0.0284 for the guided filter's defaults against 0.0483 for the best plain one (0.59);
    without the demodulation, or with the plain filter's colour sigma of 1 on the demodulated signal (1.07), the bound fails."""
    sc = scenes.cornell_textured(96, 96)
    rm = render.RenderingManager(render.RenderParameters(max_bounces=5))
    rm.start_rendering(sc)
    rm.render(4)
    rm.render_features()
    noisy = rm.get_pass("beauty")
    plain = {}
    for sigma in (0.5, 1.0, 2.0):
        rm.denoise(5, sigma)
        plain[sigma] = rm.get_pass("denoise")
    rm.denoise_guided()
    guided = rm.get_pass("denoise")
    rm.render(1020)
    ref = rm.get_pass("beauty")[..., :3] * f32(1025 / 1024)
    rm.close()
    err = lambda img: float(np.abs(img[..., :3] * f32(5 / 4) - ref).mean())
    e_plain = {s: err(p) for s, p in plain.items()}
    print("mean abs error vs 1024 spp: 4 spp", err(noisy), "er_denoise", e_plain, "er_denoise_guided", err(guided))
    assert err(guided) <= 0.75 * min(e_plain.values())


# ---- (h) ----

def test_host_session_serves_the_feature_planes_and_the_guided_denoise(tmp_path):
    a = client.cornell_session_assets(100, 76)                                      # partial tiles on both edges
    frames = {}
    for gpus in (1, 3):
        s = Server()
        c = client.Client(port=s.port)
        extra = dict(gpus=3, devices=[0, 0, 0], transport="local") if gpus == 3 else {}
        beauty = client.play_cornell_session(c, a, sample_target=5, denoise_guided=True, feature_samples=2, **extra)
        info = c.get_info()
        assert info["samples"] == 6 and info["gpus"] == gpus and info["feature_samples"] == 2 and info["denoise_guided"] is True
        frames[gpus] = dict(beauty=beauty, albedo=c.get_pass("albedo", 100, 76), depth=c.get_pass("Depth", 100, 76), denoise=c.get_pass("denoise", 100, 76))
        c.close()
        assert s.finish() == 0
    sc = session_scene(a, tmp_path)
    rm = render.RenderingManager(render.RenderParameters())
    rm.start_rendering(sc)
    rm.render(5)
    rm.render_features(2)
    rm.denoise_guided()
    direct = dict(beauty=rm.get_pass("beauty"), albedo=rm.get_feature("albedo"), depth=rm.get_feature("depth"), denoise=rm.get_pass("denoise"))
    rm.close()
    direct["denoise"][..., 3] = 1                                                   # (the session sends a denoised image with alpha 1)
    assert len(np.unique(direct["albedo"][..., :3].reshape(-1, 3), axis=0)) > 4          # the checker floor, three walls, the light, the misses
    for gpus in (1, 3):
        for k in direct:
            assert same(frames[gpus][k], direct[k]), (gpus, k)
