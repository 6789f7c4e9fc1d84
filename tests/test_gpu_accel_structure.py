"""The acceleration structure as it lies in DEVICE memory (er_debug_read_accel), whichever builder made it, judged by tests/accel_check.py;
the device build's determinism; the two builders' agreement where they claim it; and every triangle as the answer to a query aimed at
it, through the production traversal (er_debug_trace_rays) and the exact routine (er_debug_closest_hit) against the oracle's throwRay.

An image comparison says "0.04 % of pixels differ".  These say which node, slot, record or ray is wrong."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import accel_check
from elevenrender_amd import abi, render, scenes
from test_accel_check_cpu import SPECIAL, small_soup, translated_soup

pytestmark = pytest.mark.gpu

BUILDERS = {"host": abi.FLAG_HOST_BUILD, "device": abi.FLAG_GPU_BUILD, "default": 0}
# soups: one 256-thread block and less (3, 64), one triangle over a block (257), the global-atomic and the per-wave-LDS binning of k_sah_bin
# at several widths, triangle counts that are no multiple of 64 (20001), the default builder's threshold (20000) from above
CASES = ["soup-3", "soup-64", "soup-257", "soup-6000", "soup-20001", "soup-30000", "torture", "blobs",
         "same-centroid", "duplicates", "clusters", "translated", "flat-grid", "varied-257", "varied-6000"]
ASSERT_BUILDER_FROM = 6000        # tests/test_gpu_build.py asserts accel_info()["builder"] from this size up


@functools.lru_cache(maxsize=None)
def scene(case):
    if case.startswith("soup-"):
        return small_soup(int(case[5:]))
    if case == "torture":       # materials and tangents that are not constant (uvs and signs that are not: the "varied" cases)
        return scenes.torture(6000, 32, 24, seed=6, n_materials=8, tex_size=16, hdri_size=(32, 16))
    if case == "blobs":
        return scenes.blob_instances(n_instances=30, tris_per_blob=300, x_res=32, y_res=24, grid=(5, 3, 2), spacing=0.45)
    return SPECIAL[case]()


def read_structure(sc, flags):
    rm = render.RenderingManager(render.RenderParameters(max_bounces=4, flags=flags))
    rm.start_rendering(sc)
    dump, info = rm.debug_read_accel(), rm.accel_info()
    rm.close()
    return dump, info


@functools.lru_cache(maxsize=None)
def structure(case, builder):
    return read_structure(scene(case), BUILDERS[builder])


def raw_buffers(d):
    return {"nodes": d["nodes"].tobytes(), "nodes8": d["nodes8"].tobytes() + d["node8_stride_tail"].tobytes(), "isect": d["isect"].tobytes(), "attr": d["attr"].tobytes()}


@pytest.mark.parametrize("case,builder", [(c, b) for c in CASES for b in ("host", "device")] + [("soup-30000", "default")])
def test_structure_in_device_memory_checks_clean(case, builder):
    sc = scene(case)
    d, info = structure(case, builder)
    rep = accel_check.check(sc, d, accel_depth=info["max_depth"])
    print(f"{case} / {builder} asked: builder {info['builder']} answered; {sc.tri_count} triangles, {d['node_count']} binary nodes (depth {rep.depth2}), "
          f"{d['node8_count']} wide nodes (depth {rep.depth8})")
    assert d["builder"] == info["builder"] and d["node8_count"] == info["node_count"] and d["tri_count"] == sc.tri_count
    assert d["lift_bound"] == np.float32(info["lift_bound"])
    if builder == "default":
        assert info["builder"] == (1 if sc.tri_count >= 20000 else 0)
    elif sc.tri_count >= ASSERT_BUILDER_FROM:
        assert info["builder"] == (1 if builder == "device" else 0)
    assert rep.ok, rep.message()


def test_read_accel_before_begin_and_short_buffers():
    import ctypes as C
    lib = abi.load()
    sc = scene("soup-64")
    h = C.c_void_p()
    abi.check(lib.er_scene_create(C.byref(sc.desc()), C.byref(h)))
    info = abi.ErAccelDump()
    try:
        assert lib.er_debug_read_accel(h, C.byref(info), None, 0, None, 0, None, 0, None, 0) == abi.ER_ERR_STATE
        p = abi.ErRenderParams(1, 8, 4, 0, 0, 1, 0)
        abi.check(lib.er_render_begin(h, C.byref(p)))
        assert lib.er_debug_read_accel(h, C.byref(info), None, 0, None, 0, None, 0, None, 0) == abi.ER_OK
        assert info.tri_count == 64 and info.node8_count >= 1 and info.node8_pieces >= 5 and info.attr_pieces >= 7
        buf = np.zeros((info.tri_count + 1) * 48, np.uint8)
        assert lib.er_debug_read_accel(h, C.byref(info), None, 0, None, 0, buf.ctypes.data_as(C.c_void_p), buf.nbytes - 1, None, 0) == abi.ER_ERR_INVALID_ARG
        assert lib.er_debug_read_accel(h, C.byref(info), None, 0, None, 0, buf.ctypes.data_as(C.c_void_p), buf.nbytes, None, 0) == abi.ER_OK
        assert buf[:48].any() and not buf[-48:].any()
    finally:
        lib.er_scene_destroy(h)


def test_device_build_is_deterministic():
    """er_gpu_build.hip: "the layout never depends on thread timing" -- two builds of one scene, every byte of the four buffers."""
    a = raw_buffers(structure("soup-30000", "device")[0])
    d2, _ = read_structure(scene("soup-30000"), abi.FLAG_GPU_BUILD)
    b = raw_buffers(d2)
    differ = {}
    for k in a:
        if a[k] != b[k]:
            x, y = np.frombuffer(a[k], np.uint8), np.frombuffer(b[k], np.uint8)
            differ[k] = (len(x), len(y), int(np.nonzero(x[:min(len(x), len(y))] != y[:min(len(x), len(y))])[0][0]) if len(x) == len(y) else -1)
    # (which pass: nodes = the binned-SAH levels / k_fix_leaves, nodes8 = k_dp / k_wide_emit, isect and attr = k_records over the final order)
    assert not differ, f"buffers differ between two device builds (buffer: lengths, first differing byte): {differ}"


@pytest.mark.parametrize("case", CASES)
def test_builders_agree_where_they_say_they_do(case):
    """The bounds are the same union of the same padded boxes; each triangle's lift is the same arithmetic (both within the checker's
    band, test above, and here bit-equal by triangle id).  The trees themselves may differ where bins round differently: printed."""
    (h, hi), (d, di) = structure(case, "host"), structure(case, "device")
    n = scene(case).tri_count
    if di["builder"] != 1:
        pytest.fail(f"{case}: the forced device build was answered by builder {di['builder']}")
    assert h["lo"].tobytes() == d["lo"].tobytes() and h["hi"].tobytes() == d["hi"].tobytes(), (h["lo"], d["lo"], h["hi"], d["hi"])
    assert h["lift_bound"] == d["lift_bound"] and h["max_lift"] == d["max_lift"]
    lh, ld = np.zeros(n, np.float32), np.zeros(n, np.float32)
    lh[h["isect"]["tri_id"][:n]] = h["isect"]["lift"][:n]
    ld[d["isect"]["tri_id"][:n]] = d["isect"]["lift"][:n]
    tl = accel_check.lift_bounds(scene(case).vertices, scene(case).normals)
    for l in (lh, ld):
        assert ((tl <= l) & (l <= 1.02 * tl + 1e-29)).all()
    m = min(len(h["nodes8"]), len(d["nodes8"]))
    same = (h["nodes8"][:m].view(np.uint8).reshape(m, -1) == d["nodes8"][:m].view(np.uint8).reshape(m, -1)).all(1).sum() / max(len(h["nodes8"]), len(d["nodes8"]))
    print(f"{case}: {n} triangles; wide nodes host {len(h['nodes8'])} / device {len(d['nodes8'])}, byte-equal {same:.4f}; lift bit-equal {float((lh == ld).mean()):.4f}; "
          f"depth host {hi['max_depth']} / device {di['max_depth']}")


# ---- every triangle is the answer to a query ----

BARY = np.array([[1 / 3, 1 / 3, 1 / 3], [0.998, 0.001, 0.001], [0.001, 0.998, 0.001], [0.001, 0.001, 0.998],
                 [0.4995, 0.4995, 0.001], [0.4995, 0.001, 0.4995], [0.001, 0.4995, 0.4995]], np.float64)


def aimed_rays(sc, bary, seed=13):
    """len(bary) rays per triangle, triangle-major: towards the barycentric targets along the geometric normal (sign alternating per
    triangle) tilted by a seeded N(0, 0.2) vector, from h = 0.05 e in front of the target, e = 2 / cbrt(n) the soup's triangle size."""
    v = sc.vertices.reshape(-1, 3, 3).astype(np.float64)
    n = len(v)
    h = 0.05 * 2.0 / np.cbrt(n)
    ng = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    ng *= np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None]
    rng = np.random.default_rng(seed)
    d = ng[:, None, :] + rng.normal(0.0, 0.2, size=(n, len(bary), 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    target = np.einsum("kb,nbc->nkc", bary, v)
    o = target - d * h
    return o.reshape(-1, 3).astype(np.float32), d.reshape(-1, 3).astype(np.float32), np.repeat(np.arange(n), len(bary)), np.float32(h)


def oracle_hits(orc, o, d, threads=16):
    """Oracle.closest_hit over `threads` chunks (the call is a serial loop that holds no lock and writes only its own outputs)"""
    cuts = np.linspace(0, len(o), threads + 1).astype(int)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda k: orc.closest_hit(o[cuts[k]:cuts[k + 1]], d[cuts[k]:cuts[k + 1]]), range(threads)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


AIMED = {"soup-6000": (BARY, 0.0), "translated": (BARY, 0.0), "soup-30000": (BARY, 0.0), "blobs": (BARY[:1], 2e-4)}


@functools.lru_cache(maxsize=None)
def aimed_reference(case, oracle_mod):
    """rays and the oracle's answers, once per scene: the closest hit, and the last hit within 2 h seen from the far end (for the shadow form)"""
    sc = scene(case)
    bary, _ = AIMED[case]
    o, d, own, h = aimed_rays(sc, bary)
    orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, max_bounces=4, threads=16)
    otri, opos = oracle_hits(orc, o, d)
    # The shadow form exempts the first hit and asks whether ANOTHER triangle is hit nearer than 2 h.  The oracle only answers closest
    # hits, so it is asked twice more, from either end of what lies behind the first hit:
    #  (back)  the ray reversed, from just beyond 2 h: its closest hit is the LAST triangle the segment meets -- the first hit itself if
    #          nothing lies behind it (nothing lies before it: it is the closest), else another triangle.  A triangle between 2 h and
    #          the reversed ray's start hides the segment; the ray then goes on from just behind that triangle's plane;
    #  (on)    the ray continued from 1e-3 h behind the plane of the triangle it hit (float64 ray / plane distance; a little further
    #          where float32 rounding of the new origin left it in front of that plane: at coordinates of 60 an ulp is 4e-6).
    # (on) cannot see a triangle within that step of the first hit, and (back) meets the aimed-at triangle from the other side, where
    # a ray 0.001 of the triangle from an edge may graze differently.  The test judges the rays on which the two agree.
    v = sc.vertices.reshape(-1, 3, 3).astype(np.float64)
    o64, d64, lim, step = o.astype(np.float64), d.astype(np.float64), 2.0 * float(h), 1e-3 * float(h)

    def plane_t(rays, tris):
        ng = np.cross(v[tris, 1] - v[tris, 0], v[tris, 2] - v[tris, 0])
        return ((v[tris, 0] - o64[rays]) * ng).sum(-1) / (d64[rays] * ng).sum(-1)

    back = np.ascontiguousarray(-d)
    o2 = (o64 + d64 * (lim * 1.001)).astype(np.float32)
    tri2, pos2 = oracle_hits(orc, o2, back)
    for _ in range(4):
        along = ((pos2.astype(np.float64) - o64) * d64).sum(-1)
        again = np.nonzero((tri2 >= 0) & (along > 0) & (np.linalg.norm(pos2.astype(np.float64) - o64, axis=1) >= lim))[0]
        if not len(again):
            break
        o2[again] = (o64[again] + d64[again] * (plane_t(again, tri2[again]) - step)[:, None]).astype(np.float32)
        tri2[again], pos2[again] = orc.closest_hit(o2[again], back[again])
    hit = np.nonzero(otri >= 0)[0]
    t1 = plane_t(hit, otri[hit])
    o3 = o.copy()
    o3[hit] = (o64[hit] + d64[hit] * (t1 + step)[:, None]).astype(np.float32)
    tri3, pos3 = oracle_hits(orc, o3, d)
    for _ in range(4):
        again = np.nonzero(tri3[hit] == otri[hit])[0]
        if not len(again):
            break
        step *= 8
        o3[hit[again]] = (o64[hit[again]] + d64[hit[again]] * (t1[again] + step)[:, None]).astype(np.float32)
        tri3[hit[again]], pos3[hit[again]] = orc.closest_hit(o3[hit[again]], d[hit[again]])
    tri3[otri < 0] = -1          # (a ray that missed has nothing behind it either)
    orc.close()
    return o, d, own, h, otri, opos, tri2, pos2, tri3, pos3


@pytest.mark.parametrize("case,builder", [("soup-6000", "host"), ("soup-6000", "device"), ("translated", "host"), ("translated", "device"),
                                          ("soup-30000", "default"), ("blobs", "host"), ("blobs", "device")])
def test_every_triangle_is_the_answer_to_a_query(oracle_mod, case, builder):
    sc = scene(case)
    bary, tol = AIMED[case]
    n, k = sc.tri_count, len(bary)
    o, d, own, h, otri, opos, tri2, pos2, tri3, pos3 = aimed_reference(case, oracle_mod)
    own_share = float((otri == own).mean())
    answered = float((otri == own).reshape(n, k).any(1).mean())
    print(f"{case} / {builder}: {len(o)} rays, oracle: own-triangle share {own_share:.4f}, triangles answering one of their rays {answered:.4f}, misses {int((otri < 0).sum())}")
    if tol == 0.0:      # the test traces something relevant: conditions on the oracle alone (soups: 0.990-0.992 and 1.0 measured on the CPU)
        assert own_share >= 0.98
        assert answered == 1.0
    rm = render.RenderingManager(render.RenderParameters(max_bounces=4, flags=BUILDERS[builder]))
    rm.start_rendering(sc)
    print(f"   builder {rm.accel_info()['builder']} answered, {rm.accel_info()['node_count']} wide nodes")
    tri, slot, pos, dist, info = rm.debug_trace_rays(o, d)
    etri, epos, edist = rm.debug_closest_hit(o, d)
    # shadow form: the same rays, the first hit exempt, limit 2 h -- occluded iff ANOTHER triangle is hit nearer than 2 h
    limit = np.full(len(o), 2 * h, np.float32)
    occ, sinfo = rm.debug_trace_rays(o, d, self_slots=np.where(tri >= 0, slot, -1).astype(np.int32), limits=limit)
    rm.close()
    for what, t, p in (("production traversal", tri, pos), ("exact routine", etri, epos)):
        bad = ((t < 0) != (otri < 0)) | (t != otri) | (p.view(np.uint32) != opos.view(np.uint32)).any(-1)
        w = np.nonzero(bad)[0]
        print(f"   {what}: {len(w)} rays differ from the oracle" + "".join(f"; ray {i} (triangle {own[i]}, target {i % k}): got {t[i]} {p[i]}, oracle {otri[i]} {opos[i]}" for i in w[:3]))
        assert bad.mean() <= tol, (what, len(w))
    margin = 1e-5 * np.maximum(1.0, limit)                                                # around the threshold itself (tests/test_gpu_function_level.py)
    metric = lambda p: np.sqrt(((p - o).astype(np.float32) ** 2).sum(-1, dtype=np.float32))   # the hit's metric in numpy f32 (not bit-critical: see margin)
    fdist, bdist, cdist = metric(opos), metric(pos2), metric(pos3)
    nothing = (otri < 0) | (fdist > limit + margin)                                       # the closest hit of all lies beyond the limit: nothing can occlude
    other_b = (tri2 >= 0) & (tri2 != otri) & (((pos2 - o) * d).sum(-1) > 0) & ~nothing    # (not behind the origin: a reversed ray that slipped past the first hit)
    other_c = (tri3 >= 0) & (tri3 != otri) & ~nothing
    ref_occ, occ_c = other_b & (bdist < limit), other_c & (cdist < limit)
    # not judged: rays on which the oracle's two views differ (comment in aimed_reference), and the threshold itself
    near = (other_b & (np.abs(bdist - limit) <= margin)) | (other_c & (np.abs(cdist - limit) <= margin)) | ((otri >= 0) & (np.abs(fdist - limit) <= margin))
    clear = (ref_occ == occ_c) & ~near
    bad = (occ != ref_occ) & clear
    print(f"   shadow form: {int(occ.sum())} occluded (oracle {int(ref_occ.sum())}), {int(bad.sum())} differ; not judged {int((~clear).sum())} ({int((ref_occ != occ_c).sum())} where the oracle's two views differ); "
          f"exact resolves {int((sinfo >= 2).sum())}")
    assert clear.mean() >= 0.99           # (the oracle alone: the shadow form judges the rays, not the exceptions; 0.9986 - 1.0 on these scenes)
    assert bad.mean() <= tol, int(bad.sum())
