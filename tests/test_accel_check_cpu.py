"""The host builder's structure itself (er_build_bvh + er_collapse_bvh8 through er_debug_bvh_dump), judged by tests/accel_check.py -- and
the checker's ability to fail: ten corruptions of an intact dump, each of which it must report under the matching name.  No GPU.

The scenes of this file are also those of tests/test_gpu_accel_structure.py, which reads the same structure back from device memory
under either builder."""
import numpy as np
import pytest

import accel_check
import uv_scenes
from elevenrender_amd import abi, scenes


def small_soup(n, seed=13):
    return scenes.soup(n, 32, 24, seed=seed, hdri_size=(32, 16))


def _with_vertices(sc, v):
    sc.vertices = np.ascontiguousarray(np.asarray(v, np.float32).reshape(sc.vertices.shape))
    sc._desc = None
    return sc


def same_centroid():
    """every centroid at (0, 0, 3), bit-equal for many triangles (tests/test_gpu_build.py): no axis to bin on"""
    sc = scenes.soup(64, 32, 24, seed=5, hdri_size=(32, 16))
    w = sc.vertices.reshape(-1, 3, 3).copy()
    w = w - w.mean(1, keepdims=True) + np.array([0.0, 0.0, 3.0], np.float32)
    return _with_vertices(sc, np.round(w * 64) / 64)


def duplicates():
    """64 copies of one triangle"""
    sc = scenes.soup(64, 32, 24, seed=5, hdri_size=(32, 16))
    w = sc.vertices.reshape(-1, 3, 3).copy()
    w[:] = w[0]
    return _with_vertices(sc, w)


def clusters():
    """three clusters, each ~2 mm across, far apart (tests/test_gpu_build.py): most bins of the top splits are empty"""
    sc = scenes.soup(6000, 32, 24, seed=31, hdri_size=(32, 16))
    v = sc.vertices.reshape(-1, 3, 3).copy()
    c = v.mean(1, keepdims=True)
    cluster = (np.arange(len(v)) % 3)[:, None, None]
    centre = np.array([[-0.9, 0.3, 2.2], [0.8, -0.4, 3.6], [0.1, 0.7, 2.9]], np.float32)[cluster[:, 0, 0]][:, None, :]
    return _with_vertices(sc, centre + (v - c) * 0.2 + (c - c.mean(0)) * 1e-3)


TRANSLATION = np.array([40.0, -25.0, 60.0], np.float32)


def translated_soup(n=6000, seed=13):
    """coordinates ~60, extent ~2: the absolute term of the box padding (1e-6 x the largest coordinate) decides everywhere"""
    sc = small_soup(n, seed)
    return _with_vertices(sc, sc.vertices.reshape(-1, 3, 3) + TRANSLATION)


def flat_grid(g=37):
    """a quad in the plane z = 3 cut into g x g cells of two triangles: the boxes' z extent is twice the padding and nothing else"""
    t = np.linspace(-1.0, 1.0, g + 1).astype(np.float32)
    x0, y0 = np.meshgrid(t[:-1], t[:-1], indexing="ij")
    x1, y1 = np.meshgrid(t[1:], t[1:], indexing="ij")
    z = np.full_like(x0, 3.0)
    p00, p10, p11, p01 = (np.stack(q, -1).reshape(-1, 3) for q in ((x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)))
    v = np.concatenate([np.stack([p00, p10, p11], 1), np.stack([p00, p11, p01], 1)]).astype(np.float32)
    normals, tangents = scenes.face_frame(v)
    n = len(v)
    uvs = np.tile(np.array([[0, 0], [1, 0], [0, 1]], np.float32), (n, 1, 1))
    cam = abi.default_camera()
    cam.position = abi.ErVec3(0.01, 0.02, -0.5)
    return abi.SceneData(v, normals, tangents, uvs, np.ones(n, np.float32), np.zeros(n, np.int32), [abi.default_material()],
                         hdri=scenes.sky_hdri(32, 16), camera=cam, x_res=32, y_res=24)


def varied_soup(n):
    """per-triangle uvs and tangent signs (tests/uv_scenes.py): r_attr and r_sign can tell one triangle's record from another's"""
    return uv_scenes.varied(small_soup(n), 29)


def empty_scene():
    return abi.SceneData(None, None, None, None, None, None, [abi.default_material()], x_res=8, y_res=8)


SPECIAL = {"cornell": lambda: scenes.cornell(32, 24), "same-centroid": same_centroid, "duplicates": duplicates, "clusters": clusters,
           "translated": translated_soup, "flat-grid": flat_grid, "varied-257": lambda: varied_soup(257), "varied-6000": lambda: varied_soup(6000)}


def host_dump(sc, threads=0):
    return accel_check.host_records(sc, abi.debug_bvh_dump(sc.vertices, sc.normals, threads))


@pytest.mark.parametrize("case", [0, 1, 2, 3, 5, 257, 1000, 20001] + list(SPECIAL))
def test_host_built_structure_checks_clean(case):
    sc = empty_scene() if case == 0 else small_soup(case) if isinstance(case, int) else SPECIAL[case]()
    d = host_dump(sc)
    rep = accel_check.check(sc, d)
    print(f"{case}: {sc.tri_count} triangles, {d['node_count']} binary nodes (depth {rep.depth2}), {d['node8_count']} wide nodes (depth {rep.depth8})")
    assert d["tri_count"] == sc.tri_count and len(d["nodes8"]) == d["node8_count"] and len(d["nodes"]) == d["node_count"]
    assert rep.ok, rep.message()


def test_host_build_does_not_depend_on_the_thread_count():
    sc = small_soup(20001)
    a, b = abi.debug_bvh_dump(sc.vertices, sc.normals, 1), abi.debug_bvh_dump(sc.vertices, sc.normals, 8)
    for k in ("nodes", "nodes8", "slot_to_tri", "tri_lift"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_dump_size_query_and_short_buffers():
    import ctypes as C
    lib = abi.load()
    sc = small_soup(5)
    info = abi.ErAccelDump()
    args = (abi._fptr(sc.vertices), abi._fptr(sc.normals), 5, 1, C.byref(info))
    assert lib.er_debug_bvh_dump(*args, None, 0, None, 0, None, 0, None, 0) == abi.ER_OK
    assert info.tri_count == 5 and info.node_count >= 1 and info.node8_count >= 1 and info.node8_pieces == 5 and info.attr_pieces == 0
    buf = np.zeros(info.node_count * 64, np.uint8)
    assert lib.er_debug_bvh_dump(*args, buf.ctypes.data_as(C.c_void_p), buf.nbytes - 1, None, 0, None, 0, None, 0) == abi.ER_ERR_INVALID_ARG
    assert lib.er_debug_bvh_dump(*args, buf.ctypes.data_as(C.c_void_p), buf.nbytes, None, 0, None, 0, None, 0) == abi.ER_OK
    assert buf.any()


# ---- the checker must be able to fail ----

@pytest.fixture(scope="module")
def intact():
    sc = scenes.soup(1000, 32, 24, hdri_size=(32, 16))          # soup_geometry(1000)
    d = host_dump(sc)
    rep = accel_check.check(sc, d)
    assert rep.ok, rep.message()
    return sc, d, rep


def _cut_search(d, rep, side):
    """a (node, slot, axis) whose decoded plane, moved inward by one quantisation step, cuts a padded box beneath it"""
    n8 = d["nodes8"].copy()
    if side == "qhi":
        n8["qhi"] = np.maximum(n8["qhi"].astype(np.int32) - 1, 0).astype(np.uint8)
        moved = accel_check.decode_wide_boxes(n8)[1].astype(np.float64).transpose(0, 2, 1) < rep.slot_req_hi
        moved &= (d["nodes8"]["qhi"] > 0).transpose(0, 2, 1)
    else:
        n8["qlo"] = np.minimum(n8["qlo"].astype(np.int32) + 1, 255).astype(np.uint8)
        moved = accel_check.decode_wide_boxes(n8)[0].astype(np.float64).transpose(0, 2, 1) > rep.slot_req_lo
        moved &= (d["nodes8"]["qlo"] < 255).transpose(0, 2, 1)
    hits = np.argwhere(moved)
    assert len(hits), "no slot is within one step of its contents"
    return tuple(int(x) for x in hits[len(hits) // 2])


def _leaf_slot(n8):
    i = int(np.nonzero(n8["tri_present"])[0][0])
    s = int(np.nonzero([(int(n8["tri_present"][i]) >> (2 * k)) & 1 for k in range(8)])[0][0])
    return i, s


def c_qhi(d, rep):
    i, s, a = _cut_search(d, rep, "qhi")
    d["nodes8"]["qhi"][i, a, s] -= 1


def c_qlo(d, rep):
    i, s, a = _cut_search(d, rep, "qlo")
    d["nodes8"]["qlo"][i, a, s] += 1


def c_exponent(d, rep):
    d["nodes8"]["e"][0, 0] -= 1


def c_tri_present(d, rep):
    i, s = _leaf_slot(d["nodes8"])
    d["nodes8"]["tri_present"][i] &= ~np.uint32(1 << (2 * s))


def c_imask(d, rep):
    i, s = _leaf_slot(d["nodes8"])
    d["nodes8"]["imask"][i] |= np.uint8(1 << s)


def c_child_base(d, rep):
    i = int(np.nonzero(d["nodes8"]["imask"])[0][-1])
    d["nodes8"]["child_base"][i] += 1


def c_swap(d, rep):
    ids = d["isect"]["tri_id"]
    n = d["tri_count"]
    ids[0], ids[n - 1] = ids[n - 1], ids[0]          # the first and the last slot lie in different leaves


def c_duplicate(d, rep):
    d["isect"]["tri_id"][7] = d["isect"]["tri_id"][400]


def c_leaf_ref(d, rep):
    i = int(np.nonzero(d["nodes"]["c0"] < 0)[0][0])
    code = ~int(d["nodes"]["c0"][i])
    d["nodes"]["c0"][i] = ~((((code >> 3) + 1) << 3) | (code & 7))


def c_sentinel(d, rep):
    d["isect"][d["tri_count"]:].view(np.uint8)[13] = 1


CORRUPTIONS = [(c_qhi, "w_box"), (c_qlo, "w_box"), (c_exponent, "w_box"), (c_tri_present, "w_tri_partition"), (c_imask, "w_inner_tri_bits"),
               (c_child_base, "w_parent"), (c_swap, "r_vertices"), (c_duplicate, "r_perm"), (c_leaf_ref, "b_leaf_partition"), (c_sentinel, "r_sentinel")]


@pytest.mark.parametrize("corrupt,name", CORRUPTIONS, ids=[c.__name__[2:] for c, _ in CORRUPTIONS])
def test_checker_reports_a_corruption(intact, corrupt, name):
    sc, d, rep = intact
    saved = {k: d[k].copy() for k in ("nodes", "nodes8", "isect", "attr")}
    try:
        corrupt(d, rep)
        assert any(d[k].tobytes() != saved[k].tobytes() for k in saved), "the corruption changed nothing"
        got = accel_check.check(sc, d)
        print(corrupt.__name__, got.failed())
        assert got.counts[name] > 0, (name, got.message())
    finally:
        for k in saved:
            d[k][...] = saved[k]
    again = accel_check.check(sc, d)
    assert again.ok, again.message()
