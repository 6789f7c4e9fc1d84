"""er_skin_set / er_render_skin / er_skin_info on a machine without a GPU: the symbols, the layouts of their structs against the C
compiler's, the host form of the arithmetic (er_debug_skin_apply, csrc/er_skin.h) against its numpy restatement (elevenrender_amd/skin.py)
bit for bit, every refusal of er_skin_set on a created scene, the call-order errors that need no device, and the host half of the calls
-- checks, the bound on linear entries, mark and the lazy application of both kinds of pending pose -- as a stand-alone program under
ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from elevenrender_amd import abi, render, scenes, skin, transform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
HP = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))
FP = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))


def test_library_exports_the_skin_entry_points():
    lib = abi.load()
    for name in ("er_skin_set", "er_render_skin", "er_skin_info"):
        assert hasattr(lib, name) and name in abi.SYMBOLS
    assert hasattr(lib, "er_debug_skin_apply")
    assert lib.er_abi_version() == 2          # an addition: nothing existing changed layout


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eleven_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %u\\n", sizeof(ErSkin), offsetof(ErSkin, bones), offsetof(ErSkin, weights),\n'
                   '  sizeof(ErSkinPose), offsetof(ErSkinPose, bone_count), offsetof(ErSkinPose, palette),\n'
                   '  sizeof(ErSkinUpdate), offsetof(ErSkinUpdate, camera), offsetof(ErSkinUpdate, count), offsetof(ErSkinUpdate, poses),\n'
                   '  sizeof(ErSkinInfo), offsetof(ErSkinInfo, bones), offsetof(ErSkinInfo, why_full), offsetof(ErSkinInfo, refit_ms),\n'
                   '  offsetof(ErSkinInfo, bytes_uploaded), offsetof(ErSkinInfo, influence_bytes), ER_SKIN_INFLUENCES, ER_SKIN_MAX_BONES); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    K, P, U, I = abi.ErSkin, abi.ErSkinPose, abi.ErSkinUpdate, abi.ErSkinInfo
    assert got == [C.sizeof(K), K.bones.offset, K.weights.offset, C.sizeof(P), P.bone_count.offset, P.palette.offset,
                   C.sizeof(U), U.camera.offset, U.count.offset, U.poses.offset,
                   C.sizeof(I), I.bones.offset, I.why_full.offset, I.refit_ms.offset, I.bytes_uploaded.offset, I.influence_bytes.offset,
                   skin.INFLUENCES, skin.MAX_BONES]
    assert C.sizeof(I) == 56


# ---- the arithmetic ----

def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def seeded_palette(bones, seed):
    """rotation x non-uniform scale x translation per bone"""
    rng = np.random.default_rng(seed)
    P = np.empty((bones, 3, 4), np.float32)
    for b in range(bones):
        L = rotation(rng.normal(size=3), rng.uniform(0.1, 3.0)) @ np.diag(rng.uniform(0.3, 2.5, size=3))
        P[b] = np.concatenate([L, rng.normal(size=(3, 1)) * 2], 1)
    return P


def seeded_case(seed, bones=7, count=600):
    """`count` seeded triangles whose corners have exactly 1, 2, 3 and 4 non-zero weights in turn; the weights of every second triangle
    do not sum to 1; the awkward rest data in front: normals that are not unit, a zero normal, a zero tangent"""
    rng = np.random.default_rng(seed)
    v = (rng.normal(size=(count, 3, 3)) * 4).astype(np.float32)
    n = rng.normal(size=(count, 3, 3)).astype(np.float32)      # (not unit)
    t = rng.normal(size=(count, 3, 3)).astype(np.float32)
    n[0], t[1] = 0, 0
    n[2] = (n[2] * np.float32(1e3)).astype(np.float32)
    b = rng.integers(0, bones, size=(count, 3, 4)).astype(np.uint16)
    w = rng.uniform(0.05, 1.0, size=(count, 3, 4))
    nonzero = (np.arange(count * 3).reshape(count, 3) % 4) + 1
    w[np.arange(4)[None, None, :] >= nonzero[:, :, None]] = 0
    w /= w.sum(-1, keepdims=True)
    w[1::2] *= rng.uniform(0.3, 0.9, size=(len(w[1::2]), 3, 1))
    w = w.astype(np.float32)
    assert sorted(set(((w != 0).sum(-1)).reshape(-1).tolist())) == [1, 2, 3, 4]
    assert (np.abs(w[1::2].astype(np.float64).sum(-1) - 1) > 0.05).all() and w.min() >= 0 and w.max() <= 1
    assert (np.abs(np.linalg.norm(n[3:].astype(np.float64), axis=-1) - 1) > 1e-3).mean() > 0.99
    return seeded_palette(bones, seed + 100), b, w, v, n, t


def same_bits(a, b):
    """bit for bit, NaN matching NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_form_equals_the_numpy_restatement_bit_for_bit(seed):
    P, b, w, v, n, t = seeded_case(seed)
    got = abi.debug_skin_apply(P, b, w, v, n, t)
    want = skin.pose(P, b, w, v, n, t)
    for what, x, y in zip(("vertices", "normals", "tangents"), got, want):
        assert same_bits(x, y), (what, int((x.view(np.uint32) != y.view(np.uint32)).sum()))
    pv, pn, pt = got
    assert (pn[0] == 0).all() and (pt[1] == 0).all()                       # zero directions stay zero
    lengths = np.linalg.norm(pn[3:].astype(np.float64), axis=-1)
    assert np.abs(lengths - 1).max() < 1e-6                                # directions come out unit
    assert (pv.view(np.uint32) != v.view(np.uint32)).any(-1).mean() > 0.9  # (and the palette moves the corners)
    # the cofactor path is not the linear one: under non-uniform scales, normals posed as tangents differ
    assert not same_bits(pn, abi.debug_skin_apply(P, b, w, v, t, n)[2])
    # one bone with weight 1 is that bone's matrix: the position equals the transform's (its directions are scaled first and may differ)
    one = np.zeros_like(w)
    one[..., 2] = 1
    for k in range(len(P)):
        pv1 = abi.debug_skin_apply(P, np.full_like(b, k), one, v, n, t)[0]
        assert same_bits(pv1, transform.pose(P[k], v, n, t)[0])


def test_identities_with_one_weight_of_one_reproduce_the_rest_vertices():
    _, b, w, v, n, t = seeded_case(9)
    P = np.tile(np.eye(3, 4, dtype=np.float32), (7, 1, 1))
    for slot in range(4):
        one = np.zeros_like(w)
        one[..., slot] = 1
        for pv, _, _ in (abi.debug_skin_apply(P, b, one, v, n, t), skin.pose(P, b, one, v, n, t)):
            assert same_bits(pv, v), slot


def test_refused_influences_are_refused_by_the_host_form():
    P, b, w, v, n, t = seeded_case(4, count=8)
    lib = abi.load()
    out = [np.empty_like(v) for _ in range(3)]

    def call(P=P, bones=b, weights=w, bone_count=None):
        return lib.er_debug_skin_apply(FP(np.ascontiguousarray(P)), len(P) if bone_count is None else bone_count, len(v), HP(np.ascontiguousarray(bones)),
                                       FP(np.ascontiguousarray(weights)), FP(v), FP(n), FP(t), *(FP(o) for o in out))

    assert call() == abi.ER_OK
    bad_b, nan, neg, big = b.copy(), w.copy(), w.copy(), w.copy()
    bad_b[7, 2, 3] = len(P)
    nan[0, 0, 0], neg[3, 1, 2], big[7, 2, 3] = np.nan, -1e-3, np.nextafter(np.float32(1), np.float32(2))
    for what, rc in {"a bone index equal to bone_count": call(bones=bad_b), "a NaN weight": call(weights=nan), "a negative weight": call(weights=neg),
                     "a weight above 1": call(weights=big), "bone_count 0": call(bone_count=0), "bone_count above the maximum": call(bone_count=skin.MAX_BONES + 1)}.items():
        assert rc == abi.ER_ERR_INVALID_ARG, what
    assert lib.er_debug_skin_apply(None, 1, 0, None, None, None, None, None, None, None, None) == abi.ER_ERR_INVALID_ARG


def test_palette_checks_of_the_restatement():
    B = np.array([2.0, 3.0, 5.0])
    P = seeded_palette(4, 1)
    assert skin.palette_ok(P, B)
    for k, (i, j, x) in enumerate([(0, 0, np.nan), (1, 3, np.inf), (2, 3, 2e37), (2, 1, 2 * skin.MAX_LINEAR)]):
        Q = P.copy()
        Q[k, i, j] = x
        assert not skin.palette_ok(Q, B), (k, i, j, x)
    mirror = P.copy()
    mirror[2, :, 0] *= -1
    assert not skin.palette_ok(mirror, B)
    at = np.tile(np.eye(3, 4, dtype=np.float32), (1, 1, 1)) * np.float32(skin.MAX_LINEAR)
    assert skin.palette_ok(at, np.zeros(3)) and not skin.palette_ok(at * np.float32(1.0001), np.zeros(3))


# ---- the calls that need no device ----

def created(sc):
    h = C.c_void_p()
    abi.check(abi.load().er_scene_create(C.byref(sc.desc()), C.byref(h)))
    return h


def skin_info(h):
    info = abi.ErSkinInfo()
    abi.check(abi.load().er_skin_info(h, C.byref(info)))
    return {n: getattr(info, n) for n, _ in abi.ErSkinInfo._fields_}


def test_every_refusal_of_skin_set_on_a_created_scene():
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    assert sc.tri_count >= 8
    h = created(sc)
    try:
        def call(obj, bone_count, bones, weights):
            k = abi.ErSkin()
            k.object, k.bone_count = obj, bone_count
            keep = []
            if bones is not None:
                keep.append(np.ascontiguousarray(bones, np.uint16))
                k.bones = HP(keep[-1])
            if weights is not None:
                keep.append(np.ascontiguousarray(weights, np.float32))
                k.weights = FP(keep[-1])
            return lib.er_skin_set(h, C.byref(k))

        b3 = np.array([0, 1, 2, 1] * 9, np.uint16).reshape(3, 3, 4)
        w3 = np.tile(np.array([0.5, 0.25, 0.25, 0.0], np.float32), (3, 3, 1))
        assert call(0, 3, b3[:2], w3[:2]) == abi.ER_ERR_STATE                     # no object table yet
        assert b"er_objects_set" in lib.er_last_error()
        assert lib.er_objects_set(h, 3, UP(np.array([0, 2, 5, 5], np.uint32)), UP(np.array([4, 1, 0, 7, 2], np.uint32))) == abi.ER_OK
        assert skin_info(h)["skinned"] == 0
        assert call(1, 3, b3, w3) == abi.ER_OK
        assert skin_info(h)["skinned"] == 1

        def edited(a, at, x):
            a = a.copy()
            a[at] = x
            return a

        refused = {"a NULL scene": lib.er_skin_set(None, C.byref(abi.ErSkin())),
                   "a NULL skin": lib.er_skin_set(h, None),
                   "NULL bones": call(1, 3, None, w3),
                   "NULL weights": call(1, 3, b3, None),
                   "an object index equal to the object count": call(3, 3, b3, w3),
                   "an empty object": call(2, 3, b3, w3),
                   "an empty object, removal": call(2, 0, None, None),
                   "bone_count above the maximum": call(1, skin.MAX_BONES + 1, b3, w3),
                   "a bone index equal to bone_count": call(1, 3, edited(b3, (2, 2, 3), 3), w3),
                   "a bone index out of range under a weight of 0": call(1, 2, edited(np.minimum(b3, 1), (0, 1, 3), 2), w3),
                   "a NaN weight": call(1, 3, b3, edited(w3, (1, 0, 1), np.nan)),
                   "an infinite weight": call(1, 3, b3, edited(w3, (2, 2, 3), np.inf)),
                   "a negative weight": call(1, 3, b3, edited(w3, (0, 0, 0), -0.5)),
                   "a weight above 1": call(1, 3, b3, edited(w3, (0, 0, 0), np.nextafter(np.float32(1), np.float32(2))))}
        for what, rc in refused.items():
            assert rc == abi.ER_ERR_INVALID_ARG, what
            assert skin_info(h)["skinned"] == 1, what                              # the skin set before is still there
        assert b"er_skin_set" in lib.er_last_error()
        # legal: the maximum bone count, weights that do not sum to 1 (w3 with a zeroed entry), a second skin, a replacement, a removal
        assert call(1, skin.MAX_BONES, b3, edited(w3, (0, 0, 0), 0.0)) == abi.ER_OK
        assert call(0, 3, b3[:2], w3[:2]) == abi.ER_OK
        assert skin_info(h)["skinned"] == 2
        assert call(1, 0, None, None) == abi.ER_OK
        assert skin_info(h)["skinned"] == 1
        assert call(1, 0, None, None) == abi.ER_OK                                 # removing what is not there
        # a new table drops every skin
        assert lib.er_objects_set(h, 1, UP(np.array([0, 2], np.uint32)), UP(np.array([3, 1], np.uint32))) == abi.ER_OK
        assert skin_info(h)["skinned"] == 0
        assert call(0, 3, b3[:2], w3[:2]) == abi.ER_OK
        assert lib.er_objects_set(h, 0, None, None) == abi.ER_OK
        assert skin_info(h)["skinned"] == 0 and call(0, 3, b3[:2], w3[:2]) == abi.ER_ERR_STATE
    finally:
        lib.er_scene_destroy(h)


def test_skin_needs_a_begun_scene_and_arguments():
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    h = created(sc)
    try:
        P = np.eye(3, 4, dtype=np.float32).reshape(1, 12).copy()
        p = (abi.ErSkinPose * 1)()
        p[0].object, p[0].bone_count, p[0].palette = 0, 1, FP(P)
        u = abi.ErSkinUpdate()
        u.what, u.count, u.poses = abi.UPDATE_GEOMETRY, 1, p
        assert lib.er_render_skin(None, C.byref(u)) == abi.ER_ERR_INVALID_ARG
        assert lib.er_render_skin(h, None) == abi.ER_ERR_INVALID_ARG
        assert b"NULL" in lib.er_last_error()
        assert lib.er_render_skin(h, C.byref(u)) == abi.ER_ERR_STATE              # created, not begun
        assert b"er_render_begin" in lib.er_last_error()
        info = abi.ErSkinInfo(*([7] * 9), 7.0, 7, 7)
        assert lib.er_skin_info(h, None) == abi.ER_ERR_INVALID_ARG and lib.er_skin_info(None, C.byref(info)) == abi.ER_ERR_INVALID_ARG
        assert lib.er_skin_info(h, C.byref(info)) == abi.ER_OK                     # counts since er_scene_create: valid before a begin
        assert [getattr(info, n) for n, _ in abi.ErSkinInfo._fields_] == [0] * 9 + [0.0, 0, 0]
    finally:
        lib.er_scene_destroy(h)


def test_python_binding_checks_its_arguments():
    rm = render.RenderingManager()
    rm.scene = scenes.cornell(16, 16)
    b, w = np.zeros((2, 3, 4), np.int64), np.zeros((2, 3, 4), np.float32)
    for args in ((-1, b, w), (0, b.astype(np.float32), w), (0, b[:, :, :3], w[:, :, :3]), (0, b, w[:1]), (0, b - 1, w), (0, b + 0x10000, w)):
        with pytest.raises(ValueError):      # (before the library is reached: this manager has no handle)
            rm.set_skin(*args)
    with pytest.raises(ValueError) as e:
        rm.skin({0: np.eye(4, dtype=np.float32)})
    assert "3x4" in str(e.value)
    with pytest.raises(ValueError):
        rm.skin({-1: np.eye(3, 4, dtype=np.float32)})


def test_host_half_under_sanitizers(tmp_path):
    """tests/native/skin_host.cpp: er_skin.h alone -- the skin's and the list's checks, the bound on linear entries, mark and the lazy
    application of both pending kinds, the drop on a table change -- with ASan + UBSan, on heap arrays of exactly the sizes the contract names"""
    exe = str(tmp_path / "skin_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "elevenrender_amd", "csrc"), os.path.join(ROOT, "tests", "native", "skin_host.cpp"), "-o", exe])
    out = subprocess.run([exe], text=True, capture_output=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "skin_host ok" in out.stdout
