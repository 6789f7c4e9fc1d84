"""er_objects_set / er_render_transform / er_transform_info on a machine without a GPU: the symbols, the layouts of their structs against
the C compiler's, every refusal of er_objects_set on a created scene, the call-order errors that need no device, the host form of the
arithmetic (er_debug_transform_apply, csrc/er_xform.h) against its numpy restatement (elevenrender_amd/transform.py) bit for bit, the
overflow bound, and the host half of the calls -- checks, matrix derivation, the lazy application of pending poses -- as a stand-alone
program under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from elevenrender_amd import abi, render, scenes, transform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))


def test_library_exports_the_transform_entry_points():
    lib = abi.load()
    for name in ("er_objects_set", "er_render_transform", "er_transform_info"):
        assert hasattr(lib, name) and name in abi.SYMBOLS
    assert hasattr(lib, "er_debug_transform_apply")
    assert lib.er_abi_version() == 2          # an addition: nothing existing changed layout


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eleven_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ErObjectTransform), offsetof(ErObjectTransform, m),\n'
                   '  sizeof(ErTransformUpdate), offsetof(ErTransformUpdate, camera), offsetof(ErTransformUpdate, count), offsetof(ErTransformUpdate, transforms),\n'
                   '  sizeof(ErTransformInfo), offsetof(ErTransformInfo, objects), offsetof(ErTransformInfo, moved), offsetof(ErTransformInfo, path),\n'
                   '  offsetof(ErTransformInfo, why_full), offsetof(ErTransformInfo, dirty_nodes8), offsetof(ErTransformInfo, bytes_uploaded),\n'
                   '  offsetof(ErTransformInfo, refit_ms)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    X, U, I = abi.ErObjectTransform, abi.ErTransformUpdate, abi.ErTransformInfo
    assert got == [C.sizeof(X), X.m.offset, C.sizeof(U), U.camera.offset, U.count.offset, U.transforms.offset,
                   C.sizeof(I), I.objects.offset, I.moved.offset, I.path.offset, I.why_full.offset, I.dirty_nodes8.offset, I.bytes_uploaded.offset, I.refit_ms.offset]
    assert C.sizeof(X) == 52


def created(sc):
    h = C.c_void_p()
    abi.check(abi.load().er_scene_create(C.byref(sc.desc()), C.byref(h)))
    return h


def test_every_refusal_of_objects_set_on_a_created_scene():
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    n = sc.tri_count
    assert n >= 8
    h = created(sc)
    try:
        def call(first, ids, count=None):
            first, ids = np.asarray(first, np.uint32), np.asarray(ids, np.uint32)
            return lib.er_objects_set(h, len(first) - 1 if count is None else count, UP(first), UP(ids))

        assert call([0, 2, 5], [4, 1, 0, 7, 2]) == abi.ER_OK
        refused = {"first does not start at 0": call([1, 2, 5], [4, 1, 0, 7, 2]),
                   "first decreases": call([0, 3, 2], [4, 1, 0]),
                   "an id equal to tri_count": call([0, 2, 5], [4, 1, 0, n, 2]),
                   "an id far beyond": call([0, 2], [0xffffffff, 1]),
                   "an id in two objects": call([0, 2, 5], [4, 1, 0, 4, 2]),
                   "an id twice in one object": call([0, 2, 5], [4, 1, 0, 7, 7]),
                   "more ids than triangles": call([0, n + 1], list(range(n)) + [0]),
                   "a NULL scene": lib.er_objects_set(None, 1, UP(np.array([0, 1], np.uint32)), UP(np.array([0], np.uint32))),
                   "NULL first": lib.er_objects_set(h, 1, None, UP(np.array([0], np.uint32))),
                   "NULL tri_ids": lib.er_objects_set(h, 1, UP(np.array([0, 1], np.uint32)), None)}
        for what, rc in refused.items():
            assert rc == abi.ER_ERR_INVALID_ARG, what
        assert b"er_objects_set" in lib.er_last_error()
        # legal: triangles in no object, an empty object, a table replaced, a table cleared (nothing is read then)
        assert call([0, 0, 1], [3]) == abi.ER_OK
        assert call([0, n], list(range(n))[::-1]) == abi.ER_OK
        assert lib.er_objects_set(h, 0, None, None) == abi.ER_OK
    finally:
        lib.er_scene_destroy(h)


def test_transform_needs_a_begun_scene_and_arguments():
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    h = created(sc)
    try:
        assert lib.er_objects_set(h, 1, UP(np.array([0, 2], np.uint32)), UP(np.array([3, 1], np.uint32))) == abi.ER_OK
        x = (abi.ErObjectTransform * 1)()
        x[0].object = 0
        x[0].m[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
        u = abi.ErTransformUpdate()
        u.what, u.count, u.transforms = abi.UPDATE_GEOMETRY, 1, x
        assert lib.er_render_transform(None, C.byref(u)) == abi.ER_ERR_INVALID_ARG
        assert lib.er_render_transform(h, None) == abi.ER_ERR_INVALID_ARG
        assert b"NULL" in lib.er_last_error()
        assert lib.er_render_transform(h, C.byref(u)) == abi.ER_ERR_STATE          # created, not begun
        assert b"er_render_begin" in lib.er_last_error()
        info = abi.ErTransformInfo(7, 7, 7, 7, 7, 7, 7, 7, 7, 7.0)
        assert lib.er_transform_info(h, None) == abi.ER_ERR_INVALID_ARG and lib.er_transform_info(None, C.byref(info)) == abi.ER_ERR_INVALID_ARG
        assert lib.er_transform_info(h, C.byref(info)) == abi.ER_OK                # counts since er_scene_create: valid before a begin
        assert [getattr(info, n) for n, _ in abi.ErTransformInfo._fields_] == [0] * 9 + [0.0]
    finally:
        lib.er_scene_destroy(h)


def test_python_binding_checks_its_arguments():
    rm = render.RenderingManager()
    rm.scene = scenes.cornell(16, 16)
    for objects in ([[[0, 1]]], [[0.5, 1.0]], [[0, -1]]):
        with pytest.raises(ValueError):      # (before the library is reached: this manager has no handle)
            rm.set_objects(objects)
    with pytest.raises(ValueError) as e:
        rm.transform({0: np.eye(4, dtype=np.float32)})
    assert "3x4" in str(e.value)
    with pytest.raises(ValueError):
        rm.transform({-1: np.eye(3, 4, dtype=np.float32)})


# ---- the arithmetic ----

def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def matrix(L, t=(0, 0, 0)):
    return np.concatenate([np.asarray(L, np.float64), np.asarray(t, np.float64)[:, None]], 1).astype(np.float32)


MATRICES = {
    "identity": matrix(np.eye(3)),
    "translation": matrix(np.eye(3), (1.25, -300.0, 0.001)),
    "rotation about (1, 2, 3) by 0.7345": matrix(rotation((1, 2, 3), 0.7345), (0.1, 2.0, 3.0)),
    "rotation about (-0.3, 0.11, 5) by 3.1": matrix(rotation((-0.3, 0.11, 5), 3.1)),
    "rotation about (7, -1, 0.01) by 1e-4": matrix(rotation((7, -1, 0.01), 1e-4), (-4.0, 0.0, 9.5)),
    "non-uniform scale": matrix(np.diag([1.0, 2.5, 0.3])),
    "shear": matrix([[1, 0.3, 0], [0, 1, 0.7], [0, 0, 1]], (0, 1, 0)),
    "rotation x non-uniform scale": matrix(rotation((2, -1, 0.5), 2.2) @ np.diag([3.0, 0.25, 1.7]), (5, 6, 7)),
    "uniform scale 1e-20": matrix(np.eye(3) * 1e-20),
    "uniform scale 1e15": matrix(np.eye(3) * 1e15),
}


def seeded_triangles():
    """1 000 seeded triangles with the awkward ones in front: zero normals and tangents, denormal coordinates, a rest normal of length
    1e20, a tangent of length 1e-30"""
    rng = np.random.default_rng(20)
    v = (rng.normal(size=(1000, 3, 3)) * 4).astype(np.float32)
    n = rng.normal(size=(1000, 3, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    t = rng.normal(size=(1000, 3, 3)).astype(np.float32)
    n[0], t[1] = 0, 0
    v[2] = (v[2] * np.float32(1e-40)).astype(np.float32)
    v[3, 1] = np.float32(1e-45)
    n[4] = (n[4] * np.float32(1e20)).astype(np.float32)
    t[5] = (t[5] * np.float32(1e-30)).astype(np.float32)
    assert (v[2] != 0).any() and (np.abs(v[2]) < np.finfo(np.float32).tiny).all()
    return v, n.astype(np.float32), t


def same_bits(a, b):
    """bit for bit, NaN matching NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("name", list(MATRICES))
def test_host_form_equals_the_numpy_restatement_bit_for_bit(name):
    m = MATRICES[name]
    v, n, t = seeded_triangles()
    got = abi.debug_transform_apply(m, v, n, t)
    want = transform.pose(m, v, n, t)
    for what, a, b in zip(("vertices", "normals", "tangents"), got, want):
        assert same_bits(a, b), (name, what, int((a.view(np.uint32) != b.view(np.uint32)).sum()))
    pv, pn, pt = got
    assert (pn[0] == 0).all() and (pt[1] == 0).all()                       # zero directions stay zero
    lengths = np.linalg.norm(pn[6:].astype(np.float64), axis=-1)
    assert np.abs(lengths - 1).max() < 1e-6                                # directions come out unit
    if name == "identity":
        assert same_bits(pv, v)                                            # pose(rest, identity) reproduces the vertices
    if name == "translation":
        assert same_bits(pn, abi.debug_transform_apply(MATRICES["identity"], v, n, t)[1])      # a translation does not turn a direction


def test_refused_matrices_are_refused_by_both_forms():
    v, n, t = seeded_triangles()
    nan, inf = matrix(np.eye(3)), matrix(np.eye(3))
    nan[1, 2], inf[2, 3] = np.nan, np.inf
    for what, m in (("a mirror", matrix(np.diag([1.0, -1.0, 1.0]))), ("singular", matrix([[1, 2, 3], [2, 4, 6], [0, 0, 1]])), ("zero", matrix(np.zeros((3, 3)))),
                    ("a NaN", nan), ("an infinite translation", inf)):
        out = [np.empty_like(v) for _ in range(3)]
        rc = abi.load().er_debug_transform_apply(abi._fptr(np.ascontiguousarray(m.reshape(12))), len(v), abi._fptr(v), abi._fptr(n), abi._fptr(t), *(abi._fptr(o) for o in out))
        assert rc == abi.ER_ERR_INVALID_ARG, what
        with pytest.raises(ValueError):
            transform.matrices(m)
    assert abi.load().er_debug_transform_apply(None, 0, None, None, None, None, None, None) == abi.ER_ERR_INVALID_ARG


def test_overflow_bound_refuses_just_beyond_and_accepts_just_inside():
    """B = the object's largest rest |coordinate| per axis; a row may reach 1e37 and no further.  The matrix just inside poses every vertex
    to a finite float."""
    rng = np.random.default_rng(4)
    v = (rng.uniform(-1, 1, size=(1000, 3, 3)) * np.array([2.0, 3.0, 5.0])).astype(np.float32)
    v[17, 0] = (2.0, -3.0, 5.0)
    n = np.zeros_like(v)
    B = np.abs(v).reshape(-1, 3).max(0)
    assert B.tolist() == [2.0, 3.0, 5.0]
    inside = matrix(np.diag([0.49e37, 1.0, 1.0]), (0.01e37, 0.0, 0.0))
    beyond = matrix(np.diag([0.49e37, 1.0, 1.0]), (0.03e37, 0.0, 0.0))
    assert transform.bound_ok(inside, B) and not transform.bound_ok(beyond, B)
    assert not transform.bound_ok(matrix(np.diag([0.49e37, 1.0, 1.0]), (-0.03e37, 0.0, 0.0)), B)
    pv, _, _ = abi.debug_transform_apply(inside, v, n, n)
    assert np.isfinite(pv).all() and np.abs(pv).max() > 0.9e37
    assert same_bits(pv, transform.pose(inside, v, n, n)[0])


def test_host_half_under_sanitizers(tmp_path):
    """tests/native/xform_host.cpp: er_xform.h alone -- the table's and the list's checks, the matrix derivation, the bound, mark and the lazy
    application -- with ASan + UBSan, on heap arrays of exactly the sizes the contract names"""
    exe = str(tmp_path / "xform_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "elevenrender_amd", "csrc"), os.path.join(ROOT, "tests", "native", "xform_host.cpp"), "-o", exe])
    out = subprocess.run([exe], text=True, capture_output=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "xform_host ok" in out.stdout
