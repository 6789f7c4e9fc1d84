"""er_render_update_sparse / er_sparse_info on a machine without a GPU: the symbols, the layouts of their structs against the C
compiler's, the call-order and argument errors that need no device, the Python binding's own shape checks, and the host half of the call
(csrc/er_sparse_host.h: id validation, duplicate detection, the patch of the host copy) as a stand-alone program under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from elevenrender_amd import abi, render, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_sparse_entry_points():
    lib = abi.load()
    for name in ("er_render_update_sparse", "er_sparse_info"):
        assert hasattr(lib, name) and name in abi.SYMBOLS
    assert lib.er_abi_version() == 2          # an addition: nothing existing changed layout


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "eleven_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ErSparseUpdate), offsetof(ErSparseUpdate, camera),\n'
                   '  offsetof(ErSparseUpdate, count), offsetof(ErSparseUpdate, tri_ids), offsetof(ErSparseUpdate, vertices), offsetof(ErSparseUpdate, tangents),\n'
                   '  sizeof(ErSparseInfo), offsetof(ErSparseInfo, dirty_nodes8), offsetof(ErSparseInfo, bytes_uploaded), offsetof(ErSparseInfo, refit_ms)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    U, I = abi.ErSparseUpdate, abi.ErSparseInfo
    assert got == [C.sizeof(U), U.camera.offset, U.count.offset, U.tri_ids.offset, U.vertices.offset, U.tangents.offset,
                   C.sizeof(I), I.dirty_nodes8.offset, I.bytes_uploaded.offset, I.refit_ms.offset]


def test_sparse_update_needs_a_begun_scene_and_arguments():
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    h = C.c_void_p()
    abi.check(lib.er_scene_create(C.byref(sc.desc()), C.byref(h)))
    try:
        ids = np.array([3, 1], np.uint32)
        v = np.ascontiguousarray(sc.vertices.reshape(-1, 3, 3)[ids])
        u = abi.ErSparseUpdate()
        u.what, u.count = abi.UPDATE_GEOMETRY, 2
        u.tri_ids, u.vertices = ids.ctypes.data_as(C.POINTER(C.c_uint32)), abi._fptr(v)
        assert lib.er_render_update_sparse(None, C.byref(u)) == abi.ER_ERR_INVALID_ARG
        assert lib.er_render_update_sparse(h, None) == abi.ER_ERR_INVALID_ARG
        assert b"NULL" in lib.er_last_error()
        assert lib.er_render_update_sparse(h, C.byref(u)) == abi.ER_ERR_STATE          # created, not begun
        assert b"er_render_begin" in lib.er_last_error()
        info = abi.ErSparseInfo(7, 7, 7, 7, 7, 7, 7, 7.0)
        assert lib.er_sparse_info(h, None) == abi.ER_ERR_INVALID_ARG and lib.er_sparse_info(None, C.byref(info)) == abi.ER_ERR_INVALID_ARG
        assert lib.er_sparse_info(h, C.byref(info)) == abi.ER_OK                        # counts since er_scene_create: valid before a begin
        assert [getattr(info, n) for n, _ in abi.ErSparseInfo._fields_] == [0, 0, 0, 0, 0, 0, 0, 0.0]
    finally:
        lib.er_scene_destroy(h)


def test_python_update_checks_the_listed_arrays():
    rm = render.RenderingManager()
    rm.scene = scenes.cornell(16, 16)
    v = np.zeros((3, 3, 3), np.float32)
    for kwargs, word in ((dict(tri_ids=[0, 1], vertices=v), "lists 2 triangles"),
                         (dict(tri_ids=[0, 1, 2], vertices=v, normals=np.zeros((12, 3, 3), np.float32)), "normals has 108 floats"),
                         (dict(tri_ids=[0, 1, 2], vertices=v, tangents=v[:2]), "tangents has 18 floats"),
                         (dict(tri_ids=[0, 1, 2]), "vertices"),
                         (dict(tri_ids=[[0, 1, 2]], vertices=v), "one-dimensional"),
                         (dict(tri_ids=[0.0, 1.0, 2.0], vertices=v), "triangle ids"),
                         (dict(tri_ids=[0, -1, 2], vertices=v), "triangle ids")):
        with pytest.raises(ValueError) as e:      # (before the library is reached: this manager has no handle)
            rm.update(**kwargs)
        assert word in str(e.value), (kwargs.keys(), str(e.value))


def test_check_and_patch_of_the_host_copy_under_sanitizers(tmp_path):
    """tests/native/sparse_patch.cpp: er_sparse_check and er_sparse_patch alone, with ASan + UBSan, on heap arrays of exactly the sizes the
    contract names (a read or write past count or tri_count entries is reported)"""
    exe = str(tmp_path / "sparse_patch")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "elevenrender_amd", "csrc"), os.path.join(ROOT, "tests", "native", "sparse_patch.cpp"), "-o", exe])
    out = subprocess.run([exe], text=True, capture_output=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sparse_patch ok" in out.stdout
