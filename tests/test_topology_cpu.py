"""er_render_topology / er_topology_info on a machine without a GPU: the symbols, the layouts of their structs against the C compiler's,
the call-order and argument errors that need no device, the host half of the call (csrc/er_topology_host.h: every refusal, the
compaction of the host arrays, the remap of the object table) as a stand-alone program under ASan + UBSan, elevenrender_amd/topology.py
against that program on seeded random lists, and the host server's rule for answering a --start by a topology edit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from elevenrender_amd import abi, render, scenes, topology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_topology_entry_points():
    lib = abi.load()
    for name in ("er_render_topology", "er_topology_info"):
        assert hasattr(lib, name) and name in abi.SYMBOLS
    assert lib.er_abi_version() == 2          # an addition: nothing existing changed layout
    assert (abi.TOPO_REMOVE, abi.TOPO_APPEND) == (1, 2)


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    T, I = abi.ErTopologyEdit, abi.ErTopologyInfo
    tf = [n for n, _ in T._fields_]
    inf = [n for n, _ in I._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eleven_hip.h"\n'
                   'int main(void) { printf("%zu %zu %u %u\\n", sizeof(ErTopologyEdit), sizeof(ErTopologyInfo), ER_TOPO_REMOVE, ER_TOPO_APPEND);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(ErTopologyEdit, {n}));\n' for n in tf)
                   + "".join(f'  printf("%zu\\n", offsetof(ErTopologyInfo, {n}));\n' for n in inf)
                   + '  return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got[:4] == [C.sizeof(T), C.sizeof(I), abi.TOPO_REMOVE, abi.TOPO_APPEND]
    assert got[4:] == [getattr(T, n).offset for n in tf] + [getattr(I, n).offset for n in inf]


def _append_edit(sc, k=2):
    t = abi.ErTopologyEdit()
    t.what, t.append_count = abi.TOPO_APPEND, k
    arrays = [np.ascontiguousarray(getattr(sc, n)[:k]) for n in topology.ARRAYS]
    for n, a in zip(topology.ARRAYS[:5], arrays):
        setattr(t, n, abi._fptr(a))
    t.material_id = arrays[5].ctypes.data_as(C.POINTER(C.c_int32))
    return t, arrays


def test_topology_needs_a_begun_scene_and_arguments():
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    h = C.c_void_p()
    abi.check(lib.er_scene_create(C.byref(sc.desc()), C.byref(h)))
    try:
        t, keep = _append_edit(sc)
        assert lib.er_render_topology(None, C.byref(t)) == abi.ER_ERR_INVALID_ARG
        assert lib.er_render_topology(h, None) == abi.ER_ERR_INVALID_ARG
        assert b"NULL" in lib.er_last_error()
        assert lib.er_render_topology(h, C.byref(t)) == abi.ER_ERR_STATE          # created, not begun
        assert b"er_render_begin" in lib.er_last_error()
        t.what = 0
        assert lib.er_render_topology(h, C.byref(t)) == abi.ER_ERR_STATE          # (the state comes first, as in every edit path)
        info = abi.ErTopologyInfo(7, 7, 7, 7, 7, 7, 7, 7.0, 7.0, 7.0, 7.0)
        assert lib.er_topology_info(h, None) == abi.ER_ERR_INVALID_ARG and lib.er_topology_info(None, C.byref(info)) == abi.ER_ERR_INVALID_ARG
        assert lib.er_topology_info(h, C.byref(info)) == abi.ER_OK                # counts since er_scene_create: valid before a begin
        assert [getattr(info, n) for n, _ in abi.ErTopologyInfo._fields_] == [0] * 7 + [0.0] * 4
    finally:
        lib.er_scene_destroy(h)


def test_python_topology_checks_its_lists():
    rm = render.RenderingManager()
    rm.scene = scenes.cornell(16, 16)
    tail = {n: getattr(rm.scene, n)[:3] for n in topology.ARRAYS}
    short = dict(tail, normals=tail["normals"][:2])
    n = rm.scene.tri_count
    for kwargs, word in ((dict(remove=[[0, 1]]), "one-dimensional"),
                         (dict(remove=[0.5]), "triangle ids"),
                         (dict(remove=[-1]), "triangle ids"),
                         (dict(append=short), "normals holds 2 triangles"),
                         (dict(append=tail, material_id=np.zeros(n, np.int32)), "material_id comes with the material list"),
                         (dict(remove=[0], append=tail, materials=rm.scene.materials, material_id=np.zeros(n, np.int32)), f"the scene has {n + 2} triangles")):
        with pytest.raises(ValueError) as e:      # (before the library is reached: this manager has no handle)
            rm.topology(**kwargs)
        assert word in str(e.value), (kwargs.keys(), str(e.value))


def test_numbering_in_numpy():
    assert topology.new_ids(6, [3, 0]).tolist() == [-1, 0, 1, -1, 2, 3]
    assert topology.new_ids(4, None).tolist() == [0, 1, 2, 3]
    assert topology.new_ids(3, [0, 1, 2]).tolist() == [-1, -1, -1]
    for bad in ([3], [1, 1], [-1]):
        with pytest.raises(ValueError):
            topology.new_ids(3, bad)
    assert topology.bytes_uploaded(10, 3) == 4 * 10 + 140 * 3
    sc = scenes.cornell(16, 16)
    n = sc.tri_count
    tail = {k: getattr(sc, k)[:2] for k in topology.ARRAYS}
    out = topology.apply(sc, remove=[0, n - 1], append=tail, material_id=np.zeros(n, np.int32))
    assert out.tri_count == n and (out.vertices[:n - 2] == sc.vertices[1:n - 1]).all() and (out.vertices[n - 2:] == sc.vertices[:2]).all()
    assert (out.uvs[:n - 2] == sc.uvs[1:n - 1]).all() and (out.tangent_sign[n - 2:] == sc.tangent_sign[:2]).all() and not out.material_id.any()
    assert (topology.apply(sc, remove=[1]).material_id == np.delete(sc.material_id, 1)).all()
    lists = topology.remap_objects([[6, 1], [2, 3], [], [7, 0, 4]], [7, 2, 3, 6, 0], 8, append_count=2, as_object=True)
    assert [o.tolist() for o in lists] == [[0], [], [], [1], [3, 4]]
    assert [o.tolist() for o in topology.remap_objects([], [0], 8, append_count=2, as_object=True)] == []      # no table: none is made


@pytest.fixture(scope="module")
def topology_patch(tmp_path_factory):
    """tests/native/topology_patch.cpp: csrc/er_topology_host.h alone, with ASan + UBSan"""
    exe = str(tmp_path_factory.mktemp("topo") / "topology_patch")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "elevenrender_amd", "csrc"), os.path.join(ROOT, "tests", "native", "topology_patch.cpp"), "-o", exe])
    return exe


def test_checks_compaction_and_object_remap_under_sanitizers(topology_patch):
    """every refusal with its text, the compaction on heap arrays of exactly the sizes the contract names (a read or write past them is
    reported), and the object table's remap against hand-written cases: removal of a whole object, of the first and the last id, of
    nothing but an append, of everything"""
    out = subprocess.run([topology_patch], text=True, capture_output=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "topology_patch ok" in out.stdout


def test_numpy_numbering_equals_the_headers_on_seeded_random_lists(topology_patch):
    rng = np.random.default_rng(20)
    for case in range(24):
        n = int(rng.integers(1, 700))
        r = int(rng.integers(0, n + 1)) if case % 4 else (0 if case % 8 else n)
        a = int(rng.integers(0, 5)) if r else int(rng.integers(1, 5))      # (an edit names at least one of the two)
        remove = rng.permutation(n)[:r]
        objects = int(rng.integers(0, 5))
        listed = rng.permutation(n)[:int(rng.integers(0, n + 1))]
        cuts = np.sort(rng.integers(0, listed.size + 1, max(objects - 1, 0)))
        objs = [o for o in np.split(listed, cuts)] if objects else []
        as_object = int(rng.integers(0, 2))
        text = f"{n} {r} " + " ".join(map(str, remove)) + f" {a} {as_object} {len(objs)} " + " ".join(f"{o.size} " + " ".join(map(str, o)) for o in objs)
        out = subprocess.run([topology_patch, "apply"], input=text, text=True, capture_output=True)
        assert out.returncode == 0, (case, out.stdout, out.stderr)
        lines = out.stdout.split("\n")
        got = [int(x) for x in lines[0].split()]
        ids = topology.new_ids(n, remove)
        order = np.argsort(ids[ids >= 0])      # new id -> old id, through the numbering alone
        want = np.flatnonzero(ids >= 0)[order].tolist() + [-1 - j for j in range(a)]
        assert got == want, case
        tables = topology.remap_objects(objs, remove, n, append_count=a, as_object=bool(as_object))
        assert len(tables) == len(objs) + (1 if objs and as_object and a else 0)
        for k, o in enumerate(tables):
            assert [int(x) for x in lines[1 + k].split()] == o.tolist(), (case, k)


def test_host_answers_a_start_after_object_loads_by_a_topology_edit():
    """eleven::SessionEdits through tests/native/session_topology.cpp: s / f = a --start that succeeds / fails, c = --load_camera,
    h = --load_hdri, m = --load_brdf_material or --load_texture, o = --load_object, g = --load_config; per --start c = in-place camera
    update, e = in-place scene edit, t = in-place topology edit, 0 = the full start."""
    exe = os.path.join(ROOT, "tests", "native", "session_topology")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "native", "session_topology.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "elevenrender_amd"), "-leleven_hip", "-Wl,-rpath,$ORIGIN/../../elevenrender_amd"])
    sessions = {"gochms": "0",            # the first start of a session builds
                "gochmsos": "0t",         # an object alone: appended in place
                "gosochms": "0t",         # ... with a camera, an HDRI, materials and textures beside it
                "gosoosos": "0tt",        # two objects in one edit, then another
                "gosgs": "00",            # --load_config still forces the full start
                "gosogs": "00",           # ... also beside an object
                "gosofos": "0t0",         # a failed start leaves nothing to edit
                "gosfs": "0c0",
                "os": "0",                # an object before the first start is part of that start
                "goscshsmscs": "0ceec",   # the existing answers stay
                "gosohscs": "0tc"}        # after a topology edit the session is editable as after a start
    out = subprocess.check_output([exe] + list(sessions), text=True).split("\n")[:len(sessions)]
    assert out == list(sessions.values()), dict(zip(sessions, out))
