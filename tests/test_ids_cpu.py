"""Id planes, mattes and picking (include/eleven_hip.h er_render_ids, er_id_info, er_read_ids, er_gather_ids, er_id_matte, er_pick_rect,
er_pick) on a machine without a GPU: the symbols and constants, the layouts of ErIdInfo and ErPick against the C compiler's, the
argument and call-order errors that need no device, the ranking of a pixel's ids (er_debug_id_rank: csrc/er_ids.h, the function the
kernel calls) against its numpy restatement (elevenrender_amd/ids.py) word for word, and the header's host functions as a stand-alone
program under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from elevenrender_amd import abi, ids, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("er_render_ids", "er_id_info", "er_read_ids", "er_gather_ids", "er_id_matte", "er_pick_rect", "er_pick")
NONE = abi.ID_NONE


def test_library_exports_the_id_entry_points():
    lib = abi.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in abi.SYMBOLS, name
    assert hasattr(lib, "er_debug_id_rank")
    assert lib.er_abi_version() == 2          # entry points and structs were added, none grew
    assert (abi.ID_TRIANGLE, abi.ID_OBJECT, abi.ID_MATERIAL, abi.ID_KIND_COUNT) == (0, 1, 2, 3)
    assert abi.ID_KIND_NAMES == {"triangle": 0, "object": 1, "material": 2}
    assert (abi.ID_NONE, abi.ID_SLOTS) == (0xFFFFFFFF, 4) == (ids.ID_NONE, ids.ID_SLOTS)
    assert abi.FEATURE_COUNT == 2 and abi.PASS_COUNT == 5          # a new family, not new members of those enums


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eleven_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %d %d %d %d %d\\n", sizeof(ErIdInfo), offsetof(ErIdInfo, samples),\n'
                   '  offsetof(ErIdInfo, rays), offsetof(ErIdInfo, ms), offsetof(ErIdInfo, objects), offsetof(ErIdInfo, overflow_pixels),\n'
                   '  sizeof(ErPick), offsetof(ErPick, hit), offsetof(ErPick, triangle), offsetof(ErPick, object), offsetof(ErPick, material),\n'
                   '  offsetof(ErPick, distance), offsetof(ErPick, position), offsetof(ErPick, uv), ER_ID_NONE, (int)ER_ID_SLOTS, (int)ER_ID_TRIANGLE,\n'
                   '  (int)ER_ID_OBJECT, (int)ER_ID_MATERIAL, (int)ER_ID_KIND_COUNT); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    I, P = abi.ErIdInfo, abi.ErPick
    assert got == [C.sizeof(I), I.samples.offset, I.rays.offset, I.ms.offset, I.objects.offset, I.overflow_pixels.offset,
                   C.sizeof(P), P.hit.offset, P.triangle.offset, P.object.offset, P.material.offset, P.distance.offset, P.position.offset, P.uv.offset,
                   abi.ID_NONE, abi.ID_SLOTS, abi.ID_TRIANGLE, abi.ID_OBJECT, abi.ID_MATERIAL, abi.ID_KIND_COUNT]
    assert C.sizeof(I) == 40 and C.sizeof(P) == 40


def test_arguments_and_call_order_without_a_device():
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    h = C.c_void_p()
    abi.check(lib.er_scene_create(C.byref(sc.desc()), C.byref(h)))
    comms = (C.c_void_p * 2)()
    abi.check(lib.er_comm_create_local(2, comms))
    words = np.zeros(16 * 16 * 4, np.uint32)
    up = words.ctypes.data_as(C.POINTER(C.c_uint32))
    plane = np.zeros(16 * 16, np.float32)
    fp = plane.ctypes.data_as(C.POINTER(C.c_float))
    info, pick, n = abi.ErIdInfo(), abi.ErPick(), C.c_uint32()
    INV, STATE = abi.ER_ERR_INVALID_ARG, abi.ER_ERR_STATE
    try:
        # NULL arguments
        assert lib.er_render_ids(None, 4) == INV
        assert lib.er_id_info(None, C.byref(info)) == INV and lib.er_id_info(h, None) == INV
        assert lib.er_read_ids(None, 0, up, up) == INV and lib.er_read_ids(h, 0, None, None) == INV
        assert lib.er_gather_ids(None, 0, comms[0], 0) == INV and lib.er_gather_ids(h, 0, None, 0) == INV
        assert lib.er_id_matte(None, 0, up, 1, fp) == INV and lib.er_id_matte(h, 0, None, 1, fp) == INV and lib.er_id_matte(h, 0, up, 1, None) == INV
        assert lib.er_pick_rect(None, 0, 0, 1, 1, 0, up, 4, C.byref(n)) == INV and lib.er_pick_rect(h, 0, 0, 1, 1, 0, up, 4, None) == INV
        assert lib.er_pick_rect(h, 0, 0, 1, 1, 0, None, 4, C.byref(n)) == INV          # (NULL ids go with capacity 0 only)
        assert lib.er_pick(None, 0, 0, C.byref(pick)) == INV and lib.er_pick(h, 0, 0, None) == INV
        assert b"NULL" in lib.er_last_error()
        # a created scene that is not begun: a state error from all seven
        assert lib.er_render_ids(h, 0) == STATE
        assert b"er_render_begin" in lib.er_last_error()
        assert lib.er_render_ids(h, 64) == STATE
        assert lib.er_id_info(h, C.byref(info)) == STATE
        for kind in range(abi.ID_KIND_COUNT):
            assert lib.er_read_ids(h, kind, up, up) == STATE and lib.er_read_ids(h, kind, up, None) == STATE and lib.er_read_ids(h, kind, None, up) == STATE
            assert lib.er_gather_ids(h, kind, comms[0], 0) == STATE
            assert lib.er_id_matte(h, kind, up, 3, fp) == STATE
            assert lib.er_pick_rect(h, 0, 0, 16, 16, kind, up, 8, C.byref(n)) == STATE and lib.er_pick_rect(h, 3, 4, 4, 5, kind, None, 0, C.byref(n)) == STATE
        assert lib.er_pick(h, 0, 0, C.byref(pick)) == STATE and lib.er_pick(h, 15, 15, C.byref(pick)) == STATE
        # values out of range are argument errors, begun or not
        assert lib.er_render_ids(h, 65) == INV
        assert b"64" in lib.er_last_error()
        for kind in (-1, 3, 7):
            assert lib.er_read_ids(h, kind, up, up) == INV
            assert lib.er_gather_ids(h, kind, comms[0], 0) == INV
            assert lib.er_id_matte(h, kind, up, 1, fp) == INV
            assert lib.er_pick_rect(h, 0, 0, 1, 1, kind, up, 4, C.byref(n)) == INV
            assert b"kind" in lib.er_last_error()
        assert lib.er_gather_ids(h, 0, comms[0], 2) == INV                              # root >= world
        assert lib.er_id_matte(h, 0, up, 0, fp) == INV                                  # an empty list
        for rect in ((4, 0, 4, 1), (5, 0, 4, 1), (0, 4, 1, 4), (0, 5, 1, 4), (0, 0, 17, 1), (0, 0, 1, 17), (16, 0, 17, 1)):
            assert lib.er_pick_rect(h, *rect, 0, up, 4, C.byref(n)) == INV, rect
        for x, y in ((16, 0), (0, 16), (0xFFFFFFFF, 0)):
            assert lib.er_pick(h, x, y, C.byref(pick)) == INV
        # neither the passes nor the features grew, and the id planes are not part of the state
        assert lib.er_read_pass(h, 5, fp) == INV and lib.er_read_feature(h, 2, fp) == INV
        size = C.c_uint64()
        assert lib.er_state_size(h, C.byref(size)) == abi.ER_OK and size.value == 64 + 16 * 16 * (5 * 16 + 8)
    finally:
        lib.er_scene_destroy(h)
        for c in comms:
            lib.er_comm_destroy(c)


# ---- the ranking ----

def rank_cases():
    rng = np.random.default_rng(11)
    cases = {}
    for m in range(1, 65):          # random multisets of 1 .. 64 ids out of a few, so counts repeat and tie
        cases[f"random-{m}"] = rng.integers(0, 1 + m // 3, m).astype(np.uint32) * np.uint32(2654435761)
    cases["wide-ids"] = rng.integers(0, 2**32, 40, dtype=np.uint64).astype(np.uint32)
    cases["64-distinct"] = rng.permutation(64).astype(np.uint32) + np.uint32(1000)
    cases["64-equal"] = np.full(64, 77, np.uint32)
    cases["tie-at-the-cut"] = np.array([9, 9, 9, 5, 5, 8, 8, 2, 3, 3, 7, 7, 1], np.uint32)          # counts 3 2 2 | 2 2 1 1: ids 3 and 5 stay, 7 and 8 go
    cases["all-tied"] = np.array([50, 40, 30, 20, 10, 60], np.uint32)
    cases["none-among"] = np.array([NONE, 4, NONE, 4, 6, 6, 1, 1, NONE], np.uint32)
    cases["none-tied-last"] = np.array([NONE, NONE, 3, 3, 2, 2, 1, 1, 0, 0], np.uint32)              # five ids tied: NONE is the one cut
    cases["none-only"] = np.full(5, NONE, np.uint32)
    cases["zero-hits"] = np.zeros(0, np.uint32)
    return cases


@pytest.mark.parametrize("name", list(rank_cases()))
def test_rank_equals_the_numpy_restatement(name):
    a = rank_cases()[name]
    gi, gc, gd = abi.debug_id_rank(a)
    wi, wc, wd = ids.rank(a)
    assert (gi == wi).all() and (gc == wc).all() and gd == wd, (name, gi, gc, gd, wi, wc, wd)
    # the properties, from the definition alone
    assert gc.sum() <= a.size and (gc.sum() == a.size) == (wd <= 4)
    assert all(int(gc[s]) == int((a == gi[s]).sum()) for s in range(4) if gc[s])
    assert all((int(gc[s]), -int(gi[s])) >= (int(gc[s + 1]), -int(gi[s + 1])) for s in range(3))
    assert all(gi[s] == NONE for s in range(4) if gc[s] == 0)
    if name == "tie-at-the-cut":
        assert ids.tie_at_the_cut(a) and list(gi) == [9, 3, 5, 7] and list(gc) == [3, 2, 2, 2] and gd == 7
    if name == "none-tied-last":
        assert ids.tie_at_the_cut(a) and list(gi) == [0, 1, 2, 3] and gd == 5
    if name == "none-among":
        assert list(gi) == [NONE, 1, 4, 6] and list(gc) == [3, 2, 2, 2]
    if name == "zero-hits":
        assert list(gi) == [NONE] * 4 and list(gc) == [0] * 4 and gd == 0
    if name == "64-distinct":
        assert list(gi) == [1000, 1001, 1002, 1003] and gd == 64
    if name == "64-equal":
        assert list(gi) == [77, NONE, NONE, NONE] and list(gc) == [64, 0, 0, 0]


def test_rank_refuses_what_it_cannot_hold():
    lib = abi.load()
    a = np.zeros(80, np.uint32)
    o = np.zeros(4, np.uint32)
    up = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))
    d = C.c_uint32()
    assert lib.er_debug_id_rank(up(a), 65, up(o), up(o), C.byref(d)) == abi.ER_ERR_INVALID_ARG
    assert lib.er_debug_id_rank(None, 3, up(o), up(o), C.byref(d)) == abi.ER_ERR_INVALID_ARG
    assert lib.er_debug_id_rank(up(a), 3, None, up(o), C.byref(d)) == abi.ER_ERR_INVALID_ARG
    assert lib.er_debug_id_rank(up(a), 3, up(o), up(o), None) == abi.ER_ERR_INVALID_ARG


def test_numpy_helpers_on_a_small_frame():
    i = np.array([[[3, 1, NONE, NONE], [NONE, 2, NONE, NONE]], [[NONE, NONE, NONE, NONE], [7, NONE, NONE, NONE]]], np.uint32)
    c = np.array([[[2, 1, 0, 0], [3, 1, 0, 0]], [[0, 0, 0, 0], [4, 0, 0, 0]]], np.uint32)
    assert list(ids.rect(i, c, 0, 0, 2, 2)) == [1, 2, 3, 7, NONE] and list(ids.rect(i, c, 0, 1, 1, 2)) == []
    m = ids.matte(i, c, [NONE, 3, 3], 4)
    assert m.dtype == np.float32 and (m == np.array([[0.5, 0.75], [0.0, 0.0]], np.float32)).all()
    assert list(ids.object_of(6, [[4, 1], [], [0]])) == [2, 0, NONE, NONE, 0, NONE]


def test_host_functions_under_sanitizers(tmp_path):
    """tests/native/ids_host.cpp: er_ids.h alone -- the ranking, the membership and object searches, the list preparation, the map and a
    matte pixel -- with ASan + UBSan, on heap arrays of exactly the sizes the contract names"""
    exe = str(tmp_path / "ids_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "elevenrender_amd", "csrc"), os.path.join(ROOT, "tests", "native", "ids_host.cpp"), "-o", exe])
    out = subprocess.run([exe], text=True, capture_output=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ids_host ok" in out.stdout
