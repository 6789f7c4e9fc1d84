"""er_render_update / er_update_info on a machine without a GPU: the symbols, the layouts of their structs against the C compiler's,
the call-order and argument errors that need no device, and the host server's rule for restarting a render in place."""
import ctypes as C
import os
import subprocess

import numpy as np

from elevenrender_amd import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_update_entry_points():
    lib = abi.load()
    for name in ("er_render_update", "er_update_info"):
        assert hasattr(lib, name) and name in abi.SYMBOLS
    assert lib.er_abi_version() == 2          # nothing existing changed layout
    assert (abi.UPDATE_CAMERA, abi.UPDATE_GEOMETRY) == (1, 2)


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "eleven_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %u %u\\n", sizeof(ErSceneUpdate), offsetof(ErSceneUpdate, camera), offsetof(ErSceneUpdate, vertices),\n'
                   '  offsetof(ErSceneUpdate, tangents), sizeof(ErUpdateInfo), offsetof(ErUpdateInfo, update_ms), ER_UPDATE_CAMERA, ER_UPDATE_GEOMETRY); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    U, I = abi.ErSceneUpdate, abi.ErUpdateInfo
    assert got == [C.sizeof(U), U.camera.offset, U.vertices.offset, U.tangents.offset, C.sizeof(I), I.update_ms.offset, abi.UPDATE_CAMERA, abi.UPDATE_GEOMETRY]


def test_update_needs_a_begun_scene_and_arguments():
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    h = C.c_void_p()
    abi.check(lib.er_scene_create(C.byref(sc.desc()), C.byref(h)))
    try:
        u = abi.ErSceneUpdate()
        u.what = abi.UPDATE_CAMERA
        u.camera = sc.camera
        assert lib.er_render_update(None, C.byref(u)) == abi.ER_ERR_INVALID_ARG
        assert lib.er_render_update(h, None) == abi.ER_ERR_INVALID_ARG
        assert b"NULL" in lib.er_last_error()
        assert lib.er_render_update(h, C.byref(u)) == abi.ER_ERR_STATE          # created, not begun
        assert b"er_render_begin" in lib.er_last_error()
        u.what = abi.UPDATE_GEOMETRY
        u.vertices = abi._fptr(sc.vertices)
        assert lib.er_render_update(h, C.byref(u)) == abi.ER_ERR_STATE
        info = abi.ErUpdateInfo(7, 7, 7.0, 7.0)
        assert lib.er_update_info(h, None) == abi.ER_ERR_INVALID_ARG and lib.er_update_info(None, C.byref(info)) == abi.ER_ERR_INVALID_ARG
        assert lib.er_update_info(h, C.byref(info)) == abi.ER_OK                # counts since er_scene_create: valid before a begin
        assert (info.updates, info.refits, info.refit_ms, info.update_ms) == (0, 0, 0.0, 0.0)
    finally:
        lib.er_scene_destroy(h)


def test_python_update_checks_the_array_sizes():
    from elevenrender_amd import render
    rm = render.RenderingManager()
    rm.scene = scenes.cornell(16, 16)
    try:
        rm.update(vertices=np.zeros((5, 3, 3), np.float32))
    except ValueError as e:
        assert "12 triangles" in str(e)
    else:
        raise AssertionError("a vertex array of another size was accepted")


def test_host_restarts_in_place_only_after_nothing_but_a_camera():
    """eleven::SessionEdits through tests/native/session_edits.cpp: s / f = a --start that succeeds / fails, c = --load_camera, o = any
    other load; per --start 1 = in-place camera update, 0 = the full start."""
    exe = os.path.join(ROOT, "tests", "native", "session_edits")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "native", "session_edits.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "elevenrender_amd"), "-leleven_hip", "-Wl,-rpath,$ORIGIN/../../elevenrender_amd"])
    sessions = {"ocs": "0",            # the first start of a session builds
                "ocscs": "01",         # a camera alone: in place
                "ocscscs": "011",      # ... every time
                "ocsss": "011",        # no edit at all: the same render again, no rebuild either
                "ocsos": "00",         # another load: full start
                "ocscocs": "00",       # camera and another load, either order
                "ocsocs": "00",
                "ocsoscs": "001",      # the flag clears with the start that consumed it
                "ocfcs": "00",         # a start that failed left nothing to update
                "ocscfcs": "010"}      # ... nor does an update that failed
    out = subprocess.check_output([exe] + list(sessions), text=True).split("\n")
    assert dict(zip(sessions, out)) == sessions


def test_server_reports_no_update_without_a_render():
    """the CPU part of the session: loads are answered ok, --start fails cleanly without a device, and a second --start after a new
    camera fails the same way (there is no render to update)"""
    import pytest
    from elevenrender_amd import client
    from test_host_server import Server
    if abi.load().er_device_count() > 0:
        return      # (with a device tests/test_gpu_update.py plays the whole session)
    s = Server()
    c = client.Client(port=s.port)
    with pytest.raises(client.ProtocolError) as e:
        client.play_cornell_session(c, client.cornell_session_assets(32, 24), sample_target=2)
    assert "no HIP device" in str(e.value)
    c.load_camera(position=(0.2, 0.0, -1.7))
    t, f, d = c.command("--start")
    assert d.startswith(b"error:") and b"no HIP device" in d
    c.close()
    assert s.finish() == 0
