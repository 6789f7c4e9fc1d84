"""The feature planes and the guided denoise (include/eleven_hip.h er_render_features, er_feature_info, er_read_feature,
er_gather_feature, er_denoise_guided) on a machine without a GPU: the symbols, the layouts of their structs against the C
compiler's, the argument and call-order errors that need no device, that the pass ids of the existing entry points did not
grow, and the host server's two new config keys."""
import ctypes as C
import os
import subprocess

import numpy as np

from elevenrender_amd import abi, client, scenes
from test_host_server import Server

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("er_render_features", "er_feature_info", "er_read_feature", "er_gather_feature", "er_denoise_guided")


def test_library_exports_the_feature_entry_points():
    lib = abi.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in abi.SYMBOLS, name
    assert lib.er_abi_version() == 2          # entry points were added, no caller-allocated struct grew
    assert (abi.FEATURE_ALBEDO, abi.FEATURE_DEPTH, abi.FEATURE_COUNT) == (0, 1, 2)
    assert abi.FEATURE_NAMES == {"albedo": 0, "depth": 1}
    assert abi.PASS_COUNT == 5 and set(abi.PASS_NAMES) == {"beauty", "denoise", "normal", "tangent", "bitangent"}


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "eleven_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(ErFeatureInfo), offsetof(ErFeatureInfo, samples),\n'
                   '  offsetof(ErFeatureInfo, rays), offsetof(ErFeatureInfo, ms), sizeof(ErDenoiseGuided), offsetof(ErDenoiseGuided, colour_sigma),\n'
                   '  offsetof(ErDenoiseGuided, depth_sigma), (int)ER_FEATURE_ALBEDO, (int)ER_FEATURE_DEPTH, (int)ER_FEATURE_COUNT, (int)ER_PASS_COUNT); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    I, G = abi.ErFeatureInfo, abi.ErDenoiseGuided
    assert got == [C.sizeof(I), I.samples.offset, I.rays.offset, I.ms.offset, C.sizeof(G), G.colour_sigma.offset, G.depth_sigma.offset,
                   abi.FEATURE_ALBEDO, abi.FEATURE_DEPTH, abi.FEATURE_COUNT, abi.PASS_COUNT]
    assert C.sizeof(I) == 24 and C.sizeof(G) == 16


def test_arguments_and_call_order_without_a_device():
    lib = abi.load()
    sc = scenes.cornell(16, 16)
    h = C.c_void_p()
    abi.check(lib.er_scene_create(C.byref(sc.desc()), C.byref(h)))
    comms = (C.c_void_p * 2)()
    abi.check(lib.er_comm_create_local(2, comms))
    buf = np.zeros(16 * 16 * 4, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    info = abi.ErFeatureInfo()
    g = abi.ErDenoiseGuided(0, 0.0, 0.0, 0.0)
    try:
        # NULL arguments
        assert lib.er_render_features(None, 4) == abi.ER_ERR_INVALID_ARG
        assert lib.er_feature_info(None, C.byref(info)) == abi.ER_ERR_INVALID_ARG and lib.er_feature_info(h, None) == abi.ER_ERR_INVALID_ARG
        assert lib.er_read_feature(None, 0, fp) == abi.ER_ERR_INVALID_ARG and lib.er_read_feature(h, 0, None) == abi.ER_ERR_INVALID_ARG
        assert lib.er_gather_feature(None, 0, comms[0], 0) == abi.ER_ERR_INVALID_ARG and lib.er_gather_feature(h, 0, None, 0) == abi.ER_ERR_INVALID_ARG
        assert lib.er_denoise_guided(None, C.byref(g)) == abi.ER_ERR_INVALID_ARG and lib.er_denoise_guided(h, None) == abi.ER_ERR_INVALID_ARG
        assert b"NULL" in lib.er_last_error()
        # a created scene that is not begun: a state error from all five
        assert lib.er_render_features(h, 0) == abi.ER_ERR_STATE
        assert b"er_render_begin" in lib.er_last_error()
        assert lib.er_render_features(h, 64) == abi.ER_ERR_STATE
        assert lib.er_feature_info(h, C.byref(info)) == abi.ER_ERR_STATE
        assert lib.er_read_feature(h, abi.FEATURE_ALBEDO, fp) == abi.ER_ERR_STATE and lib.er_read_feature(h, abi.FEATURE_DEPTH, fp) == abi.ER_ERR_STATE
        assert lib.er_gather_feature(h, abi.FEATURE_DEPTH, comms[0], 0) == abi.ER_ERR_STATE
        assert lib.er_denoise_guided(h, C.byref(g)) == abi.ER_ERR_STATE
        assert lib.er_denoise_guided(h, C.byref(abi.ErDenoiseGuided(8, 2.0, 0.1, 0.05))) == abi.ER_ERR_STATE
        # values out of range are argument errors, begun or not
        assert lib.er_render_features(h, 65) == abi.ER_ERR_INVALID_ARG
        assert b"64" in lib.er_last_error()
        for bad in (abi.ErDenoiseGuided(0, -1.0, 0.0, 0.0), abi.ErDenoiseGuided(0, 0.0, -0.5, 0.0), abi.ErDenoiseGuided(0, 0.0, 0.0, -1e-9),
                    abi.ErDenoiseGuided(0, float("nan"), 0.0, 0.0), abi.ErDenoiseGuided(0, 0.0, 0.0, float("nan")), abi.ErDenoiseGuided(9, 0.0, 0.0, 0.0)):
            assert lib.er_denoise_guided(h, C.byref(bad)) == abi.ER_ERR_INVALID_ARG
        for f in (-1, 2, 5):
            assert lib.er_read_feature(h, f, fp) == abi.ER_ERR_INVALID_ARG
            assert lib.er_gather_feature(h, f, comms[0], 0) == abi.ER_ERR_INVALID_ARG
        assert lib.er_gather_feature(h, 0, comms[0], 2) == abi.ER_ERR_INVALID_ARG          # root >= world
        # the pass ids of the existing entry points did not grow: a feature is not a pass
        for p in (5, 6, 7):
            assert lib.er_read_pass(h, p, fp) == abi.ER_ERR_INVALID_ARG
            assert lib.er_gather_pass(h, p, comms[0], 0) == abi.ER_ERR_INVALID_ARG
            assert lib.er_pack_owned(h, p, C.c_void_p(16)) == abi.ER_ERR_INVALID_ARG
            assert lib.er_unpack_owned(h, p, 0, C.c_void_p(16)) == abi.ER_ERR_INVALID_ARG
        n = C.c_uint64()
        assert lib.er_state_size(h, C.byref(n)) == abi.ER_OK and n.value == 64 + 16 * 16 * (5 * 16 + 8)      # features are not part of the state
    finally:
        lib.er_scene_destroy(h)
        for c in comms:
            lib.er_comm_destroy(c)


def test_textured_cornell_scene():
    sc, plain = scenes.cornell_textured(32, 24), scenes.cornell(32, 24)
    assert (sc.vertices == plain.vertices).all() and (sc.material_id == plain.material_id).all()
    (data, w, h, ch, flt), = sc.textures
    assert (w, h, ch, flt) == (64, 64, 3, 0) and data.shape == (64, 64, 3)
    assert (data[0:8, 0:8] == np.array([0.9, 0.85, 0.8], np.float32)).all() and (data[0:8, 8:16] == np.array([0.15, 0.2, 0.3], np.float32)).all()
    assert (data[8:16, 0:8] == data[0:8, 8:16]).all() and (data[8:16, 8:16] == data[0:8, 0:8]).all()
    assert sc.materials[0].albedo_tex == 0 and all(m.albedo_tex == -1 for m in sc.materials[1:])
    assert scenes.cornell(32, 24).materials[0].albedo_tex == -1          # the generator it starts from is unchanged


def test_host_server_config_keys_for_the_guided_denoise():
    """load_config accepts `denoise_guided` and `feature_samples` and refuses bad values with its usual error replies; --get_pass albedo
    before a render is the error every get_pass gives."""
    s = Server()
    c = client.Client(port=s.port)
    base = dict(x_res=32, y_res=24, sample_target=2, denoise=True, device="", block_size=8)
    for good in (dict(denoise_guided=True), dict(denoise_guided=False, feature_samples=1), dict(denoise_guided=True, feature_samples=64)):
        c.expect_ok("--load_config", client.Client._json(dict(base, **good)))
    for bad, text in ((dict(feature_samples=0), b"feature_samples out of range"), (dict(feature_samples=65), b"feature_samples out of range"),
                      (dict(feature_samples=-3), b"feature_samples out of range"), (dict(feature_samples=2.5), b"integer expected"),
                      (dict(denoise_guided=1), b"json"), (dict(denoise_guided="yes"), b"json")):
        t, f, d = c.command("--load_config", client.Client._json(dict(base, **bad)))
        assert t == "status" and d.startswith(b"error:") and text in d, (bad, d)
    for name in ("albedo", "depth", "ALBEDO"):
        t, f, d = c.command(f"--get_pass {name}")
        assert d.startswith(b"error:") and b"no render" in d, d
    c.close()
    assert s.finish() == 0
