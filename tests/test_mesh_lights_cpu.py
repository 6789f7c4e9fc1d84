"""ER_FLAG_MESH_LIGHTS (next-event estimation of emissive triangles, csrc/er_shade.h) without a GPU: the flag and struct of the
ABI, the argument checks of er_light_info that need no device, and the host server's config key."""
import ctypes as C
import os
import re

import pytest

from elevenrender_amd import abi, client, scenes

from test_host_server import Server

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_matches_the_header():
    text = open(os.path.join(ROOT, "include", "eleven_hip.h")).read()
    m = re.search(r"#define ER_FLAG_MESH_LIGHTS\s+(\d+)u", text)
    assert m and int(m.group(1)) == abi.FLAG_MESH_LIGHTS == 1024
    others = [int(v) for k, v in re.findall(r"#define (ER_FLAG_\w+)\s+(\d+)u", text) if k != "ER_FLAG_MESH_LIGHTS"]
    assert abi.FLAG_MESH_LIGHTS not in others
    assert C.sizeof(abi.ErLightInfo) == 8


def test_light_info_validates_without_a_device():
    lib = abi.load()
    for n in ("er_light_info", "er_debug_read_light_table"):
        assert hasattr(lib, n) and n in abi.SYMBOLS
    info = abi.ErLightInfo()
    assert lib.er_light_info(None, C.byref(info)) == abi.ER_ERR_INVALID_ARG
    sc = scenes.cornell(16, 16)
    h = C.c_void_p()
    assert lib.er_scene_create(C.byref(sc.desc()), C.byref(h)) == abi.ER_OK
    try:
        assert lib.er_light_info(h, None) == abi.ER_ERR_INVALID_ARG
        assert lib.er_light_info(h, C.byref(info)) == abi.ER_ERR_STATE
        assert b"er_light_info" in lib.er_last_error()
        assert lib.er_debug_read_light_table(h, None, None, 4) == abi.ER_ERR_STATE
    finally:
        lib.er_scene_destroy(h)


def test_host_parses_the_mesh_lights_key():
    s = Server()
    c = client.Client(port=s.port)
    base = dict(x_res=32, y_res=24, sample_target=2, denoise=False, device="", block_size=8)
    t, f, d = c.command("--load_config", client.Client._json(dict(base, mesh_lights="yes")))      # read as a boolean
    assert d.startswith(b"error:"), d
    for v in (True, False):
        t, f, d = c.command("--load_config", client.Client._json(dict(base, mesh_lights=v)))
        assert not d.startswith(b"error:"), d
    c.close()
    assert s.finish() == 0
