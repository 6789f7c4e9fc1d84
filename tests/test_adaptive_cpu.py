"""Adaptive sampling (include/eleven_hip.h er_adaptive_set / er_adaptive_info / er_read_tile_state) without a GPU: the ABI's
structs and symbols, the argument checks that need no device, and the host server's validation of the config key."""
import ctypes as C
import math

import pytest

from elevenrender_amd import abi, client, scenes

from test_host_server import Server


def test_adaptive_structs_match_the_header():
    assert C.sizeof(abi.ErAdaptiveParams) == 12
    assert C.sizeof(abi.ErAdaptiveInfo) == 6 * 4 + 8 + 4 + 4      # (the u64 is 8-aligned; the struct is padded to 8)
    assert abi.ErAdaptiveInfo.pixel_samples.offset == 24 and abi.ErAdaptiveInfo.max_active_error.offset == 32


def test_adaptive_symbols_are_exported_and_declared():
    lib = abi.load()
    for n in ("er_adaptive_set", "er_adaptive_info", "er_read_tile_state"):
        assert hasattr(lib, n) and n in abi.SYMBOLS


def test_adaptive_entry_points_validate_without_a_device():
    lib = abi.load()
    p = abi.ErAdaptiveParams(0.05, 16, 8)
    info = abi.ErAdaptiveInfo()
    err = (C.c_float * 4)()
    assert lib.er_adaptive_set(None, C.byref(p)) == abi.ER_ERR_INVALID_ARG
    assert lib.er_adaptive_info(None, C.byref(info)) == abi.ER_ERR_INVALID_ARG
    assert lib.er_read_tile_state(None, err, None) == abi.ER_ERR_INVALID_ARG
    sc = scenes.cornell(16, 16)
    h = C.c_void_p()
    assert lib.er_scene_create(C.byref(sc.desc()), C.byref(h)) == abi.ER_OK
    try:
        assert lib.er_adaptive_info(h, None) == abi.ER_ERR_INVALID_ARG
        # parameters are checked before the render state
        for bad in (abi.ErAdaptiveParams(-1.0, 16, 8), abi.ErAdaptiveParams(math.nan, 16, 8), abi.ErAdaptiveParams(0.1, 8, 8),
                    abi.ErAdaptiveParams(0.1, 4, 0), abi.ErAdaptiveParams(0.1, 0, 16)):
            assert lib.er_adaptive_set(h, C.byref(bad)) == abi.ER_ERR_INVALID_ARG, (bad.threshold, bad.min_samples, bad.interval)
        assert b"er_adaptive_set" in lib.er_last_error()
        # ... and a scene that has not been begun is a state error
        assert lib.er_adaptive_set(h, C.byref(p)) == abi.ER_ERR_STATE
        assert lib.er_adaptive_set(h, None) == abi.ER_ERR_STATE
        assert lib.er_adaptive_info(h, C.byref(info)) == abi.ER_ERR_STATE
        assert lib.er_read_tile_state(h, err, None) == abi.ER_ERR_STATE
    finally:
        lib.er_scene_destroy(h)


@pytest.mark.parametrize("bad,text", [
    ("yes", b"adaptive must be an object"),
    ({}, b"needs a threshold"),
    ({"threshold": -0.5}, b"threshold must be >= 0"),
    ({"threshold": "high"}, b"a number or"),
    ({"threshold": 0.1, "min_samples": 8, "interval": 8}, b"interval must be smaller"),
    ({"threshold": 0.1, "interval": 20}, b"interval must be smaller"),
    ({"threshold": 0.1, "min_samples": -3}, b"min_samples out of range"),
])
def test_host_rejects_a_malformed_adaptive_key(bad, text):
    s = Server()
    c = client.Client(port=s.port)
    base = dict(x_res=32, y_res=24, sample_target=2, denoise=False, device="", block_size=8)
    t, f, d = c.command("--load_config", client.Client._json(dict(base, adaptive=bad)))
    assert d.startswith(b"error:") and text in d, d
    # a well-formed key (threshold "inf" included) is accepted
    t, f, d = c.command("--load_config", client.Client._json(dict(base, adaptive={"threshold": "inf", "min_samples": 4, "interval": 2})))
    assert not d.startswith(b"error:"), d
    c.close()
    assert s.finish() == 0
