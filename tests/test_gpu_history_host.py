"""Temporal reprojection behind eleven_server: `"history": true` in the config, two camera loads each followed by --start (the
camera-update path: capture before, resolve after).  --get_pass blended equals get_blended() of the same sequence through the Python
mirror, word for word; --get_pass beauty is what it was; --get_info reports history_resolves."""
import time

import numpy as np
import pytest

from elevenrender_amd import abi, client, render
from test_host_server import Server, session_scene

pytestmark = pytest.mark.gpu

CAMERAS = (dict(position=(0.05, -0.03, -1.55), rotation=(0.5, -1.5, 0.0)), dict(position=(0.1, -0.05, -1.6), rotation=(1.0, -3.0, 0.0)))
SAMPLES = 4


def wait_for(c, samples):
    deadline = time.time() + 120
    while c.get_info()["samples"] < samples + 1:      # (every poll is a round trip to the server: no sleep between them)
        assert time.time() < deadline, "render did not reach the sample target"


def session_camera(sc, position, rotation):
    cam = abi.ErCamera.from_buffer_copy(sc.camera)
    cam.position, cam.rotation = abi.ErVec3(*position), abi.ErVec3(*rotation)
    return cam


def test_blended_through_the_server_equals_the_python_sequence(tmp_path):
    a = client.cornell_session_assets(48, 48)
    s = Server()
    c = client.Client(port=s.port)
    client.play_cornell_session(c, a, sample_target=SAMPLES, history=True)
    assert c.get_info()["history_resolves"] == 0
    with pytest.raises(client.ProtocolError):
        c.get_pass("blended", 48, 48)                     # nothing resolved yet
    got = []
    for cam in CAMERAS:
        c.load_camera(**cam)
        c.start()
        wait_for(c, SAMPLES)
        got.append((c.get_pass("blended", 48, 48), c.get_pass("beauty", 48, 48)))
    info = c.get_info()
    c.close()
    assert s.finish() == 0
    assert info["history_resolves"] == 2 and info["camera_updates"] == 2 and info["samples"] == SAMPLES + 1
    # the same sequence through the Python mirror
    sc = session_scene(a, tmp_path)
    rm = render.RenderingManager(render.RenderParameters())
    rm.start_rendering(sc)
    try:
        rm.render(SAMPLES)
        for (blended, beauty), cam in zip(got, CAMERAS):
            rm.update(camera=session_camera(sc, **cam), keep_history=True)
            rm.render(SAMPLES)
            assert (blended.view(np.uint32) == rm.get_blended().view(np.uint32)).all()
            assert (beauty.view(np.uint32) == rm.get_pass("beauty").view(np.uint32)).all()
            assert (blended[..., 3] == 1).all() and (blended[..., :3] != beauty[..., :3]).any()
    finally:
        rm.close()
    # a session without the key answers as before: no blended pass, no history_resolves
    s = Server()
    c = client.Client(port=s.port)
    plain = client.play_cornell_session(c, a, sample_target=SAMPLES)
    c.load_camera(**CAMERAS[0])
    c.start()
    wait_for(c, SAMPLES)
    moved = c.get_pass("beauty", 48, 48)
    assert "history_resolves" not in c.get_info()
    with pytest.raises(client.ProtocolError):
        c.get_pass("blended", 48, 48)
    c.close()
    assert s.finish() == 0
    assert plain.shape == moved.shape and (moved.view(np.uint32) == got[0][1].view(np.uint32)).all()      # beauty is unchanged by the key
