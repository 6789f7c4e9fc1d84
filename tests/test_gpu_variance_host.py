"""The variance plane behind eleven_server: `"denoise_variance": true, "variance_batch": 2` in the config.  The render thread cuts its
calls at multiples of the batch and folds there, so --get_pass variance and --get_pass denoise equal the direct-ABI results of the same
fold points through the Python mirror word for word, however the thread sized its calls; --get_pass beauty is what it was; --get_info
reports variance_folds."""
import time

import numpy as np
import pytest

from elevenrender_amd import client, render
from test_host_server import Server, session_scene

pytestmark = pytest.mark.gpu

SAMPLES, BATCH = 7, 2      # folds at 2, 4 and 6 samples; the seventh sample changes M, not the moments


def wait_for(c, samples):
    deadline = time.time() + 120
    while c.get_info()["samples"] < samples + 1:      # (every poll is a round trip to the server: no sleep between them)
        assert time.time() < deadline, "render did not reach the sample target"


def test_variance_and_denoise_through_the_server_equal_the_python_sequence(tmp_path):
    a = client.cornell_session_assets(48, 48)
    s = Server()
    c = client.Client(port=s.port)
    client.play_cornell_session(c, a, sample_target=SAMPLES, denoise_variance=True, variance_batch=BATCH)
    wait_for(c, SAMPLES)
    info = c.get_info()
    var, den, beauty = c.get_pass("variance", 48, 48), c.get_pass("denoise", 48, 48), c.get_pass("beauty", 48, 48)
    c.close()
    assert s.finish() == 0
    assert info["variance_folds"] == SAMPLES // BATCH and info["samples"] == SAMPLES + 1
    # the same fold points through the Python mirror
    sc = session_scene(a, tmp_path)
    rm = render.RenderingManager(render.RenderParameters())
    rm.start_rendering(sc)
    try:
        rm.render(SAMPLES, fold_every=BATCH)
        assert rm.variance_info()["folds"] == SAMPLES // BATCH
        want_var = rm.get_variance()
        rm.render_features()
        rm.denoise_variance()
        want_den = rm.get_pass("denoise")
        want_den[..., 3] = 1.0                                                               # (the server answers a denoised pass with alpha 1)
        assert (var.view(np.uint32) == want_var.view(np.uint32)).all()
        assert (den.view(np.uint32) == want_den.view(np.uint32)).all()
        assert (beauty.view(np.uint32) == rm.get_pass("beauty").view(np.uint32)).all()
        assert (var[..., 3] == SAMPLES // BATCH).all() and (var[..., :3] > 0).any() and (den[..., :3] != beauty[..., :3]).any()
    finally:
        rm.close()
    # a batch of 0 is the default, 2: the same plane
    s = Server()
    c = client.Client(port=s.port)
    client.play_cornell_session(c, a, sample_target=SAMPLES, denoise_variance=True)
    wait_for(c, SAMPLES)
    again = c.get_pass("variance", 48, 48)
    c.close()
    assert s.finish() == 0
    assert (again.view(np.uint32) == var.view(np.uint32)).all()
    # a session without the key answers as before: no variance pass, no variance_folds, the same beauty
    s = Server()
    c = client.Client(port=s.port)
    client.play_cornell_session(c, a, sample_target=SAMPLES)
    wait_for(c, SAMPLES)
    assert "variance_folds" not in c.get_info()
    with pytest.raises(client.ProtocolError):
        c.get_pass("variance", 48, 48)
    plain = c.get_pass("beauty", 48, 48)
    c.close()
    assert s.finish() == 0
    assert (plain.view(np.uint32) == beauty.view(np.uint32)).all()
