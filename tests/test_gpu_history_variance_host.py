"""The denoise of the blended frame behind eleven_server: `"history": true, "denoise_variance": true, "denoise_blended": true` in the
config.  After a camera-only --start the server holds a resolved history, and --get_pass denoise answers er_denoise_blended: it equals
the Python mirror's capture / update / resolve / render / features / denoise_blended sequence word for word, with alpha 1.  --get_pass
beauty and --get_pass blended are what they were, --get_info counts blended_denoises, and the key without its two prerequisites is
refused."""
import numpy as np
import pytest

from elevenrender_amd import client, render
from test_gpu_history_host import CAMERAS, session_camera, wait_for
from test_host_server import Server, session_scene

pytestmark = pytest.mark.gpu

SAMPLES, BATCH = 6, 2      # folds at 2, 4 and 6 samples of either frame
KEYS = dict(history=True, denoise_variance=True, denoise_blended=True)
same = lambda a, b: bool((a.view(np.uint32) == b.view(np.uint32)).all())


def test_denoise_through_the_server_is_the_blended_filter_after_a_camera_update(tmp_path):
    a = client.cornell_session_assets(48, 48)
    s = Server()
    c = client.Client(port=s.port)
    client.play_cornell_session(c, a, sample_target=SAMPLES, **KEYS)
    wait_for(c, SAMPLES)
    first = c.get_pass("denoise", 48, 48)                  # no resolved history yet: er_denoise_variance, as without the key
    assert c.get_info()["blended_denoises"] == 0
    c.load_camera(**CAMERAS[0])
    c.start()                                              # camera only: capture, update, resolve
    wait_for(c, SAMPLES)
    den, beauty, blended = c.get_pass("denoise", 48, 48), c.get_pass("beauty", 48, 48), c.get_pass("blended", 48, 48)
    info = c.get_info()
    assert same(c.get_pass("denoise", 48, 48), den)
    assert c.get_info()["blended_denoises"] == 2
    c.close()
    assert s.finish() == 0
    assert info["blended_denoises"] == 1 and info["history_resolves"] == 1 and info["variance_folds"] == SAMPLES // BATCH and info["samples"] == SAMPLES + 1
    # the same sequence through the Python mirror
    sc = session_scene(a, tmp_path)
    rm = render.RenderingManager(render.RenderParameters())
    rm.start_rendering(sc)
    try:
        rm.render(SAMPLES, fold_every=BATCH)
        rm.render_features()
        rm.denoise_variance()
        want_first = rm.get_pass("denoise")
        want_first[..., 3] = 1.0
        assert same(first, want_first)
        rm.history_capture()
        rm.update(camera=session_camera(sc, **CAMERAS[0]))
        rm.history_resolve()
        rm.render(SAMPLES, fold_every=BATCH)
        rm.render_features()
        rm.denoise_blended()
        want = rm.get_pass("denoise")
        assert (want[..., 3] == 1).all()                   # (the blend's alpha: the server's answer has alpha 1 either way)
        assert same(den, want)
        assert same(beauty, rm.get_pass("beauty")) and same(blended, rm.get_blended())
        assert (den[..., :3] != blended[..., :3]).any() and rm.history_variance_info()["pixels_known_blended"] > 0
        rm.denoise_variance()
        assert not same(den[..., :3].copy(), rm.get_pass("denoise")[..., :3].copy())      # not the plain frame's filter
    finally:
        rm.close()
    # the key without its two prerequisites, or on two GPUs, is refused
    for keys in (dict(denoise_blended=True), dict(denoise_blended=True, history=True), dict(denoise_blended=True, denoise_variance=True),
                 dict(KEYS, gpus=2)):
        s = Server()
        c = client.Client(port=s.port)
        with pytest.raises(client.ProtocolError) as e:
            c.load_config(48, 48, SAMPLES, **keys)
        assert "denoise_blended" in str(e.value) or "gpus 1" in str(e.value)
        c.close()
        assert s.finish() == 0
    # the two prerequisites without the key answer as before: the plain frame's filter, no blended_denoises
    s = Server()
    c = client.Client(port=s.port)
    client.play_cornell_session(c, a, sample_target=SAMPLES, history=True, denoise_variance=True)
    wait_for(c, SAMPLES)
    c.load_camera(**CAMERAS[0])
    c.start()
    wait_for(c, SAMPLES)
    plain_den, plain_beauty = c.get_pass("denoise", 48, 48), c.get_pass("beauty", 48, 48)
    assert "blended_denoises" not in c.get_info()
    c.close()
    assert s.finish() == 0
    assert same(plain_beauty, beauty) and not same(plain_den, den)
