"""bench.py --dump-outputs without a GPU: dump_outputs() against a stand-in for the rendering manager that serves planes of
known contents, at a frame small enough to be written whole and at 1920x1080, which is written as a fixed sample of pixels."""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class FakeManager:
    """get_pass / get_render_info as render.RenderingManager returns them: (H, W, 4) float32 planes, a sample count."""

    def __init__(self, w, h, samples=7):
        self.scene = SimpleNamespace(x_res=w, y_res=h)
        self.samples = samples

    def get_pass(self, name):
        k = bench.DUMP_PLANES.index(name)
        px = np.arange(self.scene.x_res * self.scene.y_res, dtype=np.float32).reshape(self.scene.y_res, self.scene.x_res, 1)
        return (px * 4 + np.arange(4, dtype=np.float32) + k * 0.25).astype(np.float32)

    def get_render_info(self):
        return SimpleNamespace(samples=self.samples)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_a_small_frame_is_written_whole(tmp_path):
    rm = FakeManager(256, 192)
    names = bench.dump_outputs(rm, str(tmp_path))
    out = _load(tmp_path)
    assert sorted(names) == sorted(out) == ["beauty", "bitangent", "normal", "samples_done", "tangent"]
    for name in bench.DUMP_PLANES:
        assert out[name].dtype == np.float32 and np.array_equal(out[name], rm.get_pass(name))
    assert out["samples_done"].dtype == np.float64 and out["samples_done"].tolist() == [7.0]


def test_a_1080p_frame_is_a_fixed_sample_within_64_mb(tmp_path):
    rm = FakeManager(1920, 1080)
    bench.dump_outputs(rm, str(tmp_path / "a"))
    bench.dump_outputs(rm, str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["beauty", "bitangent", "normal", "pixel_index", "samples_done", "tangent"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    idx = a["pixel_index"]
    assert idx.dtype == np.float64 and idx.shape == (bench.DUMP_MAX_PIXELS,)
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < 1920 * 1080        # distinct pixels, in order
    for name in bench.DUMP_PLANES:
        assert a[name].dtype == np.float32 and a[name].shape == (bench.DUMP_MAX_PIXELS, 4)
        assert np.array_equal(a[name], rm.get_pass(name).reshape(-1, 4)[idx.astype(np.int64)])   # the planes' values at those pixels
    for name in a:                                                                          # the same sample every run
        assert a[name].tobytes() == b[name].tobytes(), name
