"""The numpy replay of a session that carries the variance through the history, shared by tests/test_history_variance_cpu.py and
tests/test_gpu_history_variance.py: the history test's scenes, object table and key planes (the oracle's entry points), variance.py
for the moments, history.py for the taps and the colour, history_variance.py for what is carried.  It is fed the BEAUTY and the sample
counts read at every fold point and before every capture, and says what every plane must then hold, word for word."""
import numpy as np

import test_gpu_history as gh
from elevenrender_amd import history, history_variance as hvar, variance

f32 = np.float32


def steps(name):
    """the sequence of three edits: a camera move that uncovers surfaces and turns the frame's edge in, a pose that uncovers more, then
    both -- chosen on the CPU with the replay alone (test_history_variance_cpu.py checks what they reach)"""
    sc = gh.scene(name)
    objects = gh.table(sc)
    dpos, rot, k = gh.PARAMS[name]
    s = lambda v, a: tuple(a * x for x in v)
    return [(gh.camera_of(sc, s(dpos, 0.5), s(rot, 0.5)), {}),
            (None, {0: gh.matrix(gh.rotation((0.1, 1.0, 0.0), 0.12 * k), t=(0.02, 0.0, 0.05), about=gh.object_centre(sc, objects, 0))}),
            (gh.camera_of(sc, dpos, rot), {2: gh.matrix(gh.rotation((0, 1, 0), 0.05), t=(0.12, 0.05, 0.0), about=gh.object_centre(sc, objects, 2))})]


class Replay:
    def __init__(self, name, max_weight=32.0, tol=0.02):
        self.st = gh.State(name)
        self.sc = self.st.sc
        self.npx = self.sc.x_res * self.sc.y_res
        self.max_weight, self.tol = max_weight, tol
        self.var = None             # the moments; None: K = 0 everywhere (never folded, or a restart is pending)
        self.allocated = False      # the scene has folded once: captures carry SV from then on
        self.cw = self.sv = self.old = None
        self.hist = self.hv = self.state = self.cls = self.tap_sv = None

    # -- what the session does --
    def fold(self, beauty, samples):
        if self.var is None:
            self.var = variance.start(self.npx)
        self.var, _ = variance.fold(self.var, beauty, samples)
        self.allocated = True

    def capture(self, beauty, samples):
        self.old = self.st.snapshot()
        self.cw = history.capture(beauty, samples, self.hist, self.max_weight)
        self.sv = hvar.capture(self.var, samples, self.hist, self.hv) if self.allocated else None
        self.hist = self.hv = None

    def edit(self, camera, poses):
        self.st.apply(camera, poses)
        self.var = None

    def resolve(self):
        old, new = self.old, self.st.snapshot()
        back, moved = history.back_table(old["poses"], new["poses"])
        k, ko = new["key"], old["key"]
        listed = (k["hit"] != 0) & (k["obj"] < len(back))
        o = np.where(listed, k["obj"], 0)
        px_back = np.where(listed[:, None], back[o], f32(0)).astype(f32)
        px_moved = np.where(listed, moved[o], 0).astype(np.uint32)
        args = (old["cam"], self.sc.x_res, self.sc.y_res, f32(self.tol), k["hit"], k["obj"], k["P"], px_moved, px_back, ko["hit"], ko["obj"], ko["dist"])
        self.hist, self.state, self.cls = history.resolve(*args, self.cw)
        self.hv = self.tap_sv = None
        if self.sv is not None:
            _, tw, q = hvar.taps(*args)
            self.tap_sv = self.sv[q]
            self.hv = hvar.mean(self.state, tw, self.tap_sv)
        return int(moved.sum())

    # -- what the planes then hold --
    def history_variance(self):
        return np.zeros((self.npx, 4), f32) if self.hv is None else self.hv

    def blended_variance(self, samples):
        return hvar.blend(self.var, samples, self.hist, self.hv)

    def denoise(self, beauty, samples, normal, albedo, depth, **kw):
        return hvar.denoise(beauty, samples, self.var, self.hist, self.hv, normal, albedo, depth, self.sc.x_res, self.sc.y_res, **kw)

    def known(self):
        """pixels whose flag is set: (captured SV, resolved HV)"""
        return (0 if self.sv is None else int((self.sv[:, 3] != 0).sum()), 0 if self.hv is None else int((self.hv[:, 3] != 0).sum()))

    def coverage(self):
        """after a resolve: pixels by how the carried variance reached them"""
        valid = self.state == history.TAP_VALID
        known_tap = valid & (self.tap_sv[:, :, 3] != 0)
        flag, w = self.hv[:, 3] != 0, self.hist[:, 3] > 0
        some_unknown = (valid & ~known_tap).any(1)
        return dict(all_known=int((flag & ~some_unknown).sum()), some_unknown=int((flag & some_unknown).sum()), none_known=int((~flag & w).sum()), no_history=int((~w).sum()))
