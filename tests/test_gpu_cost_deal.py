"""The streaming schedule's deal levelled by counted cost, on the GPU (csrc/er_stream_host.cpp stream_adapt, er_stream_level_by_cost).

While a render's first call runs the kernel adds every finished path's length to its tile's sum; after the first sample (a launch of its
own) the library takes the 8 x 8 or the 16 x 16 super-tile deal as before and then levels the one taken by those counts, and once more
when the first call has completed; ER_STREAM_COST_LEVEL=0 keeps the count deal.  Any deal renders the same pixels, so everything here is
bit-equality plus what er_debug_stream_balance reports about the deal in use -- counts, never clocks, except that a workgroup's end stamp
lies between the launch's start and the latest XCD's end."""
import contextlib
import os

import numpy as np
import pytest

from elevenrender_amd import abi, render, scenes

pytestmark = pytest.mark.gpu

PLANES = ("beauty", "normal", "tangent", "bitangent")
NONE = 0xFFFFFFFF
SPP = 12


@contextlib.contextmanager
def environment(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def uneven_frame():
    """the frame of test_deal_is_decided_by_counted_work...: a soup seen from far away -- geometry in the middle, sky around it"""
    sc = scenes.soup(60_000, 1280, 832, seed=31, hdri_size=(256, 128))
    sc.camera.position = abi.ErVec3(0.01, 0.02, -3.0)
    sc._desc = None
    return sc


def stream_render(sc, chunks, level, adaptive=None, **kw):
    with environment(ER_STREAM_COST_LEVEL=None if level else "0"):
        rm = render.RenderingManager(render.RenderParameters(max_bounces=8, **kw))
        rm.start_rendering(sc)
        if adaptive:
            rm.set_adaptive(*adaptive)
        for n in chunks:
            rm.render(n)
        out = {p: rm.get_pass(p) for p in PLANES}
        out["samples"], out["rng"] = rm.read_samples(), rm.read_rng()
        if kw.get("flags") == abi.FLAG_STREAM:
            out["info"], out["balance"] = rm.stream_info(), rm.stream_balance()
        if adaptive:
            out["adaptive"] = rm.adaptive_info()
            out["error"], _ = rm.tile_state()
        rm.close()
    return out


def same_image(a, b, what):
    for p in PLANES:
        assert (a[p].view(np.uint32) == b[p].view(np.uint32)).all(), (what, p)
    assert (a["samples"] == b["samples"]).all() and (a["rng"] == b["rng"]).all(), what


def spread(deal, tile_cost):
    """max / mean of the counted cost per workgroup of a deal ([most, blocks]) under the given tile costs, over the workgroups that own a tile"""
    c = np.concatenate([tile_cost.astype(np.uint64), [0]])
    per = c[np.where(deal == NONE, len(c) - 1, deal)].sum(0)
    per = per[(deal != NONE).any(0)]
    return float(per.max()) / float(per.mean())


@pytest.fixture(scope="module")
def frame():
    return uneven_frame()


@pytest.fixture(scope="module")
def wavefront(frame):
    return stream_render(frame, [SPP], True, flags=abi.FLAG_WAVEFRONT)


_runs = {}


def run(frame, chunks, level):
    """(cached: the image test, the repeat and the finish stamps look at the same renders)"""
    key = (tuple(chunks), level)
    if key not in _runs:
        _runs[key] = stream_render(frame, chunks, level, flags=abi.FLAG_STREAM)
    return _runs[key]


@pytest.mark.parametrize("chunks", [[8, 2, 2], [12]])
def test_levelled_deal_renders_the_same_image_and_spreads_the_counted_cost_better(frame, wavefront, chunks):
    on, off = run(frame, chunks, True), run(frame, chunks, False)
    again = stream_render(frame, chunks, True, flags=abi.FLAG_STREAM)
    for other, what in ((on, "levelled"), (off, "ER_STREAM_COST_LEVEL=0"), (again, "levelled, second run")):
        same_image(wavefront, other, what)
    b_on, b_off = on["balance"], off["balance"]
    n_tiles = (1280 // 8) * (832 // 8)
    assert b_on["levelled"] == 1 and b_off["levelled"] == 0 and b_on["counting"] == b_off["counting"] == 0
    assert on["info"]["deal_pending"] == 0 and on["info"]["large_regions"] == off["info"]["large_regions"]
    for b in (b_on, b_off):          # the deal in use is a partition of the owned tiles, within the cap
        got = b["deal"][b["deal"] != NONE]
        assert len(got) == n_tiles and (np.sort(got) == np.arange(n_tiles)).all()
        assert ((b["deal"] != NONE).sum(0) == b["wg_tiles"]).all() and b["wg_tiles"].max() <= b["cap"] and b["most"] <= b["cap"]
    # counted, not timed: the same counts and the same deal on every run
    assert (b_on["tile_cost"] == again["balance"]["tile_cost"]).all() and b_on["deal"].tobytes() == again["balance"]["deal"].tobytes()
    assert b_on["cost_tiles"] == n_tiles and b_on["tile_cost"].min() > 0
    # on the counts of the whole first call the levelled deal is more even than the count deal it was made from
    # (ER_STREAM_COST_LEVEL=0 leaves that one in use: the same decision between the two super-tile sizes)
    levelled, count = spread(b_on["deal"], b_on["tile_cost"]), spread(b_off["deal"], b_on["tile_cost"])
    reported = float(b_on["wg_cost"].max()) / float(b_on["wg_cost"].mean())
    print(f"chunks {chunks}: counted cost per workgroup max / mean {count:.4f} under the count deal, {levelled:.4f} levelled; {b_on['wg_tiles'].min()} ... {b_on['wg_tiles'].max()} tiles")
    assert abs(reported - levelled) < 1e-9
    assert levelled < count


def test_every_workgroup_reports_an_end_between_the_launchs_start_and_the_latest_xcd(frame):
    """After a call of >= 4 samples (here: the 11 that follow the first sample's own launch) every workgroup that owns a tile has
    stamped its end: after the launch's start, not after the latest XCD's end.  Nothing else about clocks is asserted."""
    for level in (True, False):
        b = run(frame, [12], level)["balance"]
        owners = b["wg_tiles"] > 0
        assert owners.all() and b["launch_ticks"] > 0
        assert (b["wg_ticks"][owners] > 0).all() and (b["wg_ticks"][owners] <= b["launch_ticks"]).all()


def test_adaptive_redeal_leaves_no_levelled_deal(frame):
    """Adaptive sampling (min_samples 4, interval 2 -- the interval must be smaller than min_samples --, the median tile error of the first test as threshold: about half the tiles stop):
    the active share is dealt by count as before -- the hook reports a count deal of the active tiles, the counting has stopped -- and
    the image is that of ER_STREAM_COST_LEVEL=0."""
    first = stream_render(frame, [4], True, adaptive=(0.0, 4, 2), flags=abi.FLAG_STREAM)
    e = first["error"][first["error"] >= 0]
    threshold = float(np.median(e))
    on = stream_render(frame, [8], True, adaptive=(threshold, 4, 2), flags=abi.FLAG_STREAM)
    off = stream_render(frame, [8], False, adaptive=(threshold, 4, 2), flags=abi.FLAG_STREAM)
    same_image(on, off, "adaptive")
    a, b = on["adaptive"], on["balance"]
    assert 0 < a["active_tiles"] < a["owned_tiles"] and a["tests_done"] >= 2
    assert b["levelled"] == 0 and b["counting"] == 0
    assert (b["deal"] != NONE).sum() == a["active_tiles"] and b["deal"].tobytes() == off["balance"]["deal"].tobytes()


def test_share_of_rank_1_of_2_renders_the_same_pixels(frame):
    on = stream_render(frame, [SPP], True, flags=abi.FLAG_STREAM, rank=1, world=2)
    off = stream_render(frame, [SPP], False, flags=abi.FLAG_STREAM, rank=1, world=2)
    same_image(on, off, "rank 1 of 2")
    b = on["balance"]
    got = b["deal"][b["deal"] != NONE]
    assert b["levelled"] == 1 and len(got) == len(np.unique(got)) == (off["balance"]["deal"] != NONE).sum()
    assert (np.sort(got) == np.sort(off["balance"]["deal"][off["balance"]["deal"] != NONE])).all()
    assert spread(b["deal"], b["tile_cost"]) < spread(off["balance"]["deal"], b["tile_cost"])
