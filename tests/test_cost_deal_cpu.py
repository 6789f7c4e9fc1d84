"""The streaming schedule's deal of tiles to workgroups, levelled by counted cost (csrc/er_stream_host.cpp er_stream_level_by_cost, through
er_debug_stream_level of include/eleven_hip_debug.h: host code, no device).  A launch lasts as long as its slowest workgroup, and the count
deal (er_stream_deal_tiles) gives every workgroup the same positions of every super-tile: on a frame with structure the same workgroups
are heavy in every sample.  The levelled deal moves the tail tiles of the costliest XCD to the cheapest and then, inside each XCD, deals
heaviest tile first to the lightest workgroup that is under the cap of tiles (the pixel rings do not grow)."""
import ctypes as C
import os

import numpy as np
import pytest

from elevenrender_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
U = C.POINTER(C.c_uint32)
BLOCKS = 256


def count_deal(owned, tiles_x, blocks=BLOCKS, xcd_aware=1, edge=8):
    lib = abi.load()
    lib.er_debug_stream_deal.argtypes = [U, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, U, C.c_uint32, U]
    lib.er_debug_stream_deal.restype = C.c_int
    owned = np.ascontiguousarray(owned, np.uint32)
    most = C.c_uint32()
    lib.er_debug_stream_deal(owned.ctypes.data_as(U), len(owned), tiles_x, blocks, xcd_aware, edge, None, 0, C.byref(most))
    out = np.zeros(blocks * most.value, np.uint32)
    assert lib.er_debug_stream_deal(owned.ctypes.data_as(U), len(owned), tiles_x, blocks, xcd_aware, edge, out.ctypes.data_as(U), len(out), C.byref(most)) == abi.ER_OK
    return out.reshape(most.value, blocks)          # [k, b] = the k-th tile of workgroup b


def level(deal, tiles_x, cost, cap, blocks=BLOCKS):
    lib = abi.load()
    deal = np.ascontiguousarray(deal, np.uint32).ravel()
    cost = np.ascontiguousarray(cost, np.uint32).ravel()
    most = C.c_uint32()
    args = (deal.ctypes.data_as(U), len(deal), tiles_x, blocks, cost.ctypes.data_as(U), len(cost), cap)
    lib.er_debug_stream_level(*args, None, 0, C.byref(most))
    out = np.zeros(blocks * most.value, np.uint32)
    assert lib.er_debug_stream_level(*args, out.ctypes.data_as(U), len(out), C.byref(most)) == abi.ER_OK
    return out.reshape(most.value, blocks)


def ring_cap_tiles(deal):
    """the cap stream_begin gives: cells of a pixel ring (a power of two >= 64 x the deal's largest share) / 64"""
    cap = 1
    while cap < deal.shape[0]:
        cap *= 2
    return cap


def wg_cost(deal, cost):
    c = np.concatenate([np.asarray(cost, np.uint64).ravel(), [0]])
    return c[np.where(deal == NONE, len(c) - 1, deal)].sum(0)          # [b]


def xcd_sequences(deal):
    """the XCDs' tile sequences in the order er_stream_deal_tiles dealt them (workgroup b is on XCD b % 8)"""
    most, blocks = deal.shape
    return [[int(t) for k in range(most) for t in deal[k, x::8] if t != NONE] for x in range(8)]


def cost_maps(tiles_x, tiles_y):
    ty, tx = np.mgrid[0:tiles_y, 0:tiles_x]
    r = np.random.RandomState(7)
    spike = np.full((tiles_y, tiles_x), 3, np.uint32)
    spike[tiles_y // 3, tiles_x // 2] = 3000
    return {
        "vertical gradient": (64 + 8 * ty).astype(np.uint32),
        "sky over ground": np.where(ty < tiles_y // 2, 1, 500).astype(np.uint32),
        "seeded random": r.randint(64, 577, (tiles_y, tiles_x)).astype(np.uint32),
        "all zero": np.zeros((tiles_y, tiles_x), np.uint32),
        "one tile 1000 x the rest": spike,
    }


def shares(tiles_x, tiles_y):
    ty, tx = np.mgrid[0:tiles_y, 0:tiles_x]
    every = np.arange(tiles_x * tiles_y, dtype=np.uint32)
    return {
        "whole frame": (every, 1),
        "rank 1 of 3": (every[((tx + ty) % 3 == 1).ravel()], 1),
        "fewer tiles than workgroups": (every[5:5 + 100], 0),          # (a share this small is dealt round-robin: stream_xcd_aware)
    }


@pytest.mark.parametrize("edge", [8, 16])
@pytest.mark.parametrize("tiles_x,tiles_y", [(50, 30), (240, 135)])
def test_levelled_deal_is_a_partition_within_the_cap_and_the_xcds_and_greedy(tiles_x, tiles_y, edge):
    """Every owned tile exactly once; no workgroup over the cap; a tile leaves its base deal's XCD only as part of the tail of that XCD's
    sequence (what the XCD levelling moves); inside every XCD whose workgroups are all under the cap the largest workgroup cost is at most
    the XCD's mean + its largest tile (the greedy rule's guarantee); all-zero costs give the input back byte for byte; two calls give the
    same bytes."""
    unbound = 0
    for share, (owned, xcd_aware) in shares(tiles_x, tiles_y).items():
        base = count_deal(owned, tiles_x, xcd_aware=xcd_aware, edge=edge)
        cap = ring_cap_tiles(base)
        for name, cost in cost_maps(tiles_x, tiles_y).items():
            what = (share, name)
            lv = level(base, tiles_x, cost, cap)
            assert (level(base, tiles_x, cost, cap) == lv).all(), what
            if name == "all zero":
                assert lv.shape == base.shape and lv.tobytes() == base.tobytes(), what
                continue
            got = lv[lv != NONE]
            assert len(got) == len(owned) and (np.sort(got) == np.sort(owned)).all(), what
            assert lv.shape[0] <= cap and ((lv != NONE).sum(0) <= cap).all(), what
            for b in range(BLOCKS):          # a workgroup's tiles in ascending order, none after the first gap
                mine = lv[:, b]
                n = int((mine != NONE).sum())
                assert (mine[:n] != NONE).all() and (np.diff(mine[:n].astype(np.int64)) > 0).all(), what
            seq_base, seq_lv = xcd_sequences(base), xcd_sequences(lv)
            flat = cost.ravel().astype(np.int64)
            for x in range(8):
                stayed = set(seq_lv[x])
                gone = [t not in stayed for t in seq_base[x]]
                assert gone == sorted(gone), (what, x)          # (False ... False True ... True: only a tail left)
                per_wg = wg_cost(lv, cost)[x::8].astype(np.int64)
                if seq_lv[x] and ((lv != NONE).sum(0)[x::8] < cap).all():
                    unbound += 1
                    assert per_wg.max() * len(per_wg) <= per_wg.sum() + flat[seq_lv[x]].max() * len(per_wg), (what, x)
            # the XCD levelling: the costliest XCD is no costlier than before
            xb = [flat[s].sum() for s in seq_base]
            xl = [flat[s].sum() for s in seq_lv]
            assert max(xl) <= max(xb), what
    assert unbound > 0


def test_levelling_rejects_bad_arguments():
    lib = abi.load()
    most = C.c_uint32()
    deal = np.zeros(256, np.uint32)
    cost = np.ones(4, np.uint32)
    d, c = deal.ctypes.data_as(U), cost.ctypes.data_as(U)
    assert lib.er_debug_stream_level(d, 256, 2, 0, c, 4, 1, None, 0, C.byref(most)) == abi.ER_ERR_INVALID_ARG          # no workgroups
    assert lib.er_debug_stream_level(d, 255, 2, 256, c, 4, 1, None, 0, C.byref(most)) == abi.ER_ERR_INVALID_ARG        # not blocks x most entries
    assert lib.er_debug_stream_level(d, 256, 2, 256, c, 4, 0, None, 0, C.byref(most)) == abi.ER_ERR_INVALID_ARG        # no cap
    assert lib.er_debug_stream_level(d, 256, 2, 256, c, 4, 1, None, 0, None) == abi.ER_ERR_INVALID_ARG


@pytest.mark.parametrize("edge", [8, 16])
def test_c2_frame_counted_by_the_oracle_is_levelled_from_one_sample(edge):
    """tests/golden/c2_tile_cost_2spp.npz (tests/analysis_tile_cost.py): the bounce-loop iterations of the C2 frame per 8 x 8 tile for
    sample 1 and sample 2 of every pixel, counted by the CPU oracle.  On 256 workgroups the count deal leaves the costliest workgroup
    >= 1.03 of the mean on the sum of both samples (1.037 at edge 8, 1.040 at edge 16); the deal levelled on sample 1 ALONE and judged on
    sample 2 is <= 1.03 (1.017 ... 1.020, of which about 1.013 is the one-sample judge's own noise) and below the count deal judged on
    the same sample."""
    cost = np.load(os.path.join(ROOT, "tests", "golden", "c2_tile_cost_2spp.npz"))["cost"].astype(np.uint32)
    assert cost.shape == (2, 135, 240) and cost.max() <= 1024
    base = count_deal(np.arange(135 * 240, dtype=np.uint32), 240, edge=edge)
    assert base.shape[0] == 127 and ring_cap_tiles(base) == 128
    ratio = lambda deal, c: float(wg_cost(deal, c).max()) / float(wg_cost(deal, c).mean())
    both = ratio(base, cost[0] + cost[1])
    lv = level(base, 240, cost[0], 128)
    count_2, level_2 = ratio(base, cost[1]), ratio(lv, cost[1])
    tiles = (lv != NONE).sum(0)
    print(f"edge {edge}: count deal max / mean {both:.4f} on both samples, {count_2:.4f} on sample 2; levelled on sample 1: {ratio(lv, cost[0]):.4f} on sample 1, "
          f"{level_2:.4f} on sample 2, {tiles.min()} ... {tiles.max()} tiles per workgroup")
    assert both >= 1.03
    assert level_2 <= 1.03 and level_2 < count_2
