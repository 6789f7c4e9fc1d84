#!/usr/bin/env python3
"""Counted cost of the C2 frame per 8 x 8 tile and per sample, from the CPU oracle (analysis helper, not a test).

What the streaming schedule's deal of tiles to workgroups needs to know about a frame: how unevenly the bounce-loop iterations -- the
unit the kernel itself counts per tile while a render's first call runs (DevScene::tile_cost) -- are spread over the tiles, and how
well one sample's counts predict the next one's (csrc/er_stream_host.cpp er_stream_level_by_cost; NOTEBOOK.md).

Eight single-thread oracles, each taking every eighth pixel row in segments of 8 pixels (one tile's width), read
counters()["bounce_samples"] before and after each segment: every pixel of the frame, reference BVH, MATH_ER, 8 bounces.

    python3 tests/analysis_tile_cost.py [samples [out.npz]]      -> tests/golden/c2_tile_cost_2spp.npz by default; minutes on 8 cores

The file holds `cost`: uint16 [samples, tiles_y, tiles_x] (a tile of 64 pixels x at most 9 iterations stays below 1 024).
"""
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle  # noqa: E402
from elevenrender_amd import scenes  # noqa: E402

WORKERS = 8


def main():
    ns = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "c2_tile_cost_2spp.npz")
    sc = scenes.soup(1_000_000, 1920, 1080, seed=12345)
    w, h = sc.x_res, sc.y_res
    tiles_x, tiles_y = (w + 7) // 8, (h + 7) // 8
    cost = np.zeros((WORKERS, ns, tiles_y, tiles_x), np.int64)

    def run(r):
        o = oracle.Oracle(sc, math_mode=oracle.MATH_ER, max_bounces=8, threads=1)
        for s in range(ns):                       # (a pixel's samples are one RNG stream: sample s of every segment before sample s + 1 of any)
            for y in range(r, h, WORKERS):
                for tx in range(tiles_x):
                    i0 = y * w + tx * 8
                    before = o.counters()["bounce_samples"]
                    o.render(1, i0, min(i0 + 8, (y + 1) * w))
                    cost[r, s, y // 8, tx] += o.counters()["bounce_samples"] - before
        o.close()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(WORKERS)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    cost = cost.sum(0)
    assert cost.max() <= 1024
    print(f"C2, {w} x {h}, {ns} samples: {cost.sum()} bounce-loop iterations, {cost.sum() / (ns * w * h):.3f} per sample; "
          f"per tile std / mean {cost.sum(0).std() / cost.sum(0).mean():.3f}")
    if ns >= 2:
        print(f"per-tile correlation of sample 1 and sample 2: {np.corrcoef(cost[0].ravel(), cost[1].ravel())[0, 1]:.3f}")
    np.savez_compressed(out, cost=cost.astype(np.uint16))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
