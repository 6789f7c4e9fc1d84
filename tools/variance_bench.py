#!/usr/bin/env python3
"""What the variance plane and the filter guided by it cost and what they buy (er_variance_fold / er_denoise_variance).

Cost: the 1 M-triangle soup at 1280x720 and 1920x1080, the variants alternated in one process, medians of 7 rounds: fold_ms and filter_ms
(device time, ErVarianceInfo; 5 levels) beside er_denoise_guided (5 levels, the yardstick; wall time of the call, which waits for the
device) and one er_render_samples(1) (wall).  er_denoise_variance's wall time is printed too, so that the two filters are compared by
the same clock.

Quality: cornell_textured 256x256 and the C5-style frame (torture, 1 M triangles, 1280x720) at 4, 16 and 64 spp in folds of 2: the mean
absolute error against 1 024 spp of the unfiltered frame, er_denoise_guided at its defaults and at the best colour_sigma of a sweep, and
er_denoise_variance at colour_sigma 2, 3, 4 and 6; every image scaled by samples / (samples - 1) (the setup sample).

EXPECTATION, written before the first run: the fold moves about 64 bytes in and 48 out per pixel (BEAUTY's float4 sits in a 64-byte
group of the interleaved passes), 0.23 GB at 1080p: tens of microseconds.  A level adds 9 + 25 sixteen-byte loads and one store to the
guided kernel's 100 loads, and three divisions per tap to its four: something like 1.3 - 1.6 x er_denoise_guided.  Above 2 x, say where
the time goes before anything else is done about it.  For quality the variance-normalised stop should win where the noise is uneven
(the Cornell box: direct light beside two-bounce corners) from 16 spp on; at 4 spp K = 2, the estimate has one degree of freedom, and
it may not.

    python tools/variance_bench.py [--quick] > profiles/variance_bench.log
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from elevenrender_amd import render, scenes  # noqa: E402

GUIDED_SWEEP = (0.5, 1.0, 2.0, 4.0, 8.0, 16.0)
VARIANCE_SWEEP = (2.0, 3.0, 4.0, 6.0)


def wall_ms(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def cost(n_tris, rounds):
    frames = {"720p": (1280, 720), "1080p": (1920, 1080)}
    keys = ("fold_ms", "variance_filter_ms", "variance_filter_wall_ms", "guided_filter_wall_ms", "sample1_ms")
    rms, rows = {}, {k: {m: [] for m in keys} for k in frames}
    for name, (w, h) in frames.items():
        sc = scenes.soup(n_tris, w, h)
        rm = render.RenderingManager(render.RenderParameters())
        rm.start_rendering(sc)
        rm.render(4, fold_every=2)
        rm.render_features()
        rms[name] = rm
    for r in range(rounds + 1):      # (round 0 warms up and allocates)
        for name, rm in rms.items():
            s1 = wall_ms(lambda: rm.render(1))
            rm.variance_fold()
            fold = rm.variance_info()["fold_ms"]
            vw = wall_ms(lambda: rm.denoise_variance(levels=5))
            vf = rm.variance_info()["filter_ms"]
            gw = wall_ms(lambda: rm.denoise_guided(levels=5))
            if r:
                for k, v in zip(keys, (fold, vf, vw, gw, s1)):
                    rows[name][k].append(v)
    for name, rm in rms.items():
        info = rm.variance_info()
        rm.close()
        med = {k: statistics.median(v) for k, v in rows[name].items()}
        print(f"cost {name} soup {n_tris} triangles, medians of {rounds}: " + ", ".join(f"{k} {v:.3f}" for k, v in med.items())
              + f"; variance / guided (wall) {med['variance_filter_wall_ms'] / med['guided_filter_wall_ms']:.2f}")
        print(f"     last fold: {info}")


def quality(label, sc):
    rm = render.RenderingManager(render.RenderParameters())
    rm.start_rendering(sc)
    rm.render_features()
    shots, done = {}, 0
    for spp in (4, 16, 64):
        rm.render(spp - done, fold_every=2)
        done = spp
        scale = (spp + 1.0) / spp
        grab = lambda name: rm.get_pass(name)[..., :3].astype(np.float64) * scale
        row = {"unfiltered": grab("beauty")}
        rm.denoise_guided()
        row["guided"] = grab("denoise")
        for s in GUIDED_SWEEP:
            rm.denoise_guided(colour_sigma=s)
            row[("guided", s)] = grab("denoise")
        for s in VARIANCE_SWEEP:
            rm.denoise_variance(colour_sigma=s)
            row[("variance", s)] = grab("denoise")
        shots[spp] = row
    rm.render(1024 - done)
    truth = rm.get_pass("beauty")[..., :3].astype(np.float64) * (1025.0 / 1024.0)
    rm.close()
    err = lambda a: float(np.abs(a - truth).mean())
    print(f"quality {label}: mean absolute error against 1024 spp")
    print("     spp  unfiltered  guided(default)  guided(best sigma)  " + "  ".join(f"variance({s:g})" for s in VARIANCE_SWEEP))
    for spp, row in shots.items():
        best = min(GUIDED_SWEEP, key=lambda s: err(row[("guided", s)]))
        print(f"     {spp:3d}  {err(row['unfiltered']):.5f}     {err(row['guided']):.5f}          {err(row[('guided', best)]):.5f} ({best:g})      "
              + "      ".join(f"{err(row[('variance', s)]):.5f}" for s in VARIANCE_SWEEP))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="20 000 triangles and 3 rounds: a check that the tool runs")
    args = ap.parse_args()
    n = 20_000 if args.quick else 1_000_000
    cost(n, 3 if args.quick else 7)
    quality("cornell_textured 256x256", scenes.cornell_textured(256, 256))
    quality(f"C5-style torture {n} triangles 1280x720", scenes.torture(n, 1280, 720))


if __name__ == "__main__":
    main()
