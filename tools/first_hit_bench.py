#!/usr/bin/env python3
"""What seeing through cut-outs costs the first-hit pass, and what it buys the guided denoise, measured on one GPU.

  cost     er_render_features(4) at 1280x720 on the C2-style soup (1 M triangles, seed 12345), which has no cut-out: every ray stops at
           its first hit, so the mode's cost is its own -- one material read and the opacity test per hit.  Mode on against mode off in
           one process, alternated, medians of --rounds (7) device times (HIP events, ErFeatureInfo.ms).  er_render_ids(4) the same way.
  quality  mean absolute error against 1 024 spp of er_denoise_guided at 4 and 16 spp on scenes.cornell_cards(192, 192) -- the textured
           Cornell box with a card of binary opacity in front of its textured back wall -- with the feature planes of the mode on
           against those of the mode off.  Images scaled by (n + 1) / n as tests/test_gpu_features.py does.

    python tools/first_hit_bench.py [--rounds 7] [--part cost|quality|all] [--log profiles/first_hit_cutouts.log]
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elevenrender_amd import render, scenes  # noqa: E402

LOG = None
f32 = np.float32

EXPECTATION = """expectation, written before the first run:
  cost     the mode-off kernels are the kernels of the commit before (same registers, LDS and kernarg in the code object), so mode off is
           what it was.  Mode on adds per hit one 128-byte material read (L2-resident: one material) and a compare, keeps the HitFull of
           the hit across the loop (157 against 141 VGPRs in the feature kernel: still 3 waves per SIMD at 64 lanes) and ends with five
           wave sums and at most five atomics per wave.  A few per cent of a pass that is bound by its four traversals per pixel.
  quality  with the mode off the card's albedo plane is one flat orange and its depth one plane: the guided filter demodulates the wall
           seen through the holes by the wrong albedo and finds no edge between a square and a hole.  Mode on should lower the error at
           4 spp and at 16 spp."""


def say(line=""):
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


def med(xs):
    return statistics.median(xs)


def cost(rounds):
    w, h = 1280, 720
    sc = scenes.soup(1_000_000, w, h, seed=12345)
    say(f"== cost: C2-style soup, {sc.tri_count} triangles, {w}x{h}, 4 rays per pixel, no cut-outs")
    rm = render.RenderingManager(render.RenderParameters(max_bounces=8, device="hip:0"))
    rm.start_rendering(sc)
    for on in (True, False):      # warm: planes, counters
        rm.set_first_hit(on)
        rm.render_features(4)
        rm.render_ids(4)
    ms = {(p, on): [] for p in ("features", "ids") for on in (True, False)}
    for _ in range(rounds):
        for on in (True, False):
            rm.set_first_hit(on)
            rm.render_features(4)
            ms["features", on].append(rm.feature_info()["ms"])
            rm.render_ids(4)
            ms["ids", on].append(rm.id_info()["ms"])
            if on:
                info = rm.first_hit_info()
    for p in ("features", "ids"):
        on, off = ms[p, True], ms[p, False]
        say(f"   {p:8s} mode on {med(on):.3f} ms | mode off {med(off):.3f} ms | on / off {med(on) / med(off):.4f}   (device, medians of {rounds})")
        say(f"            every round: on {' '.join(f'{x:.3f}' for x in on)} | off {' '.join(f'{x:.3f}' for x in off)}")
    say(f"   counters of the last pass with the mode on: {info}")
    rm.close()


def quality():
    w = h = 192
    sc = scenes.cornell_cards(w, h)
    say(f"== quality: cornell_cards {w}x{h}, {sc.tri_count} triangles, er_denoise_guided's defaults, mean |error| against 1024 spp")
    out = {}
    ref = None
    for on in (True, False):
        rm = render.RenderingManager(render.RenderParameters(max_bounces=5, device="hip:0"))
        rm.start_rendering(sc)
        rm.set_first_hit(on)
        rm.render_features()
        done = 0
        for n in (4, 16):
            rm.render(n - done)
            done = n
            rm.denoise_guided()
            out[on, n] = rm.get_pass("denoise")[..., :3] * f32((n + 1) / n)
            out["noisy", n] = rm.get_pass("beauty")[..., :3] * f32((n + 1) / n)
        if ref is None:
            rm.render(1024 - done)
            ref = rm.get_pass("beauty")[..., :3] * f32(1025 / 1024)
        if on:
            say(f"   counters of the feature pass with the mode on: {rm.first_hit_info()}")
        rm.close()
    err = lambda img: float(np.abs(img - ref).mean())
    res = {}
    for n in (4, 16):
        res[n] = (err(out[True, n]), err(out[False, n]))
        say(f"   {n:2d} spp: noisy {err(out['noisy', n]):.5f} | guided, mode off {res[n][1]:.5f} | guided, mode on {res[n][0]:.5f} | on / off {res[n][0] / res[n][1]:.4f}")
    return res


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--part", choices=["cost", "quality", "all"], default="all")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    LOG = args.log
    if LOG:
        open(LOG, "w").close()
    say(EXPECTATION)
    say()
    if args.part in ("cost", "all"):
        cost(max(3, args.rounds))
    if args.part in ("quality", "all"):
        quality()


if __name__ == "__main__":
    main()
