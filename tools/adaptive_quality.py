"""Adaptive sampling (er_adaptive_set): what it saves and what it costs, on C2 and C5 at 1080p (GPU).

For each scene: a uniform 1 024-spp reference; uniform 16 / 32 / 64 spp; adaptive runs at three thresholds capped at 64 samples
(min_samples 16, interval 8, the defaults); and threshold 0 against plain 64 spp -- the same image, so the difference is the pure
overhead of the snapshots, tests and re-deals.  Per run: device time (median of --repeats, er_wait's elapsed time of one
er_render_samples_async call from a fresh er_render_begin), pixel samples spent, RMSE of BEAUTY rgb against the reference.

    python tools/adaptive_quality.py [--configs C2 C5] [--repeats 5] [--out profiles/adaptive_quality.log]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from elevenrender_amd import abi, render, scenes  # noqa: E402

CONFIGS = {   # bench.py's scenes: (make, max_bounces, extension flags)
    "C2": (lambda: scenes.soup(1_000_000, 1920, 1080, seed=12345), 8, 0),
    "C5": (lambda: scenes.torture(1_000_000, 1920, 1080, seed=12345), 16, abi.FLAG_POINT_LIGHTS | abi.FLAG_MIS),
}


def run(sc, max_bounces, flags, spp, adaptive=None):
    rm = render.RenderingManager(render.RenderParameters(max_bounces=max_bounces, flags=flags))
    rm.start_rendering(sc)
    if adaptive is not None:
        rm.set_adaptive(adaptive, 16, 8)
    rm.render(spp, blocking=False)
    ms = rm.wait()
    img = rm.get_pass("beauty")[..., :3].copy()
    info = rm.adaptive_info()
    rm.close()
    return ms, img, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["C2", "C5"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.01, 0.03, 0.1])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_quality.log"))
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# tools/adaptive_quality.py {time.strftime('%Y-%m-%d %H:%M:%S')}: median of {args.repeats} runs, device time of one call "
        f"(er_wait elapsed) from a fresh er_render_begin; adaptive: min_samples 16, interval 8, capped at 64 samples")
    for cfg in args.configs:
        make, mb, flags = CONFIGS[cfg]
        sc = make()
        px = sc.x_res * sc.y_res
        _, ref, _ = run(sc, mb, flags, args.reference_spp)
        log(f"\n## {cfg} {sc.x_res}x{sc.y_res}, max_bounces {mb}, reference {args.reference_spp} spp")
        log(f"{'run':<22}{'ms (median)':>12}{'ms min..max':>18}{'pixel samples':>16}{'spp equiv':>11}{'RMSE':>12}{'active tiles':>14}")
        rows = [(f"uniform {n}", n, None) for n in (16, 32, 64)] + [(f"adaptive {t:g}", 64, t) for t in args.thresholds] + [("adaptive 0", 64, 0.0)]
        times = {}
        for name, spp, thr in rows:
            ms = []
            for _ in range(args.repeats):
                t, img, info = run(sc, mb, flags, spp, thr)
                ms.append(t)
            rmse = float(np.sqrt(np.mean((img.astype(np.float64) - ref) ** 2)))
            times[name] = statistics.median(ms)
            ps = int(info["pixel_samples"])
            active = f"{info['active_tiles']}/{info['owned_tiles']}" if info["enabled"] else "-"
            log(f"{name:<22}{times[name]:>12.2f}{f'{min(ms):.2f}..{max(ms):.2f}':>18}{ps:>16}{ps / px:>11.2f}{rmse:>12.6f}{active:>14}")
        log(f"threshold-0 overhead against plain 64 spp (same image): {100.0 * (times['adaptive 0'] / times['uniform 64'] - 1.0):+.2f} %")
        for t in args.thresholds:
            name = f"adaptive {t:g}"
            log(f"{name}: time {100.0 * times[name] / times['uniform 64']:.1f} % of uniform 64")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
