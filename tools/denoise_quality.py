"""The denoise guided by first-hit albedo and depth (er_render_features + er_denoise_guided) against the plain one (er_denoise): what
it buys at 4 spp on textured content and what it costs (GPU).

Scenes: scenes.cornell_textured at 256 x 256 and a C5-style scenes.torture frame at 1280 x 720.  For each: mean absolute error of
BEAUTY rgb against a --reference-spp render of the same pixels (both scaled by (n + 1) / n, as tests/test_gpu_denoise.py does) of
the noisy --spp frame, of er_denoise at colour sigma 0.5 / 1 / 2 and of er_denoise_guided with its defaults; and medians of
--repeats times, taken alternating, of er_render_features(4) (ErFeatureInfo.ms: HIP events), of one er_render_samples(1) (er_wait's
elapsed device time), and of er_denoise and er_denoise_guided (host wall time of the blocking call: the library reports no device time
for them; it includes the allocation of their scratch planes and the launches).

    python tools/denoise_quality.py [--repeats 5] [--spp 4] [--out profiles/guided_denoise.log]
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

CONFIGS = {
    "cornell_textured 256x256": lambda a: (scenes.cornell_textured(256, 256), 5),
    "torture 1280x720": lambda a: (scenes.torture(a.torture_tris, 1280, 720), 8),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--torture-tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_denoise.log"))
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# tools/denoise_quality.py {time.strftime('%Y-%m-%d %H:%M:%S')}: {args.spp} spp against {args.reference_spp} spp; medians of {args.repeats}, alternating")
    for cfg in args.configs:
        sc, bounces = CONFIGS[cfg](args)
        rm = render.RenderingManager(render.RenderParameters(max_bounces=bounces))
        rm.start_rendering(sc)
        rm.render(args.spp)
        rm.render_features(4)
        n = args.spp
        images = {"noisy": rm.get_pass("beauty")}
        for sigma in (0.5, 1.0, 2.0):
            rm.denoise(5, sigma)
            images[f"er_denoise sigma {sigma}"] = rm.get_pass("denoise")
        rm.denoise_guided()
        images["er_denoise_guided"] = rm.get_pass("denoise")
        t = {"er_render_features(4)": [], "er_render_samples(1)": [], "er_denoise": [], "er_denoise_guided": []}
        for _ in range(args.repeats):
            rm.render_features(4)
            t["er_render_features(4)"].append(rm.feature_info()["ms"])
            rm.render(1, blocking=False)
            t["er_render_samples(1)"].append(rm.wait())
            t0 = time.perf_counter()
            rm.denoise()
            t["er_denoise"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            rm.denoise_guided()
            t["er_denoise_guided"].append((time.perf_counter() - t0) * 1e3)
        done = n + args.repeats
        rm.render(args.reference_spp - done)
        ref = rm.get_pass("beauty")[..., :3].astype(np.float64) * (args.reference_spp + 1) / args.reference_spp
        rays = rm.feature_info()["rays"]
        rm.close()
        log(f"\n## {cfg}, {sc.tri_count} triangles, {len(sc.materials)} materials, max_bounces {bounces}")
        log(f"{'image':<28}{'mean abs error':>16}")
        err = {k: float(np.abs(v[..., :3].astype(np.float64) * (n + 1) / n - ref).mean()) for k, v in images.items()}
        for k, e in err.items():
            log(f"{k:<28}{e:>16.5f}")
        best = min(e for k, e in err.items() if k.startswith("er_denoise sigma"))
        log(f"guided / best plain: {err['er_denoise_guided'] / best:.3f}")
        log(f"{'step':<28}{'median ms':>12}{'min..max':>22}")
        for k, v in t.items():
            log(f"{k:<28}{statistics.median(v):>12.4f}{f'{min(v):.4f}..{max(v):.4f}':>22}")
        log(f"feature rays per pass: {rays}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
