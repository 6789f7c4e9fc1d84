"""Next-event estimation of emissive triangles (ER_FLAG_MESH_LIGHTS): what it costs and what it buys, on C1 and on C1 lit by its
emitter (scenes.cornell_dim) at 256 x 256 (GPU).

For each scene and each setting (without / with the flag): device time per sample (median of --repeats, er_wait's elapsed time of
one er_render_samples_async call of --spp samples from a fresh er_render_begin, divided by --spp); RMSE of BEAUTY rgb at --spp
against a --reference-spp render with the flag; and RMSE at equal device time: the render without the flag given as many samples as
fit in the time of the --spp-sample render with it.

    python tools/mesh_light_quality.py [--repeats 5] [--spp 16] [--out profiles/mesh_light_quality.log]
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

CONFIGS = {"C1": scenes.cornell, "C1 dim": scenes.cornell_dim}


def run(sc, flags, spp):
    rm = render.RenderingManager(render.RenderParameters(flags=flags))
    rm.start_rendering(sc)
    rm.render(spp, blocking=False)
    ms = rm.wait()
    img = rm.get_pass("beauty")[..., :3].astype(np.float64)
    rm.close()
    return ms, img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reference-spp", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_light_quality.log"))
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# tools/mesh_light_quality.py {time.strftime('%Y-%m-%d %H:%M:%S')}: median of {args.repeats} runs, device time of one call "
        f"(er_wait elapsed) from a fresh er_render_begin; reference {args.reference_spp} spp with the flag")
    for cfg in args.configs:
        sc = CONFIGS[cfg](256, 256)
        _, ref = run(sc, abi.FLAG_MESH_LIGHTS, args.reference_spp)
        log(f"\n## {cfg} {sc.x_res}x{sc.y_res}")
        log(f"{'setting':<12}{'ms/sample':>12}{'ms min..max':>18}{f'RMSE @{args.spp} spp':>16}")
        per = {}
        for name, flags in (("plain", 0), ("mesh", abi.FLAG_MESH_LIGHTS)):
            ms, img = [], None
            for _ in range(args.repeats):
                t, img = run(sc, flags, args.spp)
                ms.append(t / args.spp)
            rmse = float(np.sqrt(np.mean((img - ref) ** 2)))
            per[name] = (statistics.median(ms), rmse)
            log(f"{name:<12}{per[name][0]:>12.4f}{f'{min(ms):.4f}..{max(ms):.4f}':>18}{rmse:>16.6f}")
        n_eq = max(1, int(round(args.spp * per["mesh"][0] / per["plain"][0])))
        _, img = run(sc, 0, n_eq)
        rmse_eq = float(np.sqrt(np.mean((img - ref) ** 2)))
        log(f"time per sample with / without: {per['mesh'][0] / per['plain'][0]:.3f}")
        log(f"RMSE at equal spp, with / without: {per['mesh'][1] / per['plain'][1]:.3f}")
        log(f"equal device time: plain at {n_eq} spp RMSE {rmse_eq:.6f}; with / without: {per['mesh'][1] / rmse_eq:.3f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
