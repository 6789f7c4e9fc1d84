#!/usr/bin/env python3
"""What the temporal reprojection costs and what it buys (er_history_capture / er_history_resolve).

Cost: the 1 M-triangle soup with 64 objects at 1280x720 and 1920x1080, alternated, medians of 7 rounds: capture_ms and resolve_ms
(device time, ErHistoryInfo) beside er_render_ids(4) (ErIdInfo.ms), a camera-only er_render_update (wall) and one er_render_samples(1)
(wall).

Quality: cornell_textured 256x256 and the C5-style frame (torture, 1 M triangles, 1280x720): 64 spp, a small camera move, 4 spp; the mean
absolute error of get_blended() and of plain BEAUTY scaled by samples / n, against 1 024 spp of the new frame.

EXPECTATION, written before the first run: a resolve traces one pinhole ray per pixel where the id pass traces four jittered ones, so
about a quarter of er_render_ids(4) plus the per-pixel kernel (80 bytes per pixel of traffic: tens of microseconds at 1080p); a capture
whose key plane is still current is the per-pixel kernel alone.  Both should be well below a camera-only update plus its first sample.
For quality the blend carries up to 32 samples' weight against 4: where the history is valid the error should fall towards that of
~36 spp, so a ratio well below 1 on the Cornell box (diffuse, little parallax) and nearer 1 on the soup (thin triangles: many
partial and rejected pixels).

    python tools/history_bench.py [--quick] > profiles/history_bench.log
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from elevenrender_amd import abi, history, render, scenes  # noqa: E402


def moved(sc, dpos, rot):
    cam = abi.ErCamera.from_buffer_copy(sc.camera)
    cam.position = abi.ErVec3(sc.camera.position.x + dpos[0], sc.camera.position.y + dpos[1], sc.camera.position.z + dpos[2])
    cam.rotation = abi.ErVec3(sc.camera.rotation.x + rot[0], sc.camera.rotation.y + rot[1], sc.camera.rotation.z + rot[2])
    return cam


def cost(n_tris, rounds):
    frames = {"720p": (1280, 720), "1080p": (1920, 1080)}
    last = {}
    rms, rows = {}, {k: {m: [] for m in ("capture_ms", "capture_current_ms", "resolve_ms", "ids4_ms", "update_ms", "sample1_ms")} for k in frames}
    for name, (w, h) in frames.items():
        sc = scenes.soup(n_tris, w, h)
        rm = render.RenderingManager(render.RenderParameters())
        rm.start_rendering(sc)
        t = np.arange(sc.tri_count, dtype=np.uint32)
        rm.set_objects([t[t % 64 == o] for o in range(64)])
        rm.render(2)
        rms[name] = (rm, sc)
    for r in range(rounds + 1):      # (round 0 warms up and allocates)
        for name, (rm, sc) in rms.items():
            cam = moved(sc, (0.002 * (r + 1), 0.001, 0.0), (0.0, 0.1 * (r + 1), 0.0))
            rm.history_capture()
            c0 = rm.history_info()["capture_ms"]
            t0 = time.perf_counter()
            rm.update(camera=cam)
            t1 = time.perf_counter()
            rm.history_resolve()
            last[name] = rm.history_info()
            res = last[name]["resolve_ms"]
            rm.history_capture()      # the resolve's key plane is current: the per-pixel kernel alone
            c1 = rm.history_info()["capture_ms"]
            t2 = time.perf_counter()
            rm.render(1)
            t3 = time.perf_counter()
            rm.render_ids(4)
            ids = rm.id_info()["ms"]
            if r:
                for k, v in zip(("capture_ms", "capture_current_ms", "resolve_ms", "ids4_ms", "update_ms", "sample1_ms"), (c0, c1, res, ids, (t1 - t0) * 1e3, (t3 - t2) * 1e3)):
                    rows[name][k].append(v)
    for name, (rm, _) in rms.items():
        info = last[name]
        rm.close()
        print(f"cost {name} soup {n_tris} triangles, 64 objects, medians of {rounds}: " + ", ".join(f"{k} {statistics.median(v):.3f}" for k, v in rows[name].items()))
        print(f"     last resolve: {info}")


def quality(label, sc, dpos, rot):
    npx = sc.x_res * sc.y_res
    none = np.zeros((npx, 4), np.float32)
    plain_of = lambda rm: history.blend(rm.get_pass("beauty"), rm.read_samples(), none).reshape(sc.y_res, sc.x_res, 4)[..., :3].astype(np.float64)
    cam = moved(sc, dpos, rot)
    rm = render.RenderingManager(render.RenderParameters())
    rm.start_rendering(sc)
    rm.render(64)
    rm.update(camera=cam, keep_history=True)
    rm.render(4)
    blended, plain, info = rm.get_blended()[..., :3].astype(np.float64), plain_of(rm), rm.history_info()
    rm.update(camera=cam)
    rm.render(1024)
    truth = plain_of(rm)
    rm.close()
    eb, ep = np.abs(blended - truth).mean(), np.abs(plain - truth).mean()
    print(f"quality {label}: mean absolute error against 1024 spp: blend {eb:.5f}, plain 4 spp {ep:.5f}, ratio {eb / ep:.3f}")
    print(f"     classes: valid {info['pixels_valid']} partial {info['pixels_partial']} offscreen {info['pixels_offscreen']} rejected {info['pixels_rejected']} sky {info['pixels_sky']} of {npx}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="20 000 triangles and 3 rounds: a check that the tool runs")
    args = ap.parse_args()
    n = 20_000 if args.quick else 1_000_000
    cost(n, 3 if args.quick else 7)
    quality("cornell_textured 256x256", scenes.cornell_textured(256, 256), (0.02, 0.01, 0.0), (0.0, 1.0, 0.0))
    quality(f"C5-style torture {n} triangles 1280x720", scenes.torture(n, 1280, 720), (0.01, 0.005, 0.0), (0.0, 0.5, 0.0))


if __name__ == "__main__":
    main()
