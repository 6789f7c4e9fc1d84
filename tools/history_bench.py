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

--variance: what carrying the variance through the history costs and what er_denoise_blended buys.  The same soup and
frames, two handles per frame -- one that folds, so that its captures carry the variance plane, and one that never does --, frames and
handles alternated in one session, medians of 7: resolve_ms and capture_ms with and without the carried plane, and the device time of
er_denoise_blended beside er_denoise_variance on the handle that folds.  Quality: the same two frames and moves as above with 64 spp in
folds of 2; blend, denoised blend, and the plain 4 spp through er_denoise_guided, each against 1 024 spp.

EXPECTATION, written before the first run: the per-pixel part of the combined resolve moves about 1.5 x the bytes of the plain one --
four more 16-byte tap reads and one more 16-byte store (80 B) against 24 B of key, 4 x 32 B of taps and 16 B out (168 B) -- so at 1080p
166 MB more, some 0.04 - 0.08 ms at the bandwidth such kernels reach here; resolve_ms also holds the key pass (one traced ray per
pixel), which does not change, so the ratio of the two resolve_ms should be well below 1.5 and their DIFFERENCE is what to compare with
the per-pixel kernel (capture_current_ms is such a kernel alone).  The combined kernel counts in registers with a bounded grid where the
plain one adds once per wave and class, so it may even gain there.  A capture that carries adds one kernel of 16 B in, up to 48 B more in
and 16 B out per pixel: about the plain capture kernel again.  er_denoise_blended runs er_denoise_variance's levels on planes of the
same size; its split reads three more planes and writes one more: a few per cent above er_denoise_variance.  Quality: the blend's
variance is small where the history is valid, so the colour stop is tight there and the filter mostly removes the noise of the
disoccluded and rejected pixels, which carry only 4 spp: the denoised blend should beat the blend clearly, and beat the guided filter of
the plain 4 spp where most pixels have a history.

    python tools/history_bench.py --variance [--quick] > profiles/history_variance_bench.log
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


def cost_variance(n_tris, rounds):
    frames = {"720p": (1280, 720), "1080p": (1920, 1080)}
    keys = ("capture_ms", "capture_current_ms", "resolve_ms", "denoise_blended_ms", "denoise_variance_ms")
    rms, rows, last = {}, {}, {}
    for name, (w, h) in frames.items():
        sc = scenes.soup(n_tris, w, h)
        for mode in ("carried", "plain"):
            rm = render.RenderingManager(render.RenderParameters())
            rm.start_rendering(sc)
            t = np.arange(sc.tri_count, dtype=np.uint32)
            rm.set_objects([t[t % 64 == o] for o in range(64)])
            rm.render(2)
            if mode == "carried":
                rm.variance_fold()
            rms[name, mode], rows[name, mode] = (rm, sc), {k: [] for k in keys}
    for r in range(rounds + 1):      # (round 0 warms up and allocates)
        for (name, mode), (rm, sc) in rms.items():
            cam = moved(sc, (0.002 * (r + 1), 0.001, 0.0), (0.0, 0.1 * (r + 1), 0.0))
            rm.history_capture()
            c0 = rm.history_info()["capture_ms"]
            rm.update(camera=cam)
            rm.history_resolve()
            res = rm.history_info()["resolve_ms"]
            for _ in range(2):
                rm.render(1)
                if mode == "carried":
                    rm.variance_fold()
            rm.render_features()
            rm.denoise_blended()
            last[name, mode] = rm.history_variance_info()
            fb = last[name, mode]["filter_ms"]
            fv = float("nan")
            if mode == "carried":
                rm.denoise_variance()
                fv = rm.variance_info()["filter_ms"]
            rm.history_capture()      # the resolve's key plane is current: the per-pixel kernels alone
            c1 = rm.history_info()["capture_ms"]
            if r:
                for k, v in zip(keys, (c0, c1, res, fb, fv)):
                    rows[name, mode][k].append(v)
    for (name, mode), (rm, _) in rms.items():
        rm.close()
        print(f"cost {name} {mode} soup {n_tris} triangles, 64 objects, medians of {rounds}: " + ", ".join(f"{k} {statistics.median(v):.3f}" for k, v in rows[name, mode].items()))
        print(f"     last: {last[name, mode]}")
    for name in frames:
        a, b = rows[name, "carried"], rows[name, "plain"]
        med = lambda v: statistics.median(v)
        print(f"cost {name}: resolve carried / plain {med(a['resolve_ms']) / med(b['resolve_ms']):.3f} (difference {med(a['resolve_ms']) - med(b['resolve_ms']):+.3f} ms), "
              f"capture with a current key carried / plain {med(a['capture_current_ms']) / med(b['capture_current_ms']):.3f} "
              f"(difference {med(a['capture_current_ms']) - med(b['capture_current_ms']):+.3f} ms), "
              f"er_denoise_blended / er_denoise_variance {med(a['denoise_blended_ms']) / med(a['denoise_variance_ms']):.3f}")


def quality_variance(label, sc, dpos, rot):
    npx = sc.x_res * sc.y_res
    none = np.zeros((npx, 4), np.float32)
    mean_of = lambda rm, plane: history.blend(plane, rm.read_samples(), none).reshape(sc.y_res, sc.x_res, 4)[..., :3].astype(np.float64)      # (without the setup sample)
    cam = moved(sc, dpos, rot)
    rm = render.RenderingManager(render.RenderParameters())
    rm.start_rendering(sc)
    rm.render(64, fold_every=2)
    rm.update(camera=cam, keep_history=True)
    rm.render(4)
    rm.render_features()
    rm.denoise_blended()
    denoised, info = rm.get_pass("denoise")[..., :3].astype(np.float64), rm.history_variance_info()
    blended, plain = rm.get_blended()[..., :3].astype(np.float64), mean_of(rm, rm.get_pass("beauty"))
    rm.denoise_guided()
    guided = mean_of(rm, rm.get_pass("denoise"))
    rm.update(camera=cam)
    rm.render(1024)
    truth = mean_of(rm, rm.get_pass("beauty"))
    rm.close()
    err = lambda a: float(np.abs(a - truth).mean())
    eb, ed, ep, eg = err(blended), err(denoised), err(plain), err(guided)
    print(f"quality {label}: mean absolute error against 1024 spp: blend {eb:.5f}, er_denoise_blended {ed:.5f} (x{ed / eb:.3f} of the blend), plain 4 spp {ep:.5f}, "
          f"er_denoise_guided of it {eg:.5f} (x{eg / ep:.3f} of the plain); denoised blend / guided {ed / eg:.3f}")
    print(f"     known pixels: history {info['pixels_known_history']} blended {info['pixels_known_blended']} of {npx}; filter {info['filter_ms']:.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="20 000 triangles and 3 rounds: a check that the tool runs")
    ap.add_argument("--variance", action="store_true", help="the carried variance and er_denoise_blended (DESIGN.md 3n) instead of the history alone")
    args = ap.parse_args()
    n = 20_000 if args.quick else 1_000_000
    if args.variance:
        cost_variance(n, 3 if args.quick else 7)
        quality_variance("cornell_textured 256x256", scenes.cornell_textured(256, 256), (0.02, 0.01, 0.0), (0.0, 1.0, 0.0))
        quality_variance(f"C5-style torture {n} triangles 1280x720", scenes.torture(n, 1280, 720), (0.01, 0.005, 0.0), (0.0, 0.5, 0.0))
        return
    cost(n, 3 if args.quick else 7)
    quality("cornell_textured 256x256", scenes.cornell_textured(256, 256), (0.02, 0.01, 0.0), (0.0, 1.0, 0.0))
    quality(f"C5-style torture {n} triangles 1280x720", scenes.torture(n, 1280, 720), (0.01, 0.005, 0.0), (0.0, 0.5, 0.0))


if __name__ == "__main__":
    main()
