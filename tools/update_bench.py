#!/usr/bin/env python3
"""What er_render_update saves and what a refitted tree costs, measured on one GPU (DESIGN.md "Editing a begun scene").

For the scenes of BASELINE configs C2 (1 M-triangle soup, 1920x1080) and C4 (10 M triangles of blobs, 3840x2160):
  camera    wall time of a camera-only er_render_update against er_render_begin on the same begun scene, alternated;
  T, M, J   refit_ms / update_ms of an update that moves triangles -- T: every vertex (and the camera) + (40, -3, 7); M: an object
            moved (C4: one blob instance onto another; C2: the first 1 % of the triangles by (0.9, 0.3, 0.5)); J: every vertex
            jittered by N(0, 0.3 triangle sizes) -- against build_ms and the wall time of a fresh er_scene_create + er_render_begin of
            the edited scene;
  rate      Msamples/s (counted bounce samples / device time) of --steps samples on the refitted tree (A) against the fresh build of
            the same edited scene (B), same process, alternated A B A B ..., --rounds times each.

    python tools/update_bench.py [--configs C2,C4] [--steps 20] [--rounds 3] [--log FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elevenrender_amd import abi, render, scenes  # noqa: E402

OUT = []


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


def copy_scene(sc, vertices=None, camera=None):
    import copy
    out = copy.copy(sc)
    out._desc = None
    if vertices is not None:
        out.vertices = np.ascontiguousarray(vertices, np.float32).reshape(sc.vertices.shape)
    if camera is not None:
        out.camera = camera
    return out


def shifted_camera(cam, d):
    c = abi.ErCamera.from_buffer_copy(cam)
    c.position = abi.ErVec3(cam.position.x + d[0], cam.position.y + d[1], cam.position.z + d[2])
    return c


def manager(sc, max_bounces):
    rm = render.RenderingManager(render.RenderParameters(max_bounces=max_bounces, device="hip:0"))
    t0 = time.perf_counter()
    rm.start_rendering(sc)
    return rm, (time.perf_counter() - t0) * 1e3


def rate(rm, steps):
    """Msamples/s of `steps` more samples: counted bounce-loop iterations over the device time of the call"""
    c0 = rm.counters()["bounce_samples"]
    rm.render(steps, blocking=False)
    ms = rm.wait()
    return (rm.counters()["bounce_samples"] - c0) / ms / 1e3


def begin_again(rm, max_bounces):
    p = abi.ErRenderParams(rm.pars.sampleTarget, rm.pars.block_size, max_bounces, 0, 0, 1, 0)
    t0 = time.perf_counter()
    abi.check(rm.lib.er_render_begin(rm.handle, C.byref(p)))
    return (time.perf_counter() - t0) * 1e3


def bench(name, sc, max_bounces, steps, rounds, instances):
    v = sc.vertices.reshape(-1, 3, 3)
    n = len(v)
    say(f"== {name}: {n} triangles, {sc.x_res}x{sc.y_res}, max_bounces {max_bounces}")
    rm, first_ms = manager(sc, max_bounces)
    info = rm.accel_info()
    say(f"   er_scene_create + er_render_begin {first_ms:.1f} ms (builder {info['builder']}, build_ms {info['build_ms']:.1f}, upload_ms {info['upload_ms']:.1f})")
    rate(rm, 2)      # (warm: the streaming schedule's first call decides its deal)
    cam2 = shifted_camera(sc.camera, (0.05, 0.02, -0.1))
    for k in range(3):      # alternated: begin, update, begin, update, ...
        b = begin_again(rm, max_bounces)
        rm.render(1)
        t0 = time.perf_counter()
        rm.update(camera=cam2 if k % 2 == 0 else sc.camera)
        u = (time.perf_counter() - t0) * 1e3
        rm.render(1)
        say(f"   camera  round {k}: er_render_begin {b:8.2f} ms wall   er_render_update(camera) {u:7.3f} ms wall (update_ms {rm.update_info()['update_ms']:.3f})")
    rm.close()

    e = 2.0 / np.cbrt(n)
    rng = np.random.default_rng(7)
    shift = np.array([40.0, -3.0, 7.0], np.float32)
    vm = v.copy()
    if instances:
        per = n // instances
        vm[:per] += (v[(instances - 1) * per:].reshape(-1, 3).mean(0) - v[:per].reshape(-1, 3).mean(0)).astype(np.float32)
    else:
        vm[:n // 100] += np.array([0.9, 0.3, 0.5], np.float32)
    edits = (("T", (v + shift).astype(np.float32), shifted_camera(sc.camera, shift)),
             ("M", vm, None),
             ("J", (v + rng.normal(0.0, 0.3 * e, size=v.shape)).astype(np.float32), None))
    for tag, vnew, cam in edits:
        a, _ = manager(sc, max_bounces)
        rate(a, 2)
        kw = dict(vertices=vnew)
        if cam is not None:
            kw["camera"] = cam
        t0 = time.perf_counter()
        a.update(**kw)
        wall = (time.perf_counter() - t0) * 1e3
        ui = a.update_info()
        sc_new = copy_scene(sc, vnew, cam)
        b, fresh_ms = manager(sc_new, max_bounces)
        bi = b.accel_info()
        say(f"   {tag}: update {wall:.2f} ms wall (update_ms {ui['update_ms']:.2f}, refit_ms {ui['refit_ms']:.2f}; the first refit of a topology also derives its levels)"
            f"   fresh create + begin {fresh_ms:.1f} ms wall (build_ms {bi['build_ms']:.1f})")
        t0 = time.perf_counter()
        a.update(**kw)      # the same arrays again: the levels are there
        say(f"   {tag}: second update {(time.perf_counter() - t0) * 1e3:.2f} ms wall (refit_ms {a.update_info()['refit_ms']:.2f})")
        rate(a, 2)
        rate(b, 2)
        ra, rb = [], []
        for _ in range(rounds):
            ra.append(rate(a, steps))
            rb.append(rate(b, steps))
        say(f"   {tag}: Msamples/s of {steps} steps, A = refitted {' '.join(f'{x:7.1f}' for x in ra)}   B = fresh build {' '.join(f'{x:7.1f}' for x in rb)}"
            f"   median A/B {np.median(ra) / np.median(rb):.4f}")
        a.close()
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log")
    args = ap.parse_args()
    for cfg in args.configs.split(","):
        if cfg == "C2":
            bench("C2", scenes.soup(1_000_000, 1920, 1080, seed=12345), 8, args.steps, args.rounds, 0)
        elif cfg == "C4":
            bench("C4", scenes.blob_instances(x_res=3840, y_res=2160), 8, args.steps, args.rounds, 10000)
        else:
            raise SystemExit(f"unknown config {cfg}")
        if args.log:
            with open(args.log, "w") as f:
                f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
