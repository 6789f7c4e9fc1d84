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

--rebuild (C5 = C2's geometry with 64 textured materials is a config here too): for the edits T, M, J and S1 / S5 -- the
first 1 % / 5 % of the triangles moved, each as a whole, by U(-1/2, 1/2) x the scene's extent -- the measured cost ratio Q =
er_accel_cost(refitted) / er_accel_cost(built) and cost_ms, update_ms of the same update under ER_REBUILD_NEVER, ALWAYS and AUTO
(--ratio, default 2) with the structure stage's rebuild_ms, the rate on the refitted tree (A) against the tree rebuilt in place (B),
alternated as above, and er_render_begin again on the begun scene for comparison.

    python tools/update_bench.py --rebuild [--configs C2,C4,C5] [--ratio 2] [--log FILE]
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
LOG = None      # --log: every line is appended as it is said, so that a run that is cut short leaves what it measured


def say(line=""):
    print(line, flush=True)
    OUT.append(line)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


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


def scattered(v, share, seed=11):
    out = v.copy()
    m = max(1, int(round(share * len(v))))
    extent = v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0)
    out[:m] += (np.random.default_rng(seed).uniform(-0.5, 0.5, size=(m, 1, 3)) * extent).astype(np.float32)
    return out


def rebuild_bench(name, sc, max_bounces, steps, rounds, instances, ratio):
    v = sc.vertices.reshape(-1, 3, 3)
    n = len(v)
    say(f"== {name} (rebuild policies): {n} triangles, {sc.x_res}x{sc.y_res}, max_bounces {max_bounces}, AUTO ratio {ratio}")
    e = 2.0 / np.cbrt(n)
    shift = np.array([40.0, -3.0, 7.0], np.float32)
    vm = v.copy()
    if instances:
        per = n // instances
        vm[:per] += (v[(instances - 1) * per:].reshape(-1, 3).mean(0) - v[:per].reshape(-1, 3).mean(0)).astype(np.float32)
    else:
        vm[:n // 100] += np.array([0.9, 0.3, 0.5], np.float32)
    edits = (("T", (v + shift).astype(np.float32), shifted_camera(sc.camera, shift)),
             ("M", vm, None),
             ("J", (v + np.random.default_rng(7).normal(0.0, 0.3 * e, size=v.shape)).astype(np.float32), None),
             ("S1", scattered(v, 0.01), None),
             ("S5", scattered(v, 0.05), None))
    for tag, vnew, cam in edits:
        kw = dict(vertices=vnew)
        if cam is not None:
            kw["camera"] = cam
        walls, mgr = {}, {}
        for mode, label in ((abi.REBUILD_NEVER, "NEVER"), (abi.REBUILD_ALWAYS, "ALWAYS"), (abi.REBUILD_AUTO, "AUTO")):
            rm, _ = manager(sc, max_bounces)
            rate(rm, 2)
            rm.set_update_policy(mode, ratio if mode == abi.REBUILD_AUTO else 0.0)
            built = rm.accel_cost() if mode == abi.REBUILD_NEVER else None      # (AUTO measures its own baseline inside the update)
            t0 = time.perf_counter()
            rm.update(**kw)
            walls[label] = ((time.perf_counter() - t0) * 1e3, rm.update_info()["update_ms"], rm.rebuild_info())
            if mode == abi.REBUILD_NEVER:
                refit = rm.accel_cost()
                say(f"   {tag}: Q = cost refitted / built = {refit['cost']:.4f} / {built['cost']:.4f} = {refit['cost'] / built['cost']:.3f}   cost_ms {built['ms']:.3f} (built) {refit['ms']:.3f} (refitted)"
                    f"   refit_ms {rm.update_info()['refit_ms']:.2f}")
            if mode == abi.REBUILD_AUTO:
                begin_ms = begin_again(rm, max_bounces)
                rm.close()
            else:
                mgr[label] = rm
        r = walls["AUTO"][2]
        say(f"   {tag}: update_ms NEVER {walls['NEVER'][1]:.2f}   ALWAYS {walls['ALWAYS'][1]:.2f} (structure stage {walls['ALWAYS'][2]['rebuild_ms']:.2f}, builder {mgr['ALWAYS'].accel_info()['builder']})"
            f"   AUTO {walls['AUTO'][1]:.2f} (decision {r['last_decision']}, cost built {r['cost_built']:.4f} refit {r['cost_refit']:.4f} after {r['cost_after']:.4f}, cost_ms {r['cost_ms']:.3f})"
            f"   er_render_begin again on that scene, this build, {begin_ms:.1f} ms wall")
        a, b = mgr["NEVER"], mgr["ALWAYS"]
        rate(a, 2)
        rate(b, 2)
        ra, rb = [], []
        for _ in range(rounds):
            ra.append(rate(a, steps))
            rb.append(rate(b, steps))
        ma, mb = float(np.median(ra)), float(np.median(rb))
        # samples of this frame after which the rebuilt tree has repaid what its update cost more than the refit's
        extra_ms = walls["ALWAYS"][1] - walls["NEVER"][1]
        per_a, per_b = a.counters()["bounce_samples"], b.counters()["bounce_samples"]      # (equal: the images do not depend on the tree)
        spp = a.get_render_info().samples - 1
        ms_a, ms_b = per_a / spp / ma / 1e3, per_b / spp / mb / 1e3                          # device ms per sample of the frame
        repaid = extra_ms / (ms_a - ms_b) if ms_a > ms_b else float("inf")
        say(f"   {tag}: Msamples/s of {steps} steps, A = refitted {' '.join(f'{x:7.1f}' for x in ra)}   B = rebuilt {' '.join(f'{x:7.1f}' for x in rb)}"
            f"   median A/B {ma / mb:.4f}   ms per sample A {ms_a:.2f} B {ms_b:.2f}: the rebuild's extra {extra_ms:.1f} ms is repaid after {repaid:.1f} samples")
        a.close()
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log")
    ap.add_argument("--rebuild", action="store_true", help="the rebuild policies of er_update_policy_set instead of the update / refit figures")
    ap.add_argument("--ratio", type=float, default=2.0, help="--rebuild: max_cost_ratio of the ER_REBUILD_AUTO runs")
    args = ap.parse_args()
    if args.log:
        global LOG
        LOG = args.log
        open(LOG, "w").close()
    for cfg in args.configs.split(","):
        if args.rebuild:
            if cfg == "C2":
                rebuild_bench("C2", scenes.soup(1_000_000, 1920, 1080, seed=12345), 8, args.steps, args.rounds, 0, args.ratio)
            elif cfg == "C4":
                rebuild_bench("C4", scenes.blob_instances(x_res=3840, y_res=2160), 8, args.steps, args.rounds, 10000, args.ratio)
            elif cfg == "C5":      # (reference behaviour: its point lights and MIS are flags of the render, not of the structure)
                rebuild_bench("C5", scenes.torture(1_000_000, 1920, 1080, seed=12345), 16, args.steps, args.rounds, 0, args.ratio)
            else:
                raise SystemExit(f"unknown config {cfg}")
        elif cfg == "C2":
            bench("C2", scenes.soup(1_000_000, 1920, 1080, seed=12345), 8, args.steps, args.rounds, 0)
        elif cfg == "C4":
            bench("C4", scenes.blob_instances(x_res=3840, y_res=2160), 8, args.steps, args.rounds, 10000)
        else:
            raise SystemExit(f"unknown config {cfg}")


if __name__ == "__main__":
    main()
