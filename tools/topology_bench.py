#!/usr/bin/env python3
"""What er_render_topology costs beside what a caller had to do before it, measured on one GPU.

On the scenes of BASELINE configs C5 (scenes.torture(): 1 M triangles, 64 materials of three 256 x 256 textures = a 193 MB pool, a
2048 x 1024 HDRI, 1920x1080) and C4 (scenes.blob_instances(): 10 M triangles in blobs of 1 000, 3840x2160), per round and alternated
on one box:
  path 2   the store released by another edit (new material ids, not timed), then a topology edit that removes 1 000 consecutive
           triangles (on C4 one blob) and appends the same number (the removed ones, moved): the store is filled from the host copy
  path 1   the same kind of edit right after it: the store is resident and compacted on the device
  fresh    er_scene_destroy + er_scene_create + er_render_begin of the same edited description: what the parent commit offers
Wall times of the calls, and ErTopologyInfo's own figures: edit_ms, build_ms, store_ms, bytes_uploaded.  Medians over --rounds rounds at
the end, and the one condition the feature has to meet: the in-place edit is not slower than the destroy + create + begin beside it.
No figure was fixed before the first run: none of them had been measured.

    python tools/topology_bench.py [--configs C5,C4] [--rounds 5] [--count 1000] [--log FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elevenrender_amd import render, scenes, topology  # noqa: E402

OUT = []


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


def manager(sc, max_bounces):
    rm = render.RenderingManager(render.RenderParameters(max_bounces=max_bounces, device="hip:0"))
    t0 = time.perf_counter()
    rm.start_rendering(sc)
    return rm, (time.perf_counter() - t0) * 1e3


def lists_of(sc, first, count, shift):
    """remove [first, first + count), append the same triangles moved by `shift`"""
    ids = np.arange(first, first + count)
    tail = {k: np.ascontiguousarray(getattr(sc, k)[first:first + count]) for k in topology.ARRAYS}
    tail["vertices"] = np.ascontiguousarray(tail["vertices"] + np.asarray(shift, np.float32))
    return dict(remove=ids, append=tail)


def timed_edit(rm, kw):
    rm.render(1)
    t0 = time.perf_counter()
    rm.topology(**kw)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, rm.topology_info()


def bench(name, sc, max_bounces, rounds, count):
    say(f"== {name}: {sc.tri_count} triangles, {sc.x_res}x{sc.y_res}, {len(sc.materials)} materials, {len(sc.textures)} textures, HDRI {sc.hdri[1]}x{sc.hdri[2]}, "
        f"max_bounces {max_bounces}; every edit removes {count} triangles and appends {count}")
    rm, first_ms = manager(sc, max_bounces)
    say(f"   er_scene_create + er_render_begin {first_ms:.1f} ms wall, builder {rm.accel_info()['builder']}, build_ms {rm.accel_info()['build_ms']:.1f}")
    rm.render(2)
    cur = sc
    rows = {2: [], 1: [], "fresh": []}
    for k in range(rounds):
        rm.edit(materials=cur.materials, material_id=cur.material_id)      # another call writes material ids: the store goes (not timed)
        for want in (2, 1):
            first = (17 + 2 * k + (want == 1)) * count % max(cur.tri_count - count, 1)
            kw = lists_of(cur, first, count, (0.01 * (k + 1), 0.0, 0.0))
            wall, info = timed_edit(rm, kw)
            cur = topology.apply(cur, **kw)
            say(f"   round {k} path {info['path']}: er_render_topology {wall:9.2f} ms wall (edit_ms {info['edit_ms']:.2f}, build_ms {info['build_ms']:.2f}, store_ms {info['store_ms']:.3f}, "
                f"bytes_uploaded {info['bytes_uploaded']}, tri_count {info['tri_count']})")
            if info["path"] != want:
                say(f"   !! expected path {want}")
            rows[want].append((wall, info["edit_ms"], info["build_ms"], info["store_ms"], info["bytes_uploaded"]))
        rm.render(1)
        other, _ = manager(cur, max_bounces)      # a begun scene of the same size, so that the destroy is timed on something real
        other.render(1)
        t0 = time.perf_counter()
        other.close()
        destroy = (time.perf_counter() - t0) * 1e3
        fresh, begin = manager(cur, max_bounces)
        build = fresh.accel_info()["build_ms"]
        fresh.close()
        say(f"   round {k} fresh : er_scene_destroy {destroy:7.2f} ms + er_scene_create + er_render_begin {begin:9.2f} ms = {destroy + begin:9.2f} ms wall (build_ms {build:.2f})")
        rows["fresh"].append((destroy + begin, destroy, begin, build))
    rm.close()
    med = lambda xs, i: float(np.median([x[i] for x in xs]))
    say(f"   medians of {rounds} rounds:")
    for p in (2, 1):
        say(f"   {name} path {p}: er_render_topology {med(rows[p], 0):9.2f} ms wall, edit_ms {med(rows[p], 1):9.2f}, build_ms {med(rows[p], 2):8.2f}, store_ms {med(rows[p], 3):7.3f}, "
            f"bytes_uploaded {int(med(rows[p], 4))}")
    f = med(rows["fresh"], 0)
    say(f"   {name} fresh : destroy + create + begin {f:9.2f} ms wall (destroy {med(rows['fresh'], 1):.2f}, create + begin {med(rows['fresh'], 2):.2f}, build_ms {med(rows['fresh'], 3):.2f})")
    for p in (2, 1):
        say(f"   {name} path {p} / fresh = {med(rows[p], 0) / f:.3f}   in place not slower: {med(rows[p], 0) <= f}")
    say(f"   {name} path 1 / path 2 = {med(rows[1], 0) / med(rows[2], 0):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C5,C4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--log")
    args = ap.parse_args()
    for cfg in args.configs.split(","):
        if cfg == "C5":
            bench("C5", scenes.torture(), 8, args.rounds, args.count)
        elif cfg == "C4":
            bench("C4", scenes.blob_instances(), 8, args.rounds, args.count)
        elif cfg == "small":      # (a quick pass over the tool itself)
            bench("small", scenes.torture(n_tris=30000, x_res=64, y_res=48, n_materials=4, tex_size=16, hdri_size=(16, 8)), 4, args.rounds, min(args.count, 100))
        else:
            raise SystemExit(f"unknown config {cfg}")
        if args.log:
            with open(args.log, "w") as f:
                f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
