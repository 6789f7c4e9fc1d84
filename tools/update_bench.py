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

--sparse: one object moved back and forth -- C4: the middle blob instance onto its neighbour's place; C2: the innermost
1 % of the triangles by (0.05, 0.02, 0.03) -- through er_render_update_sparse on one manager (A) and through er_render_update with
the complete arrays on another (B), and a camera-only update on A, alternated, --rounds (at least 5) times each in one process:
update_ms and refit_ms of the first sparse call (path 2: the topology has no kept boxes yet) and the medians of the later ones
(path 1), of the full update and of the camera-only update, the sparse / full ratio and the sparse update's distance to the
camera-only one; then the rate on A against B (the same bytes: a sanity line).

    python tools/update_bench.py --sparse [--configs C2,C4] [--rounds 5] [--log FILE]

--transform (C4 only): two objects posed back and forth -- (a) one blob instance, onto its neighbour's place; (b) the first
tenth of the instances as ONE object, turned a little about its centre -- through er_render_transform on one manager (A) and through
er_render_update_sparse on another (B), whose caller poses the object's rest arrays in numpy first (elevenrender_amd/transform.py;
timed apart), alternated, --rounds (at least 7) times each in one process: the first call of either kind, then the medians of the later
ones: wall time of the call, update_ms, refit_ms, bytes uploaded, the caller's numpy time, and transform / sparse.

    python tools/update_bench.py --transform [--rounds 7] [--log FILE]

--skin (C4 only): the same two objects, each with a seeded skin of 32 bones and 4 influences per corner, deformed back and
forth between two seeded palettes -- through er_render_skin on one manager (A) and through er_render_update_sparse on another (B),
whose caller skins the object's rest arrays in numpy first (elevenrender_amd/skin.py; timed apart), alternated as above.

    python tools/update_bench.py --skin [--rounds 7] [--log FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elevenrender_amd import abi, render, scenes, skin, transform  # noqa: E402

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


def sparse_bench(name, sc, max_bounces, steps, rounds, instances):
    v = sc.vertices.reshape(-1, 3, 3)
    n = len(v)
    if instances:
        per = n // instances
        mid = instances // 2
        ids = np.arange(mid * per, (mid + 1) * per)
        delta = (v[(mid + 1) * per:(mid + 2) * per].reshape(-1, 3).mean(0) - v[ids].reshape(-1, 3).mean(0)).astype(np.float32)
    else:
        ids = np.argsort(np.abs(v).reshape(n, -1).max(1), kind="stable")[:n // 100]
        delta = np.array([0.05, 0.02, 0.03], np.float32)
    ids = np.random.default_rng(3).permutation(ids)
    say(f"== {name} (sparse updates): {n} triangles, {sc.x_res}x{sc.y_res}, max_bounces {max_bounces}; {len(ids)} triangles ({100.0 * len(ids) / n:.3f} %) moved by {delta.tolist()} and back")
    a, _ = manager(sc, max_bounces)
    b, _ = manager(sc, max_bounces)
    rate(a, 2)
    rate(b, 2)
    home, away = np.ascontiguousarray(v[ids]), np.ascontiguousarray(v[ids] + delta)
    full_home, full_away = v, v.copy()
    full_away[ids] = away
    cam2 = shifted_camera(sc.camera, (0.05, 0.02, -0.1))
    rows = {"sparse": [], "full": [], "camera": []}
    for k in range(rounds + 1):      # round 0: the first call of either kind on this topology
        out = k % 2 == 0
        a.update(tri_ids=ids, vertices=away if out else home)
        si, ui = a.sparse_info(), a.update_info()
        b.update(vertices=full_away if out else full_home)
        fi = b.update_info()
        a.update(camera=cam2 if out else sc.camera)
        ci = a.update_info()
        say(f"   round {k}: sparse update_ms {ui['update_ms']:8.3f} refit_ms {si['refit_ms']:7.3f} path {si['path']} why_full {si['why_full']} dirty nodes {si['dirty_nodes2']} / {si['dirty_nodes8']}"
            f" uploaded {si['bytes_uploaded']} B   full update_ms {fi['update_ms']:8.3f} refit_ms {fi['refit_ms']:7.3f}   camera update_ms {ci['update_ms']:7.3f}")
        if k:
            rows["sparse"].append((ui["update_ms"], si["refit_ms"], si["path"]))
            rows["full"].append((fi["update_ms"], fi["refit_ms"]))
            rows["camera"].append(ci["update_ms"])
    med = lambda xs: float(np.median(xs))
    su, sr = med([r[0] for r in rows["sparse"]]), med([r[1] for r in rows["sparse"]])
    fu, fr = med([r[0] for r in rows["full"]]), med([r[1] for r in rows["full"]])
    cu = med(rows["camera"])
    say(f"   medians of rounds 1..{rounds} (paths {sorted(set(r[2] for r in rows['sparse']))}): sparse update_ms {su:.3f} refit_ms {sr:.3f}   full update_ms {fu:.3f} refit_ms {fr:.3f}"
        f"   camera update_ms {cu:.3f}   sparse / full {su / fu:.4f} (refit {sr / fr:.4f})   sparse - camera {su - cu:.3f} ms")
    ra, rb = [], []
    for _ in range(min(rounds, 3)):
        ra.append(rate(a, steps))
        rb.append(rate(b, steps))
    say(f"   Msamples/s of {steps} steps, A = after the sparse moves {' '.join(f'{x:7.1f}' for x in ra)}   B = after the full updates {' '.join(f'{x:7.1f}' for x in rb)}"
        f"   median A/B {np.median(ra) / np.median(rb):.4f}")
    a.close()
    b.close()


def transform_bench(name, sc, max_bounces, rounds, instances):
    rest = [a.reshape(-1, 3, 3) for a in (sc.vertices, sc.normals, sc.tangents)]
    v = rest[0]
    n = len(v)
    per = n // instances
    mid = instances // 2
    blob = np.arange(mid * per, (mid + 1) * per)
    tenth = np.arange(0, (instances // 10) * per)
    delta = v[(mid + 1) * per:(mid + 2) * per].reshape(-1, 3).mean(0) - v[blob].reshape(-1, 3).mean(0)
    c = v[tenth].reshape(-1, 3).mean(0).astype(np.float64)
    a_, s_ = np.cos(0.02), np.sin(0.02)
    L = np.array([[a_, -s_, 0], [s_, a_, 0], [0, 0, 1]])
    home = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)
    cases = (("a", "one blob instance onto its neighbour's place", 0, blob, np.concatenate([np.eye(3), delta.astype(np.float64)[:, None]], 1).astype(np.float32)),
             ("b", "a tenth of the instances as one object, turned by 0.02 rad about its centre", 1, tenth, np.concatenate([L, (c - L @ c)[:, None]], 1).astype(np.float32)))
    say(f"== {name} (object transforms): {n} triangles, {sc.x_res}x{sc.y_res}, max_bounces {max_bounces}")
    a, _ = manager(sc, max_bounces)
    b, _ = manager(sc, max_bounces)
    rate(a, 2)
    rate(b, 2)
    t0 = time.perf_counter()
    a.set_objects([blob, tenth])
    say(f"   er_objects_set of {len(blob)} + {len(tenth)} triangles: {(time.perf_counter() - t0) * 1e3:.2f} ms wall; the rest copy on the device takes {112 * (len(blob) + len(tenth))} bytes")
    med = lambda xs: float(np.median(xs))
    for tag, what, obj, ids, away in cases:
        say(f"   ({tag}) {what}: {len(ids)} triangles ({100.0 * len(ids) / n:.2f} %)")
        parts = [np.ascontiguousarray(r[ids]) for r in rest]      # (the caller of the sparse path keeps its object's rest arrays)
        rows = []
        for k in range(rounds + 1):      # round 0: the first call of either kind on this topology (and the upload of the rest copy)
            m = away if k % 2 == 0 else home
            t0 = time.perf_counter()
            a.transform({obj: m})
            wa = (time.perf_counter() - t0) * 1e3
            ti, ua = a.transform_info(), a.update_info()
            t0 = time.perf_counter()
            pv, pn, pt = transform.pose(m, *parts)
            numpy_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            b.update(tri_ids=ids, vertices=pv, normals=pn, tangents=pt)
            wb = (time.perf_counter() - t0) * 1e3
            si, ub = b.sparse_info(), b.update_info()
            say(f"      round {k}: transform wall {wa:8.3f} update_ms {ua['update_ms']:8.3f} refit_ms {ti['refit_ms']:7.3f} path {ti['path']} why_full {ti['why_full']} dirty nodes {ti['dirty_nodes2']} / {ti['dirty_nodes8']}"
                f" uploaded {ti['bytes_uploaded']} B   sparse wall {wb:8.3f} update_ms {ub['update_ms']:8.3f} refit_ms {si['refit_ms']:7.3f} path {si['path']} uploaded {si['bytes_uploaded']} B"
                f"   caller's numpy {numpy_ms:8.3f} ms")
            if k:
                rows.append((wa, ua["update_ms"], ti["refit_ms"], wb, ub["update_ms"], si["refit_ms"], numpy_ms))
        m_ = [med([r[i] for r in rows]) for i in range(7)]
        say(f"      medians of rounds 1..{rounds}: transform wall {m_[0]:.3f} update_ms {m_[1]:.3f} refit_ms {m_[2]:.3f}   sparse wall {m_[3]:.3f} update_ms {m_[4]:.3f} refit_ms {m_[5]:.3f}"
            f"   caller's numpy {m_[6]:.3f}   transform / sparse: wall {m_[0] / m_[3]:.4f}, refit {m_[2] / m_[5]:.4f}; with the caller's numpy {m_[0] / (m_[3] + m_[6]):.4f}")
    a.close()
    b.close()


def skin_bench(name, sc, max_bounces, rounds, instances, bones=32):
    rest = [a.reshape(-1, 3, 3) for a in (sc.vertices, sc.normals, sc.tangents)]
    v = rest[0]
    n = len(v)
    per = n // instances
    mid = instances // 2
    blob = np.arange(mid * per, (mid + 1) * per)
    tenth = np.arange(0, (instances // 10) * per)
    rng = np.random.default_rng(17)

    def influences(size):      # 4 non-zero weights per corner, summing to 1 in float32 up to rounding, each within [0, 1]
        b = rng.integers(0, bones, size=(size, 3, 4)).astype(np.uint16)
        w = rng.uniform(0.1, 1.0, size=(size, 3, 4))
        return b, np.minimum((w / w.sum(-1, keepdims=True)).astype(np.float32), np.float32(1))

    def seeded_palette(ids, turn):      # per bone a small turn about z x a non-uniform scale about the object's centre, and a small shift
        c = v[ids].reshape(-1, 3).mean(0).astype(np.float64)
        P = np.empty((bones, 3, 4), np.float32)
        for k in range(bones):
            a = turn * rng.uniform(0.5, 1.0)
            L = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.diag(rng.uniform(0.95, 1.0, size=3))
            P[k] = np.concatenate([L, (c - L @ c + rng.normal(size=3) * 0.01)[:, None]], 1)
        return P

    say(f"== {name} (skinning): {n} triangles, {sc.x_res}x{sc.y_res}, max_bounces {max_bounces}; {bones} bones, 4 influences per corner")
    a, _ = manager(sc, max_bounces)
    b, _ = manager(sc, max_bounces)
    rate(a, 2)
    rate(b, 2)
    a.set_objects([blob, tenth])
    med = lambda xs: float(np.median(xs))
    for tag, what, obj, ids in (("a", "one blob instance", 0, blob), ("b", "a tenth of the instances as one object", 1, tenth)):
        say(f"   ({tag}) {what}: {len(ids)} triangles ({100.0 * len(ids) / n:.2f} %)")
        bw = influences(len(ids))
        t0 = time.perf_counter()
        a.set_skin(obj, (bw[0], bones), bw[1])
        say(f"      er_skin_set: {(time.perf_counter() - t0) * 1e3:.2f} ms wall; the influences on the device take {skin.INFLUENCE_BYTES * len(ids)} bytes")
        palettes = (seeded_palette(ids, 0.02), seeded_palette(ids, 0.01))
        parts = [np.ascontiguousarray(r[ids]) for r in rest]      # (the caller of the sparse path keeps its object's rest arrays)
        rows = []
        for k in range(rounds + 1):      # round 0: the first call of either kind on this topology (and the upload of rest copy and influences)
            P = palettes[k % 2]
            t0 = time.perf_counter()
            a.skin({obj: P})
            wa = (time.perf_counter() - t0) * 1e3
            ki, ua = a.skin_info(), a.update_info()
            t0 = time.perf_counter()
            pv, pn, pt = skin.pose(P, *bw, *parts)
            numpy_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            b.update(tri_ids=ids, vertices=pv, normals=pn, tangents=pt)
            wb = (time.perf_counter() - t0) * 1e3
            si, ub = b.sparse_info(), b.update_info()
            say(f"      round {k}: skin wall {wa:8.3f} update_ms {ua['update_ms']:8.3f} refit_ms {ki['refit_ms']:7.3f} path {ki['path']} why_full {ki['why_full']} dirty nodes {ki['dirty_nodes2']} / {ki['dirty_nodes8']}"
                f" uploaded {ki['bytes_uploaded']} B (influences {ki['influence_bytes']} B)   sparse wall {wb:8.3f} update_ms {ub['update_ms']:8.3f} refit_ms {si['refit_ms']:7.3f} path {si['path']}"
                f" uploaded {si['bytes_uploaded']} B   caller's numpy {numpy_ms:8.3f} ms")
            if k:
                rows.append((wa, ua["update_ms"], ki["refit_ms"], wb, ub["update_ms"], si["refit_ms"], numpy_ms))
        m_ = [med([r[i] for r in rows]) for i in range(7)]
        say(f"      medians of rounds 1..{rounds}: skin wall {m_[0]:.3f} update_ms {m_[1]:.3f} refit_ms {m_[2]:.3f}   sparse wall {m_[3]:.3f} update_ms {m_[4]:.3f} refit_ms {m_[5]:.3f}"
            f"   caller's numpy {m_[6]:.3f}   skin / sparse: wall {m_[0] / m_[3]:.4f}, refit {m_[2] / m_[5]:.4f}; with the caller's numpy {m_[0] / (m_[3] + m_[6]):.4f}")
    a.close()
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log")
    ap.add_argument("--rebuild", action="store_true", help="the rebuild policies of er_update_policy_set instead of the update / refit figures")
    ap.add_argument("--sparse", action="store_true", help="er_render_update_sparse against the full and the camera-only update")
    ap.add_argument("--transform", action="store_true", help="er_render_transform against er_render_update_sparse of the same pose (C4)")
    ap.add_argument("--skin", action="store_true", help="er_render_skin against er_render_update_sparse of the same deformation (C4)")
    ap.add_argument("--ratio", type=float, default=2.0, help="--rebuild: max_cost_ratio of the ER_REBUILD_AUTO runs")
    args = ap.parse_args()
    if args.log:
        global LOG
        LOG = args.log
        open(LOG, "w").close()
    if args.transform:
        transform_bench("C4", scenes.blob_instances(x_res=3840, y_res=2160), 8, max(7, args.rounds), 10000)
        return
    if args.skin:
        skin_bench("C4", scenes.blob_instances(x_res=3840, y_res=2160), 8, max(7, args.rounds), 10000)
        return
    for cfg in args.configs.split(","):
        if args.sparse:
            if cfg == "C2":
                sparse_bench("C2", scenes.soup(1_000_000, 1920, 1080, seed=12345), 8, args.steps, max(5, args.rounds), 0)
            elif cfg == "C4":
                sparse_bench("C4", scenes.blob_instances(x_res=3840, y_res=2160), 8, args.steps, max(5, args.rounds), 10000)
            else:
                raise SystemExit(f"unknown config {cfg}")
        elif args.rebuild:
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
