#!/usr/bin/env python3
"""What the id pass and its consumers cost, measured on one GPU.

On the C2-style soup (1 M triangles, seed 12345) at 1280x720 and 1920x1080, with an object table of 64 objects (triangle t in object
t % 64 unless t % 5 == 0), everything in one process, the two sides of each comparison alternated, medians of --rounds (7):
  pass    er_render_ids(4) against er_render_features(4): device time (HIP events, ErIdInfo.ms / ErFeatureInfo.ms) and wall time.  The
          feature pass is the yardstick: it is the code of the commit before.
  pick    er_pick of one pixel (the first one after er_render_begin pays for the tri -> object map: reported apart), er_pick_rect of the
          middle quarter of the frame per kind (the sizing call and the call that fetches), against a camera-only er_render_update --
          the cheapest way there was to ask the library anything about a changed view.
  matte   er_id_matte of eight objects against er_read_pass of BEAUTY: both move one plane over PCIe, 4 against 16 bytes per pixel.

    python tools/ids_bench.py [--rounds 7] [--log profiles/ids_bench.log]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elevenrender_amd import abi, render, scenes  # noqa: E402

LOG = None

EXPECTATION = """expectation, written before the first run: nobody has measured any of these.
  pass   er_render_ids(4) costs about what er_render_features(4) costs (4.8 ms at 720p on this scene, DESIGN.md 3e): the same four
         traversals per pixel; it drops the attribute fetch and the albedo texel of every hit and adds three rankings of at most four
         LDS words and six 16-byte stores per pixel instead of two.  Within +-15 % of the feature pass at both sizes.
  pick   one wave, one ray, two small copies and a 40-byte allocation: launch latency, a few tens of microseconds, and far below a
         camera-only update.  The first pick uploads the table (1 M ids) and pays a millisecond or so once.
  rect   a memset and four launches over tri_count marks for TRIANGLE (4 MB), almost nothing for OBJECT and MATERIAL: a tenth of a
         millisecond or two, twice for sizing + fetching; still below the camera-only update.
  matte  4 bytes per pixel over PCIe against er_read_pass's 16 and no gather kernel of four planes: faster than er_read_pass."""


def say(line=""):
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def med(xs):
    return statistics.median(xs)


def shifted_camera(cam, d):
    c = abi.ErCamera.from_buffer_copy(cam)
    c.position = abi.ErVec3(cam.position.x + d[0], cam.position.y + d[1], cam.position.z + d[2])
    return c


def bench(w, h, rounds):
    sc = scenes.soup(1_000_000, w, h, seed=12345)
    t = np.arange(sc.tri_count)
    objects = [t[(t % 64 == o) & (t % 5 != 0)].astype(np.uint32) for o in range(64)]
    say(f"== C2-style soup: {sc.tri_count} triangles, {w}x{h}, 64 objects over {sum(len(o) for o in objects)} triangles")
    rm = render.RenderingManager(render.RenderParameters(max_bounces=8, device="hip:0"))
    rm.start_rendering(sc)
    rm.set_objects(objects)
    first_pick = wall(lambda: rm.pick(w // 2, h // 2))
    rm.render_features(4)
    rm.render_ids(4)      # (warm: both allocate their planes at the first call)
    ids_ms, feat_ms, ids_wall, feat_wall = [], [], [], []
    for _ in range(rounds):
        ids_wall.append(wall(lambda: rm.render_ids(4)))
        ids_ms.append(rm.id_info()["ms"])
        feat_wall.append(wall(lambda: rm.render_features(4)))
        feat_ms.append(rm.feature_info()["ms"])
    info = rm.id_info()
    say(f"   pass   er_render_ids(4) {med(ids_ms):.3f} ms device, {med(ids_wall):.3f} ms wall | er_render_features(4) {med(feat_ms):.3f} ms device, "
        f"{med(feat_wall):.3f} ms wall | ids / features {med(ids_ms) / med(feat_ms):.3f} (device)   [{info['rays']} rays, overflow {info['overflow_pixels']}]")
    say(f"          every round, device ms: ids {' '.join(f'{x:.3f}' for x in ids_ms)} | features {' '.join(f'{x:.3f}' for x in feat_ms)}")
    cams = [shifted_camera(sc.camera, (0.01 * (k % 2), 0.0, 0.0)) for k in range(2)]
    rect = (w // 4, h // 4, w // 4 + w // 2, h // 4 + h // 2)
    pick_ms, cam_ms, rect_ms = [], [], {k: [] for k in ("triangle", "object", "material")}
    found = {}
    for k in range(rounds):
        rm.render_ids(4)
        pick_ms.append(wall(lambda: rm.pick((w // 2 + 37 * k) % w, (h // 2 + 11 * k) % h)))
        for kind in rect_ms:
            rect_ms[kind].append(wall(lambda: found.__setitem__(kind, len(rm.pick_rect(*rect, kind)))))
        cam_ms.append(wall(lambda: rm.update(camera=cams[k % 2])))
    say(f"   pick   er_pick {med(pick_ms) * 1e3:.1f} us (the first after er_objects_set, with the table's upload: {first_pick:.3f} ms) | "
        f"camera-only er_render_update {med(cam_ms):.3f} ms")
    say("   rect   middle quarter, sizing call + fetch: " + " | ".join(f"{kind} {med(v):.3f} ms ({found[kind]} ids)" for kind, v in rect_ms.items()))
    rm.render_ids(4)
    rm.render(1)
    matte_ms, read_ms = [], []
    for _ in range(rounds):
        matte_ms.append(wall(lambda: rm.id_matte("object", [1, 2, 3, 5, 8, 13, 21, 34])))
        read_ms.append(wall(lambda: rm.get_pass("beauty")))
    say(f"   matte  er_id_matte of 8 objects {med(matte_ms):.3f} ms | er_read_pass BEAUTY {med(read_ms):.3f} ms | matte / read {med(matte_ms) / med(read_ms):.3f}")
    rm.close()


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    LOG = args.log
    if LOG:
        open(LOG, "w").close()
    say(EXPECTATION)
    say()
    for w, h in ((1280, 720), (1920, 1080)):
        bench(w, h, max(3, args.rounds))


if __name__ == "__main__":
    main()
