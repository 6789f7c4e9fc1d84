#!/usr/bin/env python3
"""What er_render_edit costs beside the two ways there were before it, measured on one GPU.

On the scenes of BASELINE configs C5 (scenes.torture(): 1 M triangles, 64 materials of three 256 x 256 textures, a 2048 x 1024 HDRI,
1920x1080) and C2 (the same soup, one material, no texture), five edits of a begun scene:
  a  constants only: one material's roughness, metallic and albedo
  b  one material's roughness texture reassigned (another material's roughness texture)          [C5]
  c  one texture replaced by new texels of the same size                                          [C5]
  d  a new HDRI of the same size
  e  a new HDRI of twice the size (the first round grows the pool's allocation, the later ones find it large enough)
  f  all bits in one call: the camera, every vertex (+ (40, -3, 7)), a's constants, c's texture [C5], d's HDRI
Per round, alternated on one box: the edit (wall time of er_render_edit, and ErEditInfo.texture_stage / texture_stage_ms), then
er_render_begin again on the same begun scene (wall), then er_scene_create + er_render_begin of the edited description (wall).  Every
round's edit is a real change (the rounds go back and forth between two values).  Medians over --rounds rounds at the end.

    python tools/edit_bench.py [--configs C5,C2] [--rounds 5] [--log FILE]
"""
import argparse
import copy
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


def manager(sc, max_bounces):
    rm = render.RenderingManager(render.RenderParameters(max_bounces=max_bounces, device="hip:0"))
    t0 = time.perf_counter()
    rm.start_rendering(sc)
    return rm, (time.perf_counter() - t0) * 1e3


def begin_again(rm, max_bounces):
    p = abi.ErRenderParams(rm.pars.sampleTarget, rm.pars.block_size, max_bounces, 0, 0, 1, 0)
    t0 = time.perf_counter()
    abi.check(rm.lib.er_render_begin(rm.handle, C.byref(p)))
    return (time.perf_counter() - t0) * 1e3


def with_changes(sc, materials=None, textures=None, hdri=None, vertices=None, camera=None):
    out = copy.copy(sc)
    out._desc = None
    if vertices is not None:
        out.vertices = vertices
    if camera is not None:
        out.camera = camera
    if materials is not None:
        out.materials = materials
    if textures is not None:
        out.textures = textures
    if hdri is not None:
        out.hdri = hdri
    return out


def material_with(m, **kw):
    out = abi.ErMaterial.from_buffer_copy(m)
    for k, v in kw.items():
        setattr(out, k, abi.ErVec3(*v) if isinstance(v, tuple) else v)
    return out


def edits_of(sc, textured):
    """name -> (state A, state B): (edit arguments, edited description) each; round k applies A if k is even, B if odd, onto the other"""
    mats = sc.materials
    out = {}
    ma = [material_with(mats[0], roughness=0.3, metallic=0.7, albedo=(0.8, 0.3, 0.2))] + mats[1:]
    mb = [material_with(mats[0], roughness=0.6, metallic=0.1, albedo=(0.2, 0.3, 0.8))] + mats[1:]
    out["a constants"] = ((dict(materials=ma), with_changes(sc, materials=ma)), (dict(materials=mb), with_changes(sc, materials=mb)))
    if textured:
        ra = [material_with(mats[0], roughness_tex=mats[1].roughness_tex)] + mats[1:]
        out["b assignment"] = ((dict(materials=ra), with_changes(sc, materials=ra)), (dict(materials=mats), with_changes(sc, materials=mats)))
        i = mats[0].roughness_tex
        new = scenes.value_noise_texture(sc.textures[i][1], 4242)
        new = (abi._f32(new[0]),) + tuple(new[1:])
        keep = [None] * len(sc.textures)
        ta, tb = list(keep), list(keep)
        ta[i], tb[i] = new, sc.textures[i]
        full = list(sc.textures)
        full[i] = new
        out["c texture"] = ((dict(textures=ta), with_changes(sc, textures=full)), (dict(textures=tb), with_changes(sc, textures=list(sc.textures))))
    d, w, h, ch, flt = sc.hdri
    same = (np.ascontiguousarray(d[:, ::-1] * np.float32(0.9)), w, h, ch, flt)
    out["d hdri, same size"] = ((dict(hdri=same), with_changes(sc, hdri=same)), (dict(hdri=sc.hdri), with_changes(sc, hdri=sc.hdri)))
    big = scenes.sky_hdri(2 * w, 2 * h) if w > 1 else (np.full((2, 2, 3), 0.4, np.float32), 2, 2, 3, 0)
    big = (abi._f32(big[0]),) + tuple(big[1:])
    out["e hdri, twice the size"] = ((dict(hdri=big), with_changes(sc, hdri=big)), None)      # (B: back to the scene's own, not measured)
    shift = np.array([40.0, -3.0, 7.0], np.float32)
    moved = np.ascontiguousarray((sc.vertices.reshape(-1, 3, 3) + shift).reshape(sc.vertices.shape))
    cam = abi.ErCamera.from_buffer_copy(sc.camera)
    cam.position = abi.ErVec3(sc.camera.position.x + 40.0, sc.camera.position.y - 3.0, sc.camera.position.z + 7.0)
    fa = dict(camera=cam, vertices=moved, materials=ma, hdri=same)
    fb = dict(camera=sc.camera, vertices=sc.vertices, materials=mb, hdri=sc.hdri)
    if textured:
        fa["textures"], fb["textures"] = ta, tb
    out["f all bits"] = ((fa, with_changes(sc, ma, full if textured else None, same, moved, cam)),
                         (fb, with_changes(sc, mb, list(sc.textures) if textured else None, sc.hdri)))
    return out


def bench(name, sc, max_bounces, rounds, textured):
    say(f"== {name}: {sc.tri_count} triangles, {sc.x_res}x{sc.y_res}, {len(sc.materials)} materials, {len(sc.textures)} textures, HDRI {sc.hdri[1]}x{sc.hdri[2]}, max_bounces {max_bounces}")
    rm, first_ms = manager(sc, max_bounces)
    say(f"   er_scene_create + er_render_begin {first_ms:.1f} ms wall")
    rm.render(2)
    summary = []
    for tag, (A, B) in edits_of(sc, textured).items():
        ew, em, es, bw, fw = [], [], [], [], []
        for k in range(rounds):
            args, desc = A if (k % 2 == 0 or B is None) else B
            rm.render(1)
            t0 = time.perf_counter()
            rm.edit(**args)
            e = (time.perf_counter() - t0) * 1e3
            info = rm.edit_info()
            rm.render(1)
            b = begin_again(rm, max_bounces)      # (the begun scene holds the edited description: the host fill of the same pool)
            rm.render(1)
            fresh, f = manager(desc, max_bounces)
            fresh.close()
            if B is None:
                rm.edit(hdri=sc.hdri)             # back, for the next round
            say(f"   {tag:24s} round {k}: er_render_edit {e:9.3f} ms wall (edit_ms {info['edit_ms']:.3f}, texture_stage {info['texture_stage']}, texture_stage_ms {info['texture_stage_ms']:.3f},"
                f" pool {info['pool_floats'] * 4 / 1e6:.1f} MB)   er_render_begin again {b:8.2f} ms   create + begin {f:8.2f} ms")
            ew.append(e); em.append(info["edit_ms"]); es.append(info["texture_stage_ms"]); bw.append(b); fw.append(f)
        summary.append((tag, np.median(ew), np.median(em), min(em), max(em), np.median(es), np.median(bw), np.median(fw)))
    rm.close()
    say(f"   medians of {rounds} rounds, ms:   edit wall   edit_ms (min .. max)   texture_stage_ms   er_render_begin again   create + begin")
    for tag, e, m, lo, hi, s, b, f in summary:
        say(f"   {name} {tag:24s} {e:10.3f} {m:9.3f} ({lo:.3f} .. {hi:.3f}) {s:18.3f} {b:24.2f} {f:16.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C5,C2")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log")
    args = ap.parse_args()
    for cfg in args.configs.split(","):
        if cfg == "C5":
            bench("C5", scenes.torture(), 8, args.rounds, True)
        elif cfg == "C2":
            bench("C2", scenes.soup(1_000_000, 1920, 1080, seed=12345), 8, args.rounds, False)
        elif cfg == "small":      # (a quick pass over the tool itself)
            bench("small", scenes.torture(n_tris=600, x_res=64, y_res=48, n_materials=4, tex_size=16, hdri_size=(16, 8)), 4, args.rounds, True)
        else:
            raise SystemExit(f"unknown config {cfg}")
        if args.log:
            with open(args.log, "w") as f:
                f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
