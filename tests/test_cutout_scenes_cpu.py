"""tests/cutout_scenes.py on a machine without a GPU: the oracle and numpy alone.  (a) The replay of the pass that sees through cut-outs
reaches, on `layers()` at 4 rays per pixel, every class of ray the GPU test then holds the device to -- a scene that misses one could
hide a failure.  (b) On the copy of the scene whose opacities are only 0 and 1 the rule's hit for ray 0 of every pixel is the first
shaded hit of the oracle's own first sample: the rule is the render's behaviour wherever the draw cannot matter."""
import numpy as np

import cutout_scenes as cs
import oracle as orc
from elevenrender_amd import first_hit, ids

f32 = np.float32


def test_the_scene_is_what_its_docstring_says():
    sc = cs.layers()
    assert (sc.x_res, sc.y_res) == (44, 28) and sc.x_res % 8 and sc.y_res % 8          # partial tiles on both edges
    assert 32 <= sc.tri_count <= 48
    objects = cs.table(sc)
    listed = np.concatenate(objects)
    assert len(np.unique(listed)) == len(listed) and 0 < sc.tri_count - len(listed) <= 6          # disjoint; a few triangles in none
    of = ids.object_of(sc.tri_count, objects)
    assert len({int(of[sc.spans[k][0]]) for k in ("wall", "A", "B", "C", "D", "E", "F", "G")}) == 8
    op = sc.textures[1][0]
    assert sc.textures[1][1:] == (5, 3, 2, 1) and op[..., 0].min() < -1.2 and op[..., 0].max() > 2.2
    assert sc.materials[cs.M_F].opacity == 0.5 and sc.materials[cs.M_D].opacity == 0.0
    b = cs.layers(binary=True)
    assert {float(m.opacity) for m in b.materials} == {0.0, 1.0} and set(np.unique(b.textures[1][0])) == {0.0, 1.0} and b.textures[1][4] == 0
    assert (b.vertices.view(np.uint32) == sc.vertices.view(np.uint32)).all()


def test_the_replay_reaches_every_class_of_ray():
    sc = cs.layers()
    npx = sc.x_res * sc.y_res
    v = cs.pass_replay(4)
    c = cs.counters(v)
    print(c)
    hit, layers = v["tri"] >= 0, v["layers"]
    assert c["rays"] == 4 * npx
    assert (hit & (layers == 0)).sum() >= 200 and (~hit & (layers == 0)).sum() >= 50          # 0 layers: a plain hit, a plain miss
    assert (layers == 1).sum() >= 100 and (layers == 2).sum() >= 4
    assert (hit & (layers >= 3)).sum() >= 20                                                   # through the whole stack (A) to the wall
    assert c["rays_capped"] >= 50 and (layers[v["capped"]] == cs.MAX_BOUNCES).all() and not hit[v["capped"]].any()
    assert c["rays_through_to_miss"] >= 20 and not (v["to_miss"] & (hit | v["capped"])).any()
    assert c["rays_through"] == int((layers > 0).sum()) and c["layers_skipped"] > c["rays_through"]
    at = hit & (v["opacity"] == first_hit.DEFAULT_THRESHOLD)                                   # stopped at opacity == threshold: (F)
    assert at.sum() >= 20 and (sc.material_id[v["tri"][at]] == cs.M_F).all()
    # the textured card (B): stopped and passed, with opacities outside [0, 1] on both sides among them
    b_first = cs.pass_replay(4, cutouts=False)
    on_b = (b_first["tri"] >= 0) & (sc.material_id[np.maximum(b_first["tri"], 0)] == cs.M_B)
    a = b_first["opacity"][on_b]
    assert (a < 0).sum() >= 5 and (a > 1).sum() >= 5 and ((a >= 0) & (a < 0.5)).sum() >= 5 and ((a >= 0.5) & (a <= 1)).sum() >= 5
    # at least one pixel whose four rays do not all agree -- in what they hit and in how many layers they passed
    tri4, lay4 = v["tri"].reshape(npx, 4), layers.reshape(npx, 4)
    assert ((tri4 != tri4[:, :1]).any(1)).sum() >= 10 and ((lay4 != lay4[:, :1]).any(1)).sum() >= 10
    inside_b = on_b.reshape(npx, 4).all(1)
    assert (inside_b & (lay4 != lay4[:, :1]).any(1)).sum() >= 1                                # ... the threshold crossing inside a pixel
    # the opaque quad in front of a cut-out (E): its rays stop at once
    e0 = sc.spans["E"][0]
    on_e = hit & (v["tri"] >= e0) & (v["tri"] < e0 + 2)
    assert on_e.sum() >= 50 and (layers[on_e] == 0).all()
    # and the mode changes what the pass reports
    assert (b_first["tri"] != v["tri"]).sum() >= 400 and (b_first["layers"] == 0).all() and not b_first["capped"].any()


def test_the_key_rays_reach_the_classes_too():
    sc = cs.layers()
    of = ids.object_of(sc.tri_count, cs.table(sc))
    key, v = cs.key_plane(sc, of)
    c = cs.counters(v)
    assert c["rays"] == sc.x_res * sc.y_res and c["rays_capped"] >= 10 and c["rays_through_to_miss"] >= 5 and (v["layers"] >= 3).sum() >= 5
    assert (key["obj"][key["hit"] != 0] == 0xFFFFFFFF).sum() >= 1 and (key["dist"][key["hit"] == 0] == 0).all()


def test_on_binary_opacities_the_rule_is_the_renders_first_shaded_hit():
    """ray 0 of every pixel against Oracle.trace_pixel's first sample: the first record the oracle shaded (opaque) is the replay's hit;
    a path with none (it left the scene, or spent its max_bounces inside cut-outs) is the replay's miss"""
    sc = cs.layers(binary=True)
    npx = sc.x_res * sc.y_res
    v = cs.take(cs.pass_replay(4, binary=True), 1)
    o = orc.Oracle(sc, math_mode=orc.MATH_ER, max_bounces=cs.MAX_BOUNCES)
    want_tri, want_pos, passed = np.full(npx, -1, np.int64), np.zeros((npx, 3), f32), np.zeros(npx, np.int64)
    for idx in range(npx):
        for rec in o.trace_pixel(idx):
            if rec.tri >= 0 and rec.opaque:
                want_tri[idx], want_pos[idx] = rec.tri, rec.position[:]
                break
            passed[idx] += rec.tri >= 0
    o.close()
    assert (v["tri"] == want_tri).all(), int((v["tri"] != want_tri).sum())
    hit = want_tri >= 0
    assert (v["rec"][hit, 0:3].view(np.uint32) == want_pos[hit].view(np.uint32)).all()
    assert (v["layers"] == passed).all()
    assert (hit & (passed >= 3)).sum() >= 5 and (~hit & (passed == cs.MAX_BOUNCES)).sum() >= 10 and (~hit & (passed > 0) & (passed < cs.MAX_BOUNCES)).sum() >= 5
