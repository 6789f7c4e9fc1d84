"""Scenes whose paths live as long as max_bounces says (a module for the tests, not a conftest).

In an ordinary scene a path ends after a handful of iterations whatever max_bounces is: DisneySample often returns a direction below the
surface, the path passes through the wall it sits on, and the next ray misses.  `shells` wraps a few blobs AND the camera in n_shells
concentric, inward-facing boxes 0.05 apart: a path that leaks through one shell hits the next.  With 64 shells every path of a 16 x 12
frame runs exactly max_bounces iterations (tests/test_long_path_scenes_cpu.py asserts it for every value the GPU tests use); with 2 shells
the lengths spread from 1 to max_bounces, which at max_bounces 32 puts pixels on both sides of the streaming kernel's 7-bit draw count
(csrc/er_stream.hip ST_DRAWS_MASK) and of its clamped mean length (ST_LONG_SHIFT).

Two variants, because ER_FLAG_POINT_LIGHTS and ER_FLAG_MESH_LIGHTS may not both see lights: `shells` has one emissive wall per shell and no
point lights; `shells_point_lights` has point lights inside the innermost shell and no emissive wall.

All randomness comes from scenes.Rand (through scenes.blob_instances and scenes.point_lights)."""
import numpy as np

from elevenrender_amd import abi, scenes

f32 = np.float32

BLOBS, WALL, LAMP = 0, 1, 2      # material ids
FIRST_GAP, SHELL_GAP = 0.5, 0.05
N_POINT_LIGHTS = 4


def box_triangles(lo, hi):
    """12 triangles of the axis-aligned box [lo, hi], wound so that cross(e1, e2) faces the interior, as scenes.cornell winds its walls;
    the last two are the ceiling (y = hi)."""
    x0, y0, z0 = (float(v) for v in lo)
    x1, y1, z1 = (float(v) for v in hi)

    def quad(p0, p1, p2, p3):
        return [[p0, p1, p2], [p0, p2, p3]]
    t = []
    t += quad([x0, y0, z0], [x0, y0, z1], [x1, y0, z1], [x1, y0, z0])   # floor, normal +y
    t += quad([x0, y0, z1], [x0, y1, z1], [x1, y1, z1], [x1, y0, z1])   # back wall, normal -z
    t += quad([x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0])   # front wall (behind the camera), normal +z
    t += quad([x0, y0, z0], [x0, y1, z0], [x0, y1, z1], [x0, y0, z1])   # left wall, normal +x
    t += quad([x1, y0, z0], [x1, y0, z1], [x1, y1, z1], [x1, y1, z0])   # right wall, normal -x
    t += quad([x0, y1, z0], [x1, y1, z0], [x1, y1, z1], [x0, y1, z1])   # ceiling, normal -y
    return np.array(t, f32)


def shells(x_res=16, y_res=12, n_shells=64, seed=12345, emissive=True):
    """scenes.blob_instances(6 blobs of 200 triangles) and its camera inside n_shells concentric boxes: the first FIRST_GAP outside the
    bounds of geometry and camera, each next SHELL_GAP further out; 12 triangles a box with face_frame normals, a grey albedo of 0.9,
    and (emissive) an emission of (0.5, 0.5, 0.5) on the two ceiling triangles of every shell.  1 200 + 12 n_shells triangles."""
    sc = scenes.blob_instances(n_instances=6, tris_per_blob=200, x_res=x_res, y_res=y_res, seed=seed, grid=(3, 2, 1), spacing=0.6)
    cam = np.array([[sc.camera.position.x, sc.camera.position.y, sc.camera.position.z]], f32)
    pts = np.concatenate([sc.vertices.reshape(-1, 3), cam])
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    boxes, mats = [], []
    for k in range(n_shells):
        gap = FIRST_GAP + SHELL_GAP * k
        boxes.append(box_triangles(lo - gap, hi + gap))
        mats += [WALL] * 10 + [LAMP if emissive else WALL] * 2
    walls = np.concatenate(boxes)
    wn, wt = scenes.face_frame(walls)
    n = len(walls)
    unit = np.tile(np.array([[0, 0], [1, 0], [0, 1]], f32), (n, 1, 1))
    M = abi.default_material
    out = abi.SceneData(np.concatenate([sc.vertices, walls]), np.concatenate([sc.normals, wn]), np.concatenate([sc.tangents, wt]),
                        np.concatenate([sc.uvs, unit]), np.concatenate([sc.tangent_sign, np.ones(n, f32)]),
                        np.concatenate([sc.material_id, np.array(mats, np.int32)]),
                        [M(), M(albedo=(0.9, 0.9, 0.9)), M(albedo=(0.9, 0.9, 0.9), emission=(0.5, 0.5, 0.5))],
                        hdri=scenes.sky_hdri(64, 32), camera=sc.camera, x_res=x_res, y_res=y_res)
    assert out.tri_count == 1200 + 12 * n_shells
    return out


def shells_point_lights(x_res=16, y_res=12, n_shells=64, seed=12345):
    """`shells` without an emissive wall and with N_POINT_LIGHTS point lights inside the innermost shell (within the blobs' bounds), for
    ER_FLAG_POINT_LIGHTS: an opaque hit then draws 5 numbers instead of 4."""
    sc = shells(x_res, y_res, n_shells, seed, emissive=False)
    v = sc.vertices[:1200].reshape(-1, 3)
    sc.point_lights = scenes.point_lights(N_POINT_LIGHTS, seed=seed, lo=tuple(map(float, v.min(0))), hi=tuple(map(float, v.max(0))))
    sc._desc = None
    return sc


def emitter_order(sc):
    """the emitters of `shells` in the table order of a render begun with ER_FLAG_HOST_BUILD (ascending slot of the host builder's
    structure; no device needed) -- what Oracle.set_emitters takes"""
    slot_to_tri = abi.debug_bvh_dump(sc.vertices, sc.normals)["slot_to_tri"].astype(np.int64)
    lamp = np.asarray(sc.material_id)[slot_to_tri] == LAMP
    return slot_to_tri[lamp].astype(np.int32)


def draw_count(recs, per_opaque):
    """The random numbers one sample drew, replayed from the oracle's trace records as csrc/er_stream.hip guesses them: 5 for the camera
    ray, 1 per iteration that hit (the opacity test), per_opaque more for an opaque hit -- 4 (HDRI cell, three for the BRDF sample), 5 with
    point lights, 7 with mesh lights."""
    hits = sum(1 for r in recs if r.tri >= 0)
    opaque = sum(1 for r in recs if r.tri >= 0 and r.opaque)
    return 5 + hits + per_opaque * opaque


def traced_pixels(sc, n, seed=5):
    """the pixels the per-bounce tests look at (GPU and CPU tests must agree on them)"""
    return np.random.default_rng(seed).choice(sc.x_res * sc.y_res, n, replace=False)
