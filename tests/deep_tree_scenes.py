"""A small scene whose wide tree is deep enough to use the traversal's HBM stack levels (a module for the tests, not a conftest).

Every wide traversal keeps its first WF_LDS_STACK (8) stack entries in LDS and the deeper ones in an HBM spill area (csrc/er_trav.h,
trav_choose).  A balanced 8-wide tree over two-triangle leaves is about log8(n / 2) levels deep, so no scene small enough to compare with
the oracle bit for bit ever pushed a ninth entry.  `nested_shells` is SELF-SIMILAR instead: shell i is a ring of `per` triangles at
distance top * r^i from the world origin, shrinking towards it.  Every binned-SAH split peels off the largest shells and the rest becomes
a chain.  The shells lie along the diagonal (1, 1, 1), not along an axis, and that is what makes a ray descend the chain FIRST: the
builder gives a wide node's children the slots of their octant about the node's centre (er_collapse_bvh8), the traversal visits slots
in `slot ^ octant` order whatever the distances, and only on the diagonal is the chain -- the child nearest the origin in all three
coordinates -- in the slot that every ray of a camera looking along the diagonal visits first.  Such a ray leaves a sibling group on the
stack at almost every level (tests/test_deep_tree_scenes_cpu.py states and measures this without a GPU; tests/test_gpu_deep_tree.py
renders through it).  (Along +z the chain's slot depends on noise in x and y, and the same shells gave 1 to 4 entries.)

`first_descent_entries` replays the first descent of trav_choose / trav_apply on a dumped wide tree and counts the stack entries it
leaves: a lower bound on the deepest entry a ray reaches.

All randomness comes from scenes.Rand."""
import ctypes as C

import numpy as np

import accel_check
from elevenrender_amd import abi, scenes

f32 = np.float32
WF_LDS_STACK = 8                       # csrc/er_trav.h (both CPU and GPU tests compare the two with what er_debug_trace_rays_levels reports as compiled)
ER_STACK8 = accel_check.ER_STACK8      # csrc/er_bvh.h
MARGIN = 1e-4                          # relative; about 25 times the relative box padding tests/accel_check.py documents (4e-7 m)
# materials, dealt per triangle (0.2 / 0.35 / 0.3 / 0.15): plain grey, two coloured ones that let half / three quarters of the paths through (the continuation
# ray then starts in the middle of the chain), a smooth metal
GREY, HALF, QUARTER, METAL = 0, 1, 2, 3
# The camera's rotation (degrees about x, then y; camera_ray of csrc/er_device.h) that turns its +z onto the diagonal (1, 1, 1) / sqrt(3),
# and the same rotation as a matrix for the geometry
VIEW_DEGREES = (-float(np.degrees(np.arctan(np.sqrt(0.5)))), 45.0, 0.0)
_cx, _sx, _cy, _sy = np.sqrt(2.0 / 3.0), -np.sqrt(1.0 / 3.0), np.sqrt(0.5), np.sqrt(0.5)
VIEW = np.array([[_cy, 0, _sy], [0, 1, 0], [-_sy, 0, _cy]]) @ np.array([[1, 0, 0], [0, _cx, -_sx], [0, _sx, _cx]])


def nested_shells(x_res=24, y_res=16, top=4.0, smallest=3.4e-10, r=0.75, per=8, seed=1):
    """In the camera's frame (z the view direction, turned onto the diagonal by VIEW): shell i = 0, 1, ... while z = top * r^i >= smallest
    is a ring of `per` equilateral triangles of edge 0.3 z about the z axis, radius 0.25 z, triangle k at depth z (1 + 0.02 k).  The
    camera sits at -smallest / 10 on that axis and looks along it, so every shell lies in front of it and the view is the same at every
    scale.  The defaults give 81 shells, 648 triangles.

    The smallest edge is 0.3 * smallest and must stay at 1e-10 or more (asserted): the Moller-Trumbore determinant scales with edge^2,
    and 1e-20 is far inside the normal float range (1.2e-38), so the oracle on the CPU and the device cannot differ by how they treat
    denormals.  (Tri::hit rejects |det| < 1e-7, so triangles with an edge below about 3e-4 are never hit by either: the small shells
    shape the tree, the large ones are what the image shows.  The builders pad every box by 1e-6 of the scene's largest coordinate, so
    below about 1e-5 the shells stop lengthening the chain; the ratio top / smallest beyond that adds little depth.)

    To make the scene worth shading each triangle's plane is tilted at random (its normal within about 50 degrees of the direction to
    the camera, one in four flipped to face away from it, so paths bounce between shells), the ring turns by a random phase per shell,
    and the four materials above are dealt per triangle."""
    assert 0.3 * smallest >= 1e-10, "smallest edge below 1e-10: edge^2 must stay far inside the normal float range"
    rnd = scenes.Rand(seed, 7)
    zs = []
    z = float(top)
    while z >= smallest:
        zs.append(z)
        z *= r
    n = len(zs) * per
    zz = np.repeat(np.array(zs, np.float64), per)                               # [n]
    k = np.tile(np.arange(per, dtype=np.float64), len(zs))
    phase = np.repeat(rnd.u01(len(zs)).astype(np.float64), per)
    th = 2.0 * np.pi * (k / per + phase)
    centre = np.stack([0.25 * zz * np.cos(th), 0.25 * zz * np.sin(th), zz * (1.0 + 0.02 * k)], 1)
    tilt_v = rnd.uniform(-1, 1, n, 3).astype(np.float64)
    nrm = np.array([0.0, 0.0, -1.0]) + 0.7 * tilt_v
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    u = np.cross(nrm, np.array([0.0, 1.0, 0.0]))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(nrm, u)
    spin = 2.0 * np.pi * rnd.u01(n).astype(np.float64)
    u, v = (np.cos(spin)[:, None] * u + np.sin(spin)[:, None] * v), (-np.sin(spin)[:, None] * u + np.cos(spin)[:, None] * v)
    e = (0.3 * zz)[:, None]
    h = np.sqrt(3.0) / 2.0
    p0, p1, p2 = centre - 0.5 * e * u - (h / 3) * e * v, centre + 0.5 * e * u - (h / 3) * e * v, centre + (2 * h / 3) * e * v
    flip = rnd.u01(n) < 0.25
    tris = np.stack([p0, np.where(flip[:, None], p2, p1), np.where(flip[:, None], p1, p2)], 1) @ VIEW.T
    tris = tris.astype(f32)
    normals, tangents = scenes.face_frame(tris)
    uvs = np.tile(np.array([[0, 0], [1, 0], [0, 1]], f32), (n, 1, 1))
    deal = rnd.u01(n)
    mats = np.where(deal < 0.2, GREY, np.where(deal < 0.55, HALF, np.where(deal < 0.85, QUARTER, METAL))).astype(np.int32)
    M = abi.default_material
    materials = [M(albedo=(0.8, 0.8, 0.8)), M(albedo=(0.8, 0.3, 0.2), opacity=0.5), M(albedo=(0.2, 0.4, 0.8), opacity=0.25),
                 M(albedo=(0.9, 0.8, 0.5), metallic=1.0, roughness=0.3)]
    cam = abi.default_camera()
    cam.rotation = abi.ErVec3(*VIEW_DEGREES)
    cam.position = abi.ErVec3(*[float(c) for c in VIEW @ np.array([0.0, 0.0, -float(smallest) / 10.0])])
    out = abi.SceneData(tris, normals, tangents, uvs, np.ones(n, f32), mats, materials, hdri=scenes.sky_hdri(64, 32), camera=cam,
                        x_res=x_res, y_res=y_res)
    out.per = per      # (triangles per shell: shell i is the triangles i * per ... (i + 1) * per - 1)
    return out


def host_dump(sc):
    """the host builder's structure of a scene, with the records er_render_begin would upload: what accel_check.check takes (no device)"""
    return accel_check.host_records(sc, abi.debug_bvh_dump(sc.vertices, sc.normals))


def pixel_centre_rays(sc):
    """origins, dirs float32 [x_res * y_res, 3]: the pinhole ray through every pixel's centre (r1 = r2 = 0.5, bokeh 0), from the oracle's
    camera_ray -- the rays the first-hit passes trace, and the middle of the bundle a rendered pixel's samples come from"""
    import oracle as orc
    L = orc.lib()
    npx = sc.x_res * sc.y_res
    cam = abi.ErCamera.from_buffer_copy(sc.camera)
    cam.bokeh = 0
    origins, dirs = np.zeros((npx, 3), f32), np.zeros((npx, 3), f32)
    r = (C.c_float * 5)(0.5, 0.5, 0.0, 0.0, 0.0)
    for idx in range(npx):
        o, d = (C.c_float * 3)(), (C.c_float * 3)()
        L.oracle_camera_ray(C.byref(cam), sc.x_res, sc.y_res, idx % sc.x_res, idx // sc.x_res, r, orc.MATH_ER, o, d)
        origins[idx], dirs[idx] = o[:], d[:]
    return origins, dirs


def _slab_hit(lo, hi, o, idir, limit=None):
    """[R, 8] bool: the slab test of trav_apply_node (tmin <= tmax and tmax >= 0), in float64; lo, hi [R, 3, 8].  Without `limit` its
    pruning bound is left out; with limit [R] a box whose entry distance tmin exceeds it is pruned (tmin <= limit)"""
    a, b = (lo - o[:, :, None]) * idir[:, :, None], (hi - o[:, :, None]) * idir[:, :, None]
    tmin, tmax = np.minimum(a, b).max(1), np.maximum(a, b).min(1)
    hit = (tmin <= tmax) & (tmax >= 0.0)
    return hit if limit is None else hit & (tmin <= limit[:, None])


def first_descent_entries(dump, origins, dirs, margin=MARGIN, limits=None):
    """The first descent of trav_choose / trav_apply (csrc/er_trav.h) without its pruning, on the wide tree of `dump` (abi.debug_bvh_dump
    or RenderingManager.debug_read_accel): from the root, slab-test each inner slot's decoded box (accel_check.decode_wide_boxes), go to
    the nearest hit inner child -- the highest bit of the hit mask in `slot ^ octant` order, whatever the distances -- and count ONE
    entry for each level that leaves a hit inner sibling behind (trav_choose pushes the rest of the group), until a node has no hit
    inner child.  All pushes of a descent precede its first pop, so the count is a lower bound on the deepest stack entry the ray
    reaches, exact for that descent unless a box decision is marginal.

    Returns (entries int64 [R], marginal bool [R]): marginal = some decision on the ray's way changes when every face of the box moves
    in or out by `margin` times the box's largest |coordinate| (the traversal evaluates each plane with one fused multiply-add in
    float32 and the builders pad the boxes to cover that; a ray this close to a face may go either way).

    limits float32 [R]: the descent of a SHADOW query that finds no occluder on its way -- a box that the ray enters beyond limits[i] is
    pruned.  (The kernel prunes at limit + the largest lift + a rounding allowance, never below the limit, so this is a lower bound
    too; a box entered within `margin` x (scene extent + limit) of the limit makes the ray marginal.)"""
    nodes8 = dump["nodes8"]
    o = np.ascontiguousarray(origins, f32).reshape(-1, 3).astype(np.float64)
    d = np.ascontiguousarray(dirs, f32).reshape(-1, 3)
    R = len(o)
    entries, marginal = np.zeros(R, np.int64), np.zeros(R, bool)
    if len(nodes8) == 0 or R == 0:
        return entries, marginal
    with np.errstate(divide="ignore"):
        idir = np.clip(f32(1.0) / d, f32(-1e18), f32(1e18)).astype(np.float64)        # trav_begin
    oct7 = ((idir[:, 0] >= 0) * 1 + (idir[:, 1] >= 0) * 2 + (idir[:, 2] >= 0) * 4).astype(np.int64)
    blo, bhi = accel_check.decode_wide_boxes(nodes8)                                # float32 [N, 3, 8]
    blo, bhi = blo.astype(np.float64), bhi.astype(np.float64)
    imask_all = nodes8["imask"].astype(np.int64)
    child_base = nodes8["child_base"].astype(np.int64)
    slots = np.arange(8)
    extent = float(np.abs(np.concatenate([blo[0][np.isfinite(blo[0])], bhi[0][np.isfinite(bhi[0])]])).max())      # of the root's boxes
    lim = None if limits is None else np.ascontiguousarray(limits, f32).reshape(R).astype(np.float64)
    rays, node = np.arange(R), np.zeros(R, np.int64)
    for _ in range(ER_STACK8 + 1):
        if not len(rays):
            break
        lo, hi, oo, ii = blo[node], bhi[node], o[rays], idir[rays]
        inner = ((imask_all[node][:, None] >> slots) & 1).astype(bool)                # [R, 8]
        ll = None if lim is None else lim[rays]
        hit = _slab_hit(lo, hi, oo, ii, ll) & inner
        m = margin * np.maximum(np.abs(lo), np.abs(hi)).max(1)[:, None, :]           # [R, 1, 8]: per box
        # (the kernel's allowance beyond the limit is 4e-6 of scene scale + limit: `margin` of extent + limit covers it many times)
        slack = None if ll is None else margin * (extent + ll)
        grown = _slab_hit(lo - m, hi + m, oo, ii, None if ll is None else ll + slack) & inner
        shrunk = _slab_hit(lo + m, hi - m, oo, ii, None if ll is None else ll - slack) & inner
        marginal[rays] |= (grown != shrunk).any(1)
        # bit `slot ^ octant` of the group mask; the highest set bit is the child visited first
        bit = slots[None, :] ^ oct7[rays][:, None]
        key = np.where(hit, bit, -1)
        best = key.argmax(1)                                                         # the slot whose bit is highest
        any_hit = hit.any(1)
        entries[rays] += (hit.sum(1) > 1)
        nxt = child_base[node] + (inner & (slots[None, :] < best[:, None])).sum(1)     # child_base + popcount(imask below the slot)
        rays, node = rays[any_hit], nxt[any_hit]
    return entries, marginal


def distribution(entries, keep):
    """{entries: rays} over the rays `keep` selects, ascending"""
    vals, counts = np.unique(entries[keep], return_counts=True)
    return {int(v): int(c) for v, c in zip(vals, counts)}


# ---- the edits tests/test_gpu_deep_tree.py makes to a begun scene, and the descriptions a fresh scene is given for them ----

INNER_FROM = 16      # the shells from this one inwards form the registered object


def _replaced(sc, v, n, t):
    import copy
    out = copy.copy(sc)
    out._desc = None
    out.vertices, out.normals, out.tangents = (np.ascontiguousarray(a, f32).reshape(-1, 3, 3) for a in (v, n, t))
    return out


def scaled(sc, k=1.5):
    """every vertex scaled by k about the origin (float32 products): the shells stay self-similar and the camera just behind the origin"""
    return _replaced(sc, (sc.vertices * f32(k)).astype(f32), sc.normals, sc.tangents)


def inner_object(sc):
    """the triangle ids of the shells INNER_FROM, INNER_FROM + 1, ...: most of the chain"""
    return np.arange(INNER_FROM * sc.per, sc.tri_count, dtype=np.uint32)


def inner_pose():
    """the object turned by 3 rad about the view diagonal through the origin and scaled by 2: it stays a set of shells about that axis
    (chosen with tests/test_deep_tree_scenes_cpu.py: a fresh build of the posed arrays is as deep as the scene's own)"""
    a = np.ones(3) / np.sqrt(3.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    L = 2.0 * (np.eye(3) + np.sin(3.0) * K + (1 - np.cos(3.0)) * (K @ K))
    return np.concatenate([L, np.zeros((3, 1))], 1).astype(f32)


def posed(sc):
    """the description after er_render_transform of inner_object by inner_pose (elevenrender_amd.transform.pose, the library's arithmetic)"""
    from elevenrender_amd import transform
    ids = inner_object(sc).astype(np.int64)
    v, n, t = (a.reshape(-1, 3, 3).copy() for a in (sc.vertices, sc.normals, sc.tangents))
    pv, pn, pt = transform.pose(inner_pose(), v[ids], n[ids], t[ids])
    v[ids], n[ids], t[ids] = pv, pn, pt
    return _replaced(sc, v, n, t)


def stepped_back_camera(sc, delta=1e-5):
    """the scene's camera moved back along its view diagonal by delta: its rays still start inside the boxes of the innermost shells
    (the builders' padding is 4e-6) and leave as many entries, and the nearest visible shells shift by up to half a pixel of 160"""
    cam = abi.ErCamera.from_buffer_copy(sc.camera)
    back = VIEW @ np.array([0.0, 0.0, -float(delta)])
    cam.position = abi.ErVec3(float(sc.camera.position.x + back[0]), float(sc.camera.position.y + back[1]), float(sc.camera.position.z + back[2]))
    return cam
