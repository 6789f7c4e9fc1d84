"""The numpy replay of the structure's measured cost (elevenrender_amd/csrc/er_cost.h; a module for the tests, not a conftest).

Everything is recomputed from a dump of the structure -- RenderingManager.debug_read_accel() or abi.debug_bvh_dump() completed by
accel_check.host_records -- with the number formats of the definition: every area float32 with the association written there (numpy
rounds each float32 operation once and never fuses), every sum float64, added left to right by an explicit loop (np.sum adds pairwise).

    area(lo, hi)  d = hi - lo per axis, (d.x * d.y + d.y * d.z) + d.z * d.x
    node_i        sum over inner slots, ascending, of the decoded box's area
    leaf_i        sum over leaf slots with 1 or 2 triangles, ascending, of area x count
    root          area of the union of node 0's occupied decoded boxes
    tri_k         area of the box of record k's three vertices (0 for a record that names no triangle)
    cost          (80 x (root + sum node_i) + 48 x sum leaf_i) / sum tri_k, 0 where that sum is 0

`replay` decodes the wide nodes' quantised boxes (accel_check.decode_wide_boxes), as the library does; `replay_boxes` takes float boxes
per slot instead: the cost of a topology whose boxes were refitted in numpy.
"""
import numpy as np

import accel_check

NODE_BYTES, RECORD_BYTES = 80, 48      # sizeof(ErNode8), sizeof(ErTriIsect): ErAccelInfo.node_bytes, tri_record_bytes


def area(lo, hi):
    """float32 [..., 3] -> float32 [...]"""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    d = (hi - lo).astype(np.float32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return (((dx * dy).astype(np.float32) + (dy * dz).astype(np.float32)).astype(np.float32) + (dz * dx).astype(np.float32)).astype(np.float32)


def seq_sum(values):
    """float64 sum, left to right"""
    s = 0.0
    for x in np.asarray(values, np.float64).reshape(-1).tolist():
        s += x
    return s


def slots(nodes8):
    """(inner [N, 8] bool, cnt [N, 8] int: the triangles of a leaf slot)"""
    s = np.arange(8)
    imask = nodes8["imask"].astype(np.int64)
    tp = nodes8["tri_present"].astype(np.int64)
    inner = ((imask[:, None] >> s) & 1).astype(bool)
    cnt = ((tp[:, None] >> (2 * s)) & 1) + ((tp[:, None] >> (2 * s + 1)) & 1)
    return inner, cnt


def record_terms(isect, n):
    """float32 [n]: tri_k"""
    rec = isect[:n]
    v = np.stack([rec["v0"], rec["v1"], rec["v2"]], 1).astype(np.float32)      # [n, 3, 3]
    a = area(v.min(1), v.max(1)) if n else np.zeros(0, np.float32)
    ids = rec["tri_id"].astype(np.int64)
    return np.where((ids >= 0) & (ids < n), a, np.float32(0.0)).astype(np.float32)


def replay_boxes(nodes8, lo, hi, isect, n):
    """lo, hi: float32 [N, 8, 3], the box of every slot (whatever lies in the unoccupied ones).  Returns a dict: node_terms float64
    [N, 2] (node_i, leaf_i), tri_terms float32 [n], root, node_area, leaf_area, tri_area, cost."""
    N = len(nodes8)
    inner, cnt = slots(nodes8)
    leaf = ~inner & (cnt > 0)
    node_i, leaf_i = np.zeros(N), np.zeros(N)
    with np.errstate(invalid="ignore", over="ignore"):                          # (an unoccupied slot may hold anything: its area is never added)
        a = area(lo, hi).astype(np.float64)                                     # [N, 8]
        for s in range(8):                                                      # ascending slots; a term that is not there adds nothing
            node_i = np.where(inner[:, s], node_i + a[:, s], node_i)
            leaf_i = np.where(leaf[:, s], leaf_i + a[:, s] * cnt[:, s], leaf_i)
    root = np.float32(0.0)
    if N:
        occ = inner[0] | leaf[0]
        if occ.any():
            root = area(np.asarray(lo, np.float32)[0][occ].min(0), np.asarray(hi, np.float32)[0][occ].max(0))
    tri = record_terms(isect, n)
    node_area = float(root) + seq_sum(node_i)
    leaf_area = seq_sum(leaf_i)
    tri_area = seq_sum(tri)
    cost = (NODE_BYTES * node_area + RECORD_BYTES * leaf_area) / tri_area if n and tri_area > 0 else 0.0
    return dict(node_terms=np.stack([node_i, leaf_i], 1), tri_terms=tri, root=float(root), node_area=node_area, leaf_area=leaf_area, tri_area=tri_area, cost=cost)


def replay(dump):
    """the cost of a dump as the library measures it: over the DECODED boxes of the wide nodes"""
    dlo, dhi = accel_check.decode_wide_boxes(dump["nodes8"])                    # [N, 3, 8]
    return replay_boxes(dump["nodes8"], dlo.transpose(0, 2, 1), dhi.transpose(0, 2, 1), dump["isect"], int(dump["tri_count"]))


def refitted_float_cost(sc, dump):
    """The cost of the dump's TOPOLOGY with float boxes refitted in numpy over the triangles of `sc` (the scene's arrays need not be
    those the structure was built from): per slot the union of the padded boxes beneath it, as accel_check derives them, in float32.
    The dump's records are replaced by those of `sc` in the dump's slot order."""
    d = dict(dump)
    n = int(d["tri_count"])
    v = np.asarray(sc.vertices, np.float32).reshape(-1, 3, 3)
    ids = d["isect"]["tri_id"][:n].astype(np.int64)
    rec = d["isect"].copy()
    rec["v0"][:n], rec["v1"][:n], rec["v2"][:n] = v[ids, 0], v[ids, 1], v[ids, 2]
    d["isect"] = rec
    rep = accel_check.check(sc, d)                                              # (its verdicts are not used: only what every slot must contain)
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = rep.slot_req_lo.astype(np.float32), rep.slot_req_hi.astype(np.float32)
    return replay_boxes(d["nodes8"], lo, hi, rec, n)


def sum_bound(count):
    """relative distance two orders of adding `count` non-negative doubles can lie apart: each is within (count - 1) 2^-53 of the exact sum"""
    return max(int(count), 1) * 2.0 ** -52


def assert_matches(got, ref, what=""):
    """got: a dict of the library's terms and sums (abi.debug_accel_cost_host / RenderingManager.debug_accel_cost_terms); ref: a replay.
    Terms bit-equal; sums within the bound for reordering."""
    assert got["node_terms"].shape == ref["node_terms"].shape and got["tri_terms"].shape == ref["tri_terms"].shape, what
    bad = np.nonzero((got["node_terms"].view(np.uint64) != ref["node_terms"].view(np.uint64)).any(1))[0]
    assert not len(bad), (what, "node terms differ", len(bad), [(int(i), got["node_terms"][i].tolist(), ref["node_terms"][i].tolist()) for i in bad[:3]])
    bad = np.nonzero(got["tri_terms"].view(np.uint32) != ref["tri_terms"].view(np.uint32))[0]
    assert not len(bad), (what, "record terms differ", len(bad), [(int(k), float(got["tri_terms"][k]), float(ref["tri_terms"][k])) for k in bad[:3]])
    N, n = len(ref["node_terms"]), len(ref["tri_terms"])
    for name, count in (("node_area", N + 1), ("leaf_area", N), ("tri_area", n)):
        g, r = float(got[name]), float(ref[name])
        assert abs(g - r) <= sum_bound(count) * abs(r), (what, name, g, r)
    # the quotient: three sums within their bounds, a handful of roundings on top
    g, r = float(got["cost"]), float(ref["cost"])
    assert abs(g - r) <= (2 * sum_bound(max(N + 1, n)) + 8 * 2.0 ** -52) * abs(r), (what, "cost", g, r)
