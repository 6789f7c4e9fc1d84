"""An independent checker of the built acceleration structure (a module for the tests, not a conftest).

Everything the three schedules trace goes through the structure of elevenrender_amd/csrc/er_bvh.h: the binary ErNode tree (the exact
routine's fallback), the 80-byte ErNode8 wide tree (production), the 48-byte intersection records and the attribute records.  `check`
takes the scene's own arrays and a dump of that structure -- RenderingManager.debug_read_accel() (device memory, whichever builder
made it) or abi.debug_bvh_dump() completed by `host_records` (the host builder, no device) -- and returns NAMED violation counts
with the first few offenders of each.  Plain numpy; no library code is called, and nothing here is derived from what the builders
produce: the padded boxes and the lift bounds are recomputed in float64 from the scene's vertices and normals.

What is required, by name (DESIGN.md section 2 says why):

wide tree
  w_parent          every node 1 .. N-1 is the child of exactly one node (node 0 of none)
  w_child_order     a node's inner children are child_base + k, k < popcount(imask), in ascending slot order: all of them exist (< N)
  w_breadth_first   child_base > the node's own index
  w_inner_tri_bits  slot s inner  =>  bits 2s and 2s+1 of tri_present clear
  w_tri_bits_order  bit 2s+1 set  =>  bit 2s set
  w_reserved        reserved == 0
  w_tri_partition   the ranges [tri_base, tri_base + popcount(tri_present)) of all nodes partition [0, n): no gap, no overlap
  w_depth           measured depth == reported max_depth8 (== accel_info's, if given) and <= ER_STACK8
  w_box             for every occupied slot the decoded box float32(p + float32(q * 2^(e-127))) contains the padded box of every
                    triangle beneath that slot (a leaf slot: its 1-2 triangles; an inner slot: the child's whole subtree)
binary tree
  b_reach           every node is reachable from node 0, exactly once
  b_leaf_partition  the leaf ranges partition [0, n)
  b_leaf_box        each leaf's box contains the padded boxes of its slots
  b_child_box       each child box lies inside its parent's
  b_depth           measured depth == reported max_depth and <= ER_BVH_MAX_DEPTH
  b_leaf_size       leaves hold <= ER_BVH_LEAF_MAX triangles
records
  r_perm            tri_id over slots 0 .. n-1 is a permutation of 0 .. n-1
  r_vertices        v0, v1, v2 equal the scene's vertex bits of tri_id
  r_sign            sign equals tangent_sign[tri_id] bit for bit
  r_attr            n, t, uv, material equal the scene arrays of tri_id bit for bit, pad is zero
  r_sentinel        record n, the one past the end, is 48 zero bytes (counted: its non-zero bytes)
  r_lift            tl <= lift <= 1.02 tl + 1e-29, tl the float64 bound on |shadingPosition - geomPosition| of the triangle
  r_lift_bound      lift_bound (and max_lift) >= every tl and <= 1.02 x the largest
  r_bounds          the scene bounds contain every padded box

The padded box of a triangle: its vertex min / max per axis in float64, widened by 0.99 x max(m * 4e-7 + 1e-37, vmax * 1e-6), m the
larger magnitude of the two bounds on that axis and vmax the largest |coordinate| of the scene (er_build_bvh).  The factor 0.99 only
makes the requirement independent of whether a compiler fused m * 4e-7f + 1e-37f; it is no tolerance on containment.
"""
import numpy as np

ER_BVH_MAX_DEPTH = 64      # elevenrender_amd/csrc/er_bvh.h
ER_STACK8 = 32
ER_BVH_LEAF_MAX = 2
NO_CHILD = 0x7FFFFFFF

NAMES = ("w_parent", "w_child_order", "w_breadth_first", "w_inner_tri_bits", "w_tri_bits_order", "w_reserved", "w_tri_partition", "w_depth", "w_box",
         "b_reach", "b_leaf_partition", "b_leaf_box", "b_child_box", "b_depth", "b_leaf_size",
         "r_perm", "r_vertices", "r_sign", "r_attr", "r_sentinel", "r_lift", "r_lift_bound", "r_bounds")
KEEP = 5                   # offenders kept per name


class Report:
    def __init__(self):
        self.counts = {k: 0 for k in NAMES}
        self.first = {k: [] for k in NAMES}
        self.depth8 = self.depth2 = 0
        self.slot_req_lo = self.slot_req_hi = None      # [N, 8, 3] float64: what each wide slot's box must contain (+-inf: empty slot)

    def add(self, name, count, offenders=()):
        self.counts[name] += int(count)
        room = KEEP - len(self.first[name])
        if room > 0:
            self.first[name].extend(list(offenders)[:room])

    @property
    def ok(self):
        return not any(self.counts.values())

    def failed(self):
        return {k: v for k, v in self.counts.items() if v}

    def message(self):
        if self.ok:
            return "structure checks clean"
        return "; ".join(f"{k}: {v} (first: {self.first[k]})" for k, v in self.failed().items())


def padded_boxes(vertices):
    """float64 [n, 3] lo, hi: the box the builders promise to cover for each triangle (module docstring)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3, 3).astype(np.float64)
    if len(v) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3))
    lo, hi = v.min(1), v.max(1)
    m = np.maximum(np.abs(lo), np.abs(hi))
    vmax = np.abs(v).max()
    pad = 0.99 * np.maximum(m * 4e-7 + 1e-37, vmax * 1e-6)
    return lo - pad, hi + pad


def lift_bounds(vertices, normals):
    """float64 [n]: max over corners j and the other corners k of |dot(v_k - v_j, n_j)| * |n_j| (reference src/Tri.h:106-112: the hit point is
    a convex combination of the vertices and each corner's plane moves it by at most that much)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3, 3).astype(np.float64)
    nn = np.asarray(normals, np.float32).reshape(-1, 3, 3).astype(np.float64)
    tl = np.zeros(len(v))
    for j in range(3):
        nl = np.sqrt((nn[:, j] ** 2).sum(-1))
        for k in range(3):
            if k != j:
                tl = np.maximum(tl, np.abs(((v[:, k] - v[:, j]) * nn[:, j]).sum(-1)) * nl)
    return tl


def host_records(sc, dump):
    """The records er_render_begin uploads after a HOST build, assembled from slot_to_tri and tri_lift of abi.debug_bvh_dump and the scene
    arrays (no device): the dump gains 'isect' and 'attr' in the layout of debug_read_accel, so that the same `check` runs in the CPU
    suite.  (There the record checks test this assembly and the checker's ability to fail, not the library: the library's records are
    read back from the device in tests/test_gpu_accel_structure.py.)"""
    n = int(dump["tri_count"])
    s2t = np.asarray(dump["slot_to_tri"], np.int64)
    v = np.asarray(sc.vertices, np.float32).reshape(-1, 3, 3)
    isect = np.zeros(n + 1, np.dtype([("v0", "<f4", 3), ("tri_id", "<i4"), ("v1", "<f4", 3), ("lift", "<f4"), ("v2", "<f4", 3), ("sign", "<f4")]))
    attr = np.zeros(n, np.dtype([("n", "<f4", (3, 3)), ("t", "<f4", (3, 3)), ("uv", "<f4", (3, 2)), ("material", "<i4"), ("pad", "<u4", 3)]))
    if n:
        isect["v0"][:n], isect["v1"][:n], isect["v2"][:n] = v[s2t, 0], v[s2t, 1], v[s2t, 2]
        isect["tri_id"][:n] = s2t
        isect["lift"][:n] = np.asarray(dump["tri_lift"], np.float32)[s2t]
        isect["sign"][:n] = np.asarray(sc.tangent_sign, np.float32).reshape(-1)[s2t]
        attr["n"] = np.asarray(sc.normals, np.float32).reshape(-1, 3, 3)[s2t]
        attr["t"] = np.asarray(sc.tangents, np.float32).reshape(-1, 3, 3)[s2t]
        attr["uv"] = np.asarray(sc.uvs, np.float32).reshape(-1, 3, 2)[s2t]
        attr["material"] = np.asarray(sc.material_id, np.int32).reshape(-1)[s2t]
    out = dict(dump)
    out["isect"], out["attr"] = isect, attr
    return out


def decode_wide_boxes(nodes8):
    """float32 [N, 3, 8] lo, hi: float32(p + float32(q * 2^(e - 127))) -- the product is exact, one rounding per plane."""
    scale = np.ldexp(np.float32(1.0), nodes8["e"].astype(np.int32) - 127).astype(np.float32)          # [N, 3]
    p = nodes8["p"].astype(np.float32)
    lo = (p[:, :, None] + (nodes8["qlo"].astype(np.float32) * scale[:, :, None]).astype(np.float32)).astype(np.float32)
    hi = (p[:, :, None] + (nodes8["qhi"].astype(np.float32) * scale[:, :, None]).astype(np.float32)).astype(np.float32)
    return lo, hi


def _popcount32(x):
    x = np.asarray(x, np.uint64)
    return sum(((x >> np.uint64(b)) & np.uint64(1)) for b in range(32)).astype(np.int64)


def _partition(starts, counts, n):
    """How many of the slots 0 .. n-1 are not covered exactly once by the ranges [start, start + count), plus the ranges that leave [0, n)."""
    starts, counts = np.asarray(starts, np.int64), np.asarray(counts, np.int64)
    keep = counts > 0
    starts, counts = starts[keep], counts[keep]
    outside = (starts < 0) | (starts + counts > n)
    a, b = np.clip(starts, 0, n), np.clip(starts + counts, 0, n)
    d = np.zeros(n + 1, np.int64)
    np.add.at(d, a, 1)
    np.add.at(d, b, -1)
    cover = np.cumsum(d)[:n]
    wrong = np.nonzero(cover != 1)[0]
    return int(outside.sum()) + len(wrong), [("slot", int(s), "covered", int(cover[s])) for s in wrong[:KEEP]]


def _wide(rep, nodes8, n, slot_lo, slot_hi, reported_depth8, accel_depth):
    N = len(nodes8)
    if N == 0:
        rep.add("w_tri_partition", n, [("no wide nodes for", n, "triangles")] if n else [])
        rep.add("w_depth", int(reported_depth8 != 0))
        return
    s = np.arange(8)
    idx = np.arange(N, dtype=np.int64)
    imask = nodes8["imask"].astype(np.int64)
    tp = nodes8["tri_present"].astype(np.int64)
    inner = ((imask[:, None] >> s) & 1).astype(bool)                       # [N, 8]
    b0 = ((tp[:, None] >> (2 * s)) & 1).astype(bool)
    b1 = ((tp[:, None] >> (2 * s + 1)) & 1).astype(bool)
    cnt = b0.astype(np.int64) + b1.astype(np.int64)                         # triangles of a leaf slot
    rank = np.cumsum(inner, 1) - inner                                      # k of an inner slot
    child = nodes8["child_base"].astype(np.int64)[:, None] + rank           # [N, 8], meaningful where inner
    exists = inner & (child < N)
    rep.add("w_child_order", (inner & ~exists).sum(), [("node", int(i), "slot", int(k), "child", int(child[i, k])) for i, k in zip(*np.nonzero(inner & ~exists))][:KEEP])
    parents = np.bincount(child[exists], minlength=N)
    bad = np.nonzero(np.where(idx == 0, parents != 0, parents != 1))[0]
    rep.add("w_parent", len(bad), [("node", int(i), "parents", int(parents[i])) for i in bad[:KEEP]])
    has_inner = inner.any(1)
    bad = np.nonzero(has_inner & (nodes8["child_base"].astype(np.int64) <= idx))[0]
    rep.add("w_breadth_first", len(bad), [("node", int(i), "child_base", int(nodes8["child_base"][i])) for i in bad[:KEEP]])
    bad = inner & (b0 | b1)
    rep.add("w_inner_tri_bits", bad.sum(), [("node", int(i), "slot", int(k)) for i, k in zip(*np.nonzero(bad))][:KEEP])
    bad = b1 & ~b0
    rep.add("w_tri_bits_order", bad.sum(), [("node", int(i), "slot", int(k)) for i, k in zip(*np.nonzero(bad))][:KEEP])
    bad = np.nonzero(nodes8["reserved"] != 0)[0]
    rep.add("w_reserved", len(bad), [("node", int(i)) for i in bad[:KEEP]])
    tri_base = nodes8["tri_base"].astype(np.int64)
    c, off = _partition(tri_base, _popcount32(nodes8["tri_present"]), n)
    rep.add("w_tri_partition", c, off)

    # levels, following only edges that exist and point forward (no cycles whatever the bytes say)
    follow = exists & (child > idx[:, None])
    levels, seen, frontier = [], np.zeros(N, bool), np.array([0], np.int64)
    while len(frontier):
        frontier = np.unique(frontier[~seen[frontier]])
        if not len(frontier):
            break
        seen[frontier] = True
        levels.append(frontier)
        frontier = child[frontier][follow[frontier]]
    rep.depth8 = len(levels)
    wrong = [("measured", rep.depth8, "reported", int(reported_depth8))] if rep.depth8 != reported_depth8 else []
    if accel_depth is not None and rep.depth8 != accel_depth:
        wrong.append(("measured", rep.depth8, "accel_info", int(accel_depth)))
    if rep.depth8 > ER_STACK8:
        wrong.append(("measured", rep.depth8, "ER_STACK8", ER_STACK8))
    rep.add("w_depth", len(wrong), wrong)

    # what every slot must contain: leaf slots from their triangles, inner slots from the child's node box, bottom-up by level
    below = np.cumsum(cnt, 1) - cnt                                         # triangles of the node in lower slots: compact, in bit order
    req_lo = np.full((N, 8, 3), np.inf)
    req_hi = np.full((N, 8, 3), -np.inf)
    for j in range(ER_BVH_LEAF_MAX):
        pos = tri_base[:, None] + below + j
        use = ~inner & (cnt > j) & (pos >= 0) & (pos < n)
        req_lo[use] = np.minimum(req_lo[use], slot_lo[pos[use]])
        req_hi[use] = np.maximum(req_hi[use], slot_hi[pos[use]])
    node_lo = np.full((N, 3), np.inf)
    node_hi = np.full((N, 3), -np.inf)
    for lv in reversed(levels):
        f = follow[lv]
        ii, kk = np.nonzero(f)
        req_lo[lv[ii], kk] = node_lo[child[lv[ii], kk]]
        req_hi[lv[ii], kk] = node_hi[child[lv[ii], kk]]
        node_lo[lv] = req_lo[lv].min(1)
        node_hi[lv] = req_hi[lv].max(1)
    rep.slot_req_lo, rep.slot_req_hi = req_lo, req_hi
    dlo, dhi = decode_wide_boxes(nodes8)                                    # [N, 3, 8]
    dlo, dhi = dlo.astype(np.float64).transpose(0, 2, 1), dhi.astype(np.float64).transpose(0, 2, 1)
    cut_lo, cut_hi = dlo > req_lo, dhi < req_hi                             # (+-inf requirements of empty slots never fail)
    off = [("node", int(i), "slot", int(k), "axis", int(a), "decoded lo", float(dlo[i, k, a]), "must reach", float(req_lo[i, k, a])) for i, k, a in zip(*np.nonzero(cut_lo))][:KEEP]
    off += [("node", int(i), "slot", int(k), "axis", int(a), "decoded hi", float(dhi[i, k, a]), "must reach", float(req_hi[i, k, a])) for i, k, a in zip(*np.nonzero(cut_hi))][:KEEP]
    rep.add("w_box", cut_lo.sum() + cut_hi.sum(), off)


def _binary(rep, nodes, n, slot_lo, slot_hi, reported_depth):
    M = len(nodes)
    if M == 0:
        rep.add("b_leaf_partition", n, [("no nodes for", n, "triangles")] if n else [])
        rep.add("b_depth", int(reported_depth != 0))
        return
    refs = np.stack([nodes["c0"], nodes["c1"]], 1).astype(np.int64)         # [M, 2]
    blo = np.stack([nodes["lo0"], nodes["lo1"]], 1).astype(np.float64)      # [M, 2, 3]
    bhi = np.stack([nodes["hi0"], nodes["hi1"]], 1).astype(np.float64)
    is_inner = (refs >= 0) & (refs != NO_CHILD)
    is_leaf = refs < 0
    visits = np.zeros(M, np.int64)
    visits[0] = 1
    frontier, depth = np.array([0], np.int64), 0
    leaf_first, leaf_count = [], []
    while len(frontier) and depth <= ER_BVH_MAX_DEPTH + 1:
        depth += 1
        r, inn, lf = refs[frontier], is_inner[frontier], is_leaf[frontier]
        # child boxes inside the parent's: the box a node was given is its parent's box for it
        pi, pk = np.nonzero(inn)
        kids = r[pi, pk]
        ok = kids < M
        rep.add("b_reach", (~ok).sum(), [("node", int(frontier[i]), "child index", int(c)) for i, c in zip(pi[~ok], kids[~ok])][:KEEP])
        pi, pk, kids = pi[ok], pk[ok], kids[ok]
        plo, phi = blo[frontier[pi], pk], bhi[frontier[pi], pk]              # [K, 3]
        used = (refs[kids] != NO_CHILD)                                      # [K, 2]
        out = (((blo[kids] < plo[:, None, :]) | (bhi[kids] > phi[:, None, :])).any(-1)) & used
        rep.add("b_child_box", out.sum(), [("node", int(kids[i]), "child", int(k), "parent", int(frontier[pi[i]])) for i, k in zip(*np.nonzero(out))][:KEEP])
        # leaves of this level
        li, lk = np.nonzero(lf)
        code = ~r[li, lk]
        first, count = code >> 3, (code & 7) + 1
        leaf_first.append(first)
        leaf_count.append(count)
        big = count > ER_BVH_LEAF_MAX
        rep.add("b_leaf_size", big.sum(), [("node", int(frontier[i]), "leaf of", int(c)) for i, c in zip(li[big], count[big])][:KEEP])
        lbl, lbh = blo[frontier[li], lk], bhi[frontier[li], lk]
        for j in range(8):
            pos = first + j
            use = (count > j) & (pos >= 0) & (pos < n)
            cut = np.zeros(len(pos), bool)
            cut[use] = ((slot_lo[pos[use]] < lbl[use]) | (slot_hi[pos[use]] > lbh[use])).any(-1)
            rep.add("b_leaf_box", cut.sum(), [("node", int(frontier[li[i]]), "child", int(lk[i]), "slot", int(pos[i])) for i in np.nonzero(cut)[0]][:KEEP])
        np.add.at(visits, kids, 1)
        frontier = np.unique(kids[visits[kids] == 1])
    rep.depth2 = depth
    bad = np.nonzero(visits != 1)[0]
    rep.add("b_reach", len(bad), [("node", int(i), "reached", int(visits[i])) for i in bad[:KEEP]])
    c, off = _partition(np.concatenate(leaf_first), np.concatenate(leaf_count), n)
    rep.add("b_leaf_partition", c, off)
    wrong = [("measured", depth, "reported", int(reported_depth))] if depth != reported_depth else []
    if depth > ER_BVH_MAX_DEPTH:
        wrong.append(("measured", depth, "ER_BVH_MAX_DEPTH", ER_BVH_MAX_DEPTH))
    rep.add("b_depth", len(wrong), wrong)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _records(rep, sc, dump, n, plo, phi, valid, tid):
    isect, attr = dump["isect"], dump["attr"]
    ids = isect["tri_id"][:n].astype(np.int64)
    dup = n - len(np.unique(ids[valid]))
    rep.add("r_perm", dup, [("slot", int(k), "tri_id", int(ids[k])) for k in np.nonzero(~valid)[0][:KEEP]]
            + [("tri_id", int(t), "times", int(c)) for t, c in zip(*np.unique(ids[valid], return_counts=True)) if c > 1][:KEEP])
    tail = np.frombuffer(isect[n:n + 1].tobytes(), np.uint8)
    rep.add("r_sentinel", int((tail != 0).sum()) + (0 if len(isect) == n + 1 else 1), [("byte", int(b)) for b in np.nonzero(tail)[0][:KEEP]])
    if n == 0:
        rep.add("r_lift_bound", int(float(dump["lift_bound"]) != 0.0) + int(float(dump["max_lift"]) != 0.0))
        return
    v = np.asarray(sc.vertices, np.float32).reshape(-1, 3, 3)
    k = np.nonzero(valid)[0]
    got = np.stack([isect["v0"][:n], isect["v1"][:n], isect["v2"][:n]], 1)
    bad = k[(_bits(got[k]) != _bits(v[tid[k]])).any((1, 2))]
    rep.add("r_vertices", len(bad), [("slot", int(s), "tri_id", int(ids[s])) for s in bad[:KEEP]])
    bad = k[_bits(isect["sign"][:n])[k] != _bits(np.asarray(sc.tangent_sign, np.float32).reshape(-1))[tid[k]]]
    rep.add("r_sign", len(bad), [("slot", int(s)) for s in bad[:KEEP]])
    wrong = np.zeros(n, bool)
    for name, src, shape in (("n", sc.normals, (3, 3)), ("t", sc.tangents, (3, 3)), ("uv", sc.uvs, (3, 2))):
        ref = np.asarray(src, np.float32).reshape((-1,) + shape)
        wrong[k] |= (_bits(attr[name])[k] != _bits(ref)[tid[k]]).any((1, 2))
    wrong[k] |= attr["material"][k] != np.asarray(sc.material_id, np.int32).reshape(-1)[tid[k]]
    wrong |= (attr["pad"] != 0).any(-1)
    rep.add("r_attr", wrong.sum(), [("slot", int(s)) for s in np.nonzero(wrong)[0][:KEEP]])
    tl = lift_bounds(sc.vertices, sc.normals)
    lift = isect["lift"][:n].astype(np.float64)
    bad = k[~((tl[tid[k]] <= lift[k]) & (lift[k] <= 1.02 * tl[tid[k]] + 1e-29))]
    rep.add("r_lift", len(bad), [("slot", int(s), "lift", float(lift[s]), "tl", float(tl[ids[s]])) for s in bad[:KEEP]])
    for name in ("lift_bound", "max_lift"):
        b = float(dump[name])
        if not (b >= tl.max() and b <= 1.02 * tl.max()):
            rep.add("r_lift_bound", 1, [(name, b, "largest tl", float(tl.max()))])
    lo, hi = np.asarray(dump["lo"], np.float64), np.asarray(dump["hi"], np.float64)
    out = (lo > plo.min(0)) | (hi < phi.max(0))
    rep.add("r_bounds", out.sum(), [("axis", int(a), "bounds", float(lo[a]), float(hi[a]), "padded boxes", float(plo[:, a].min()), float(phi[:, a].max())) for a in np.nonzero(out)[0]])


def check(sc, dump, accel_depth=None):
    """sc: anything with vertices, normals, tangents, uvs, tangent_sign, material_id (abi.SceneData); dump: see the module docstring.
    accel_depth: accel_info()["max_depth"], where there is one.  Returns a Report."""
    rep = Report()
    n = int(dump["tri_count"])
    assert n == np.asarray(sc.vertices).size // 9
    plo, phi = padded_boxes(sc.vertices)
    ids = dump["isect"]["tri_id"][:n].astype(np.int64)
    valid = (ids >= 0) & (ids < n)
    tid = np.where(valid, ids, 0)
    # per SLOT: the padded box of the triangle the record names (a record that names none constrains nothing here; r_perm counts it)
    slot_lo = np.where(valid[:, None], plo[tid], np.inf) if n else np.zeros((0, 3))
    slot_hi = np.where(valid[:, None], phi[tid], -np.inf) if n else np.zeros((0, 3))
    _wide(rep, dump["nodes8"], n, slot_lo, slot_hi, int(dump["max_depth8"]), accel_depth)
    _binary(rep, dump["nodes"], n, slot_lo, slot_hi, int(dump["max_depth"]))
    _records(rep, sc, dump, n, plo, phi, valid, tid)
    return rep
