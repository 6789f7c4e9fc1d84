"""Scenes for ER_FLAG_MESH_LIGHTS with MANY emitters, cut-outs and textured light, and a replay of the emitter table (a module for the
tests, not a conftest).

Every other mesh-light check of the suite runs on a Cornell box: 12 to 14 triangles, 2 or 3 emitters, every hit opaque.  Here:
  * `emitters(n_tris, share, seed)`: a soup in which a share of the triangles, chosen by a seeded permutation, is emissive -- constant
    emissions and five emission textures (EMISSION_TEXTURES: 1 x 1 ... 33 x 31 texels, 1 to 4 channels) between them.  CASES lists the
    sizes at which the table kernels of csrc/er_lights.hip take another path.
  * `lit_soup(seed)`: the scene of the path tests -- about 3 000 triangles with jittered (smooth) normals, emitters of constant and
    textured emission under tiled and negative uvs, emitters of partial and textured opacity, non-emissive cut-outs between them, and
    an emissive triangle of zero area.
  * `replay_table(sc, order)`: the table in numpy float32 in exactly the float order the header of csrc/er_lights.hip documents, and
    `float64_cdf`, the same sums in float64 with the bound they must meet.

All scenes derive from scenes.soup geometry (no coplanar shared edges: the soup tests hold the GPU to the oracle with zero exceptions).
All randomness comes from scenes.Rand."""
import numpy as np

import uv_scenes
from elevenrender_amd import abi, scenes

f32 = np.float32

# (n_tris, share): what the case reaches in csrc/er_lights.hip
CASES = [
    (1, "all"),        # a single emitter
    (65, "all"),       # a second wave
    (1024, "all"),     # exactly one full workgroup and chunk 1
    (1025, "all"),     # a second workgroup and chunk 2
    (2049, "all"),     # chunk 3, trailing threads with empty ranges
    (3000, 1 / 2),     # mixed waves
    (3000, 1 / 97),    # whole waves, and most likely whole workgroups, without an emitter
    (3000, "one"),     # a single entry in a large table
    (3000, "none"),    # empty table
]
CASE_IDS = [f"{n}-{s if isinstance(s, str) else round(1 / s)}" for n, s in CASES]

# (width, height, channels, filter) of the emission textures of `emitters`: one texel; most of the mean kernel's 256 threads idle; 255
# texels; 256; several strides
EMISSION_TEXTURES = [(1, 1, 3, 0), (4, 4, 1, 0), (17, 15, 2, 1), (16, 16, 4, 0), (33, 31, 3, 1)]
CONSTANT_EMISSIONS = [(0.9, 0.7, 0.5), (0.05, 1.3, 0.2), (2.0, 0.0, 0.0)]


def emitter_count(n_tris, share):
    return {"all": n_tris, "one": 1, "none": 0}[share] if isinstance(share, str) else int(n_tris * share)


def emitters(n_tris, share, seed=3, x_res=16, y_res=12):
    """A soup of n_tris triangles of which emitter_count(n_tris, share), chosen by a seeded permutation, are emissive: the i-th of them
    carries material 1 + i % 8 (three constant emissions, then the five EMISSION_TEXTURES); every other triangle material 0."""
    sc = scenes.soup(n_tris, x_res, y_res, seed=seed, hdri_size=(32, 16))
    r = scenes.Rand(seed, 21)
    perm = np.argsort(r.u01(n_tris), kind="stable")
    M = abi.default_material
    mats = [M()] + [M(emission=e) for e in CONSTANT_EMISSIONS]
    textures = []
    for (w, h, ch, flt) in EMISSION_TEXTURES:
        textures.append((abi._f32(r.uniform(0.0, 1.5, h, w, ch)), w, h, ch, flt))
        mats.append(M(emission_tex=len(textures) - 1))
    mid = np.zeros(n_tris, np.int32)
    k = emitter_count(n_tris, share)
    mid[perm[:k]] = 1 + np.arange(k) % (len(mats) - 1)
    sc.materials, sc.textures, sc.material_id = mats, textures, mid
    sc._desc = None
    return sc


# ---- the scene of the path tests -------------------------------------------------------------------------------------------------
# materials of lit_soup; triangle t carries LIT_PATTERN[t % 16]
PLAIN, CONST, TEX_RGB, TEX_ONE, HALF, OP_TEX, CUTOUT, BIG = range(8)
LIT_PATTERN = [CUTOUT, PLAIN, CONST, CUTOUT, TEX_RGB, OP_TEX, CUTOUT, TEX_ONE, OP_TEX, CUTOUT, HALF, CUTOUT, OP_TEX, TEX_RGB, CUTOUT, TEX_ONE]
LIT_EMISSIVE = (CONST, TEX_RGB, TEX_ONE, HALF, OP_TEX, BIG)
LIT_TEX_RGB, LIT_TEX_ONE, LIT_TEX_OPACITY = 0, 1, 2      # texture ids
LIT_ZERO_AREA = 34                                       # this triangle (a CONST one) is degenerate: emissive, no table entry
LIT_BIG = 1                                              # this triangle is the BIG one
LIT_MAX_BOUNCES = 8


def lit_soup(seed=19, x_res=48, y_res=36, n_tris=3000):
    """3 000 soup triangles, jittered normals (hit positions are lifted, as scenes.torture(smooth=True) has them), per-triangle uvs that
    tile and go negative (uv_scenes.varied_uvs), a dim HDRI, and the materials above:
      PLAIN             opaque, no emission
      CONST             constant emission
      TEX_RGB           emission from a bilinear 3-channel 8 x 8 texture
      TEX_ONE           emission from an unfiltered 1-channel 7 x 5 texture
      HALF              constant emission, constant opacity 0.5
      OP_TEX            constant emission, opacity from a bilinear 2-channel 5 x 3 texture with values in about [-1.5, 2.5]
      CUTOUT            no emission, opacity 0.3: 6 of 16 triangles, so that bounces and emitters have cut-outs between them
      BIG               one large dim emitter behind the soup, with its face normal: it holds about a quarter of the table's weight and
                        much of the view, so that an emitter sample often picks the very triangle being shaded (the skip of rule 6)
    Emission stays below 1 and the HDRI below 0.1 so that no sample reaches the clamp at 10 (tests/test_mesh_light_scenes_cpu.py
    asserts it on the oracle's unclamped values)."""
    sc = scenes.soup(n_tris, x_res, y_res, seed=seed, hdri_size=(32, 16))
    r = scenes.Rand(seed, 23)
    sc.hdri = (abi._f32(0.02 + 0.06 * r.u01(16, 32, 3)), 32, 16, 3, 0)
    sc.vertices[LIT_ZERO_AREA, 2] = sc.vertices[LIT_ZERO_AREA, 1]
    sc.vertices[LIT_BIG] = np.array([[-2.5, -2.0, 4.3], [0.2, 2.6, 4.25], [2.6, -2.1, 4.35]], f32)
    sc.normals, sc.tangents = scenes.face_frame(sc.vertices)
    jitter = r.uniform(-0.35, 0.35, n_tris, 3, 3)
    jitter[LIT_BIG] = 0
    sc.normals = scenes._normalize(sc.normals + jitter)
    sc.uvs, _ = uv_scenes.varied_uvs(n_tris, seed + 1)
    # (opacity: the first channel cycles through seven levels, three of them below 0 and three above 1, so that bilinear samples fall on
    # both sides of [0, 1] about equally often; the second channel is never read)
    op = np.stack([np.resize(np.array([-1.3, 2.3, -0.7, 0.5, 1.7, -1.0, 1.4], f32), 15).reshape(3, 5) + r.uniform(-0.2, 0.2, 3, 5),
                   r.uniform(0.0, 1.0, 3, 5)], -1)
    sc.textures = [(abi._f32(r.uniform(0.1, 0.9, 8, 8, 3)), 8, 8, 3, 1),
                   (abi._f32(r.uniform(0.1, 0.9, 5, 7, 1)), 7, 5, 1, 0),
                   (abi._f32(op), 5, 3, 2, 1)]
    M = abi.default_material
    mats = [None] * 8
    mats[PLAIN] = M()
    mats[CONST] = M(emission=(0.8, 0.6, 0.4))
    mats[TEX_RGB] = M(emission_tex=LIT_TEX_RGB)
    mats[TEX_ONE] = M(emission_tex=LIT_TEX_ONE)
    mats[HALF] = M(emission=(0.3, 0.7, 0.9), opacity=0.5)
    mats[OP_TEX] = M(emission=(0.9, 0.9, 0.5), opacity_tex=LIT_TEX_OPACITY)
    mats[CUTOUT] = M(albedo=(0.7, 0.7, 0.6), opacity=0.3)
    mats[BIG] = M(albedo=(0.8, 0.3, 0.2), roughness=0.6, emission=(0.15, 0.12, 0.2))
    sc.materials = mats
    sc.material_id = np.array(LIT_PATTERN, np.int32)[np.arange(n_tris) % 16]
    sc.material_id[LIT_BIG] = BIG
    assert sc.material_id[LIT_ZERO_AREA] == CONST
    sc._desc = None
    return sc


def traced_pixels(sc, n=200, seed=5):
    """the pixels the per-bounce trace tests look at (GPU and CPU tests must agree on them)"""
    return np.random.default_rng(seed).choice(sc.x_res * sc.y_res, n, replace=False)


# ---- the emitter table, replayed -------------------------------------------------------------------------------------------------
def lum32(r, g, b):
    """lum(r, g, b) = (0.2126f * r + 0.7152f * g) + 0.0722f * b: float32 products and sums, none fused"""
    r, g, b = f32(r), f32(g), f32(b)
    return (f32(0.2126) * r + f32(0.7152) * g) + f32(0.0722) * b


def texture_mean32(tex):
    """er_lights_tex_mean_kernel: thread t of 256 sums the luminances of texels t, t + 256, ... ascending from 0.0f; the 256 partial sums
    are added pairwise, s[t] += s[t + h] for h = 128 ... 1; mean = s[0] / (float)(width * height)"""
    data, w, h, ch, _ = tex
    d = np.asarray(data, f32).reshape(h * w, ch)
    zero = np.zeros(h * w, f32)
    if ch == 1:
        rgb = (d[:, 0], d[:, 0], d[:, 0])
    elif ch == 2:
        rgb = (d[:, 0], d[:, 1], zero)
    else:
        rgb = (d[:, 0], d[:, 1], d[:, 2])
    l = lum32(*rgb)
    rows = -(-len(l) // 256)
    padded = np.zeros(rows * 256, f32)          # (a thread past the end adds nothing; x + 0.0f is x)
    padded[:len(l)] = l
    s = np.zeros(256, f32)
    for row in padded.reshape(rows, 256):
        s = s + row
    hh = 128
    while hh >= 1:
        s[:hh] = s[:hh] + s[hh:2 * hh]
        hh >>= 1
    return f32(s[0] / f32(w * h))


def weights32(sc):
    """per input triangle the weight A * lum of er_lights_weight_kernel (0: no entry), float32 in the kernel's order:
    c = cross(v1 - v0, v2 - v0) with the sign convention of er_device.h, A = 0.5f * sqrtf(c.x * c.x + c.y * c.y + c.z * c.z)"""
    v = np.asarray(sc.vertices, f32)
    a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = -(a[:, 0] * b[:, 2] - a[:, 2] * b[:, 0])
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    area = f32(0.5) * np.sqrt((cx * cx + cy * cy) + cz * cz)
    lum = np.zeros(len(sc.materials), f32)
    emitter = np.zeros(len(sc.materials), bool)
    for i, m in enumerate(sc.materials):
        if m.emission_tex >= 0:
            lum[i], emitter[i] = texture_mean32(sc.textures[m.emission_tex]), True
        else:
            lum[i] = lum32(m.emission.x, m.emission.y, m.emission.z)
            emitter[i] = lum[i] > 0
    mid = np.asarray(sc.material_id)
    w = (area * lum[mid]).astype(f32)
    w[~emitter[mid] | ~(area > 0) | ~(w > 0)] = 0
    return w


def cdf32(w):
    """er_lights_cdf_kernel over the compacted weights w: 1 024 threads, chunk = ceil(n / 1024) entries each, thread t owns
    [t * chunk, (t + 1) * chunk) clamped to n; s_t = its weights summed ascending from 0.0f; off_0 = 0, off_{t+1} = off_t + s_t serially;
    W = off_1024; then r = off_t, r = r + w_i ascending, cdf_i = r / W.  Returns (cdf, W)."""
    w = np.asarray(w, f32)
    n = len(w)
    chunk = -(-n // 1024)
    padded = np.zeros(1024 * chunk, f32)         # (an index past n adds nothing)
    padded[:n] = w
    cols = padded.reshape(1024, chunk)
    s = np.zeros(1024, f32)
    for c in range(chunk):
        s = s + cols[:, c]
    off = np.zeros(1025, f32)
    for t in range(1024):
        off[t + 1] = off[t] + s[t]
    W = off[1024]
    run = off[:1024].copy()
    out = np.zeros((1024, chunk), f32)
    for c in range(chunk):
        run = run + cols[:, c]
        out[:, c] = run / W
    return out.reshape(-1)[:n].copy(), f32(W)


def replay_table(sc, order):
    """The emitter table over the input triangles `order` (the device's own order), float32, in the order of operations of
    csrc/er_lights.hip: dict of weight, cdf, prob float32[n] and total (W); `emitters`: numpy's own set, ascending triangle index."""
    w = weights32(sc)
    order = np.asarray(order, np.int64)
    wo = w[order]
    if len(order) == 0:
        return dict(weight=wo, cdf=wo.copy(), prob=wo.copy(), total=f32(0), emitters=np.nonzero(w > 0)[0])
    cdf, W = cdf32(wo)
    return dict(weight=wo, cdf=cdf, prob=(wo / W).astype(f32), total=W, emitters=np.nonzero(w > 0)[0])


U = 2.0 ** -24


def float64_cdf(weight, total):
    """The same CDF from the same float32 weights with every sum in float64, over the float32 W the table was divided by, and the
    bound a float32 entry must meet.

    Derivation.  Entry i is fl(r_i / W), r_i the float32 running sum the kernel formed: off_t (thread 0's serial chain: at most 1 024
    additions) continued by at most `chunk` additions in thread t.  Every weight is positive, so by the standard result for recursive
    summation (each addition rounds once, relative error at most u = 2^-24) a weight that went through m additions carries a factor
    (1 + d)^m, and r_i = (1 + theta) * sum of its weights with |theta| <= gamma_k = k u / (1 - k u), k = chunk + 1024 the most additions
    any term went through.  (The per-thread sums s_t are formed first and then chained; a term still passes at most chunk + 1024
    additions.)  The division by the given float32 W rounds once more.  So against sum64 / W the relative error is at most gamma_(k+1),
    and the bound asserted is (k + 2) u / (1 - (k + 2) u) >= gamma_(k+1).  W itself, against the float64 sum of all weights, meets
    gamma_k for the same reason; that is asserted beside it.  Returns (cdf64, bound, total64)."""
    w = np.asarray(weight, f32).astype(np.float64)
    n = len(w)
    k = -(-n // 1024) + 1024
    bound = (k + 2) * U / (1 - (k + 2) * U)
    return np.cumsum(w) / float(total), bound, w.sum()


def numpy_emitters64(sc):
    """the set of emitters by the rule alone (er_shade.h rule 1), float64: triangles of positive area whose material has an emission
    texture or a constant emission of positive luminance"""
    v = np.asarray(sc.vertices, f32).astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    ok = np.array([m.emission_tex >= 0 or 0.2126 * m.emission.x + 0.7152 * m.emission.y + 0.0722 * m.emission.z > 0 for m in sc.materials])
    return np.nonzero(ok[np.asarray(sc.material_id)] & (area > 0))[0]


# ---- the oracle over the traced pixels -------------------------------------------------------------------------------------------
def host_order(sc):
    """the emitters in ascending slot order of the HOST builder's structure (abi.debug_bvh_dump, no device needed): the table order of
    a render begun with ER_FLAG_HOST_BUILD"""
    slot_to_tri = abi.debug_bvh_dump(sc.vertices, sc.normals)["slot_to_tri"].astype(np.int64)
    w = weights32(sc)
    return slot_to_tri[w[slot_to_tri] > 0].astype(np.int32)


TRACE_CONFIGS = [(0, 8), (abi.FLAG_MIS, 8), (0, 2), (abi.FLAG_MIS, 2)]      # (extra flags, max_bounces); 2: the last-bounce rule decides on every path


def oracle_traces(oracle_mod, sc, order, flags, max_bounces, pixels, history=2, reps=2):
    """The oracle alone: `history` rendered samples, then `reps` consecutive traced samples of each of `pixels`.  Returns the Oracle
    (the caller closes it) and a list of (pixel, rep, [OracleTraceRec ...])."""
    orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, max_bounces=max_bounces, threads=1, flags=flags | abi.FLAG_MESH_LIGHTS)
    orc.set_emitters(order)
    orc.render(history)
    out = []
    for idx in pixels:
        for rep in range(reps):
            out.append((int(idx), rep, orc.trace_pixel(int(idx), max_recs=32)))
    return orc, out


CLASSES = ("visible", "occluded", "skipped_self", "skipped_last", "hit_direct", "hit_through", "le_tex_rgb", "le_tex_one",
           "opacity_below_0", "opacity_above_1")


def class_counts(traces):
    """what the traced samples exercise, counted from the oracle's records (oracle/er_oracle.h OracleTraceRec's mesh fields)"""
    n = dict.fromkeys(CLASSES, 0)
    for _, _, recs in traces:
        for r in recs:
            n["visible"] += r.mesh_sample == 0 and r.light_occ == 0
            n["occluded"] += r.mesh_sample == 0 and r.light_occ == 1
            n["skipped_self"] += r.mesh_sample == 1
            n["skipped_last"] += r.mesh_sample == 2
            n["hit_direct"] += r.mesh_hit == 1 and f32(r.mesh_d) == f32(0.001)
            n["hit_through"] += r.mesh_hit == 2
            n["le_tex_rgb"] += r.mesh_sample == 0 and r.mesh_le_tex == LIT_TEX_RGB
            n["le_tex_one"] += r.mesh_sample == 0 and r.mesh_le_tex == LIT_TEX_ONE
            n["opacity_below_0"] += r.mesh_sample == 0 and r.mesh_opacity < 0
            n["opacity_above_1"] += r.mesh_sample == 0 and r.mesh_opacity > 1
    return {k: int(v) for k, v in n.items()}


def max_unclamped(traces):
    """the largest component of any traced sample's radiance BEFORE the clamp at 10 (the last record's `light`)"""
    return max((max(recs[-1].light) for _, _, recs in traces if recs), default=0.0)
