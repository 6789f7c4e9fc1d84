#!/usr/bin/env python3
"""Records tests/golden/reference_*.npz from the REFERENCE's own code (oracle/_ref/ref_libm and ref_er).

Unlike make_golden.py's files, these are not outputs of this repository's oracle: `make -C oracle ref` compiles the reference's
kernel.cpp, Disney.cpp, BVH.cpp, HDRI.cpp, Material.cpp, Texture.cpp and shader*.cpp, unmodified, against the stand-in headers
of oracle/ref_shim/, and oracle/ref_driver.cpp runs them on the inputs written here.  Every output is stored twice:
  *_libm  the reference with glibc's float functions under the sycl:: math names
  *_er    the same code with the six functions of csrc/er_math.h plugged in underneath -- what the GPU has to equal bit for bit.
The files hold numbers only (inputs next to outputs).  Seeded and deterministic: tests/test_reference_kat_cpu.py re-runs this
into a temporary directory wherever oracle/_ref/ exists and requires identical arrays.

  reference_functions.npz              function level; the inputs are the generators, seeds and edge rows of
                                       tests/test_gpu_function_kat.py (scene `rig_*`) plus rays on the 300-triangle scene of the existing golden
  reference_cornell_32x32.npz          whole path, 4 samples per pixel, the reference's compiled-in MAXBOUNCES: the five planes, the
  reference_torture_300tri_32x24.npz   sample counts and the final RNG states; the scene inputs are those of the two existing goldens
  reference_trihit_uv.npz              Tri::hit on the 300-triangle scene with per-triangle uvs and mirrored tangent signs
                                       (tests/uv_scenes.py): reference_functions.npz pins it under the unit triangle's uvs and sign +1 only

Usage: python tests/golden/make_golden_reference.py [output directory]
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from elevenrender_amd import abi, scenes  # noqa: E402
from golden_util import MAT_FIELDS, load  # noqa: E402

REF_DIR = os.path.join(ROOT, "oracle", "_ref")
MODES = ("libm", "er")
PASSES = ("beauty", "denoise", "normal", "tangent", "bitangent")
SPP = 4
TRACE_SCENE = "torture_300tri_32x24_4spp"      # the existing golden whose scene the closest-hit rays are thrown at


def available():
    return all(os.access(os.path.join(REF_DIR, "ref_" + m), os.X_OK) for m in MODES)


# ---------------------------------------------------------------- job files of oracle/ref_driver.cpp
_DT = {np.dtype(np.float32): 0, np.dtype(np.int32): 1, np.dtype(np.uint32): 2}


def write_job(path, arrays):
    with open(path, "wb") as f:
        f.write(b"ERKV" + struct.pack("<I", len(arrays)))
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<IQ", _DT[a.dtype], a.size) + a.tobytes())


def read_job(path):
    out = {}
    with open(path, "rb") as f:
        assert f.read(4) == b"ERKV"
        (count,) = struct.unpack("<I", f.read(4))
        for _ in range(count):
            (ln,) = struct.unpack("<I", f.read(4))
            name = f.read(ln).decode()
            dt, n = struct.unpack("<IQ", f.read(12))
            out[name] = np.frombuffer(f.read(4 * n), [np.float32, np.int32, np.uint32][dt]).copy()
    return out


def run_reference(arrays):
    """{mode: outputs of oracle/_ref/ref_<mode> on the job `arrays`}"""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        write_job(os.path.join(tmp, "in.erkv"), arrays)
        for m in MODES:
            subprocess.run([os.path.join(REF_DIR, "ref_" + m), os.path.join(tmp, "in.erkv"), os.path.join(tmp, m + ".erkv")],
                           check=True, stdout=subprocess.DEVNULL)    # (the reference's BVH build prints its progress)
            res[m] = read_job(os.path.join(tmp, m + ".erkv"))
    return res


# ---------------------------------------------------------------- scenes <-> arrays
def mat_to_row(m):
    row = []
    for n, _ in MAT_FIELDS:
        v = getattr(m, n)
        row += [v.x, v.y, v.z] if isinstance(v, abi.ErVec3) else [float(v)]
    return row


def cam_to_row(c):
    return [c.focal_length, c.sensor_width, c.sensor_height, c.aperture, c.focus_distance,
            c.rotation.x, c.rotation.y, c.rotation.z, float(c.bokeh), c.position.x, c.position.y, c.position.z]


def scene_arrays(sc, spp=0, max_bounces=5):
    """The arrays of make_golden.py's dump() for one scene."""
    out = {"vertices": sc.vertices, "normals": sc.normals, "tangents": sc.tangents, "uvs": sc.uvs,
           "tangent_sign": sc.tangent_sign, "material_id": sc.material_id,
           "materials": np.array([mat_to_row(m) for m in sc.materials], np.float64),
           "camera": np.array(cam_to_row(sc.camera), np.float64),
           "hdri": sc.hdri[0], "hdri_meta": np.array(sc.hdri[1:], np.int64),
           "res": np.array([sc.x_res, sc.y_res, spp, max_bounces], np.int64)}
    for i, (d, w, h, ch, flt) in enumerate(sc.textures):
        out[f"tex{i}"] = d
        out[f"tex{i}_meta"] = np.array([w, h, ch, flt], np.int64)
    return out


def job_scene(sc, spp=0):
    """The same scene in the driver's types (32 bit throughout)."""
    out = {}
    for k, v in scene_arrays(sc, spp).items():
        v = np.asarray(v)
        if k == "res":
            v = v[:3]
        out[k] = v.astype(np.int32) if (k.endswith("_meta") or k in ("res", "material_id")) else np.ascontiguousarray(v, np.float32).reshape(-1)
    return out


# ---------------------------------------------------------------- function level
def ibits(v):
    return np.asarray(v, np.int32).view(np.float32)


def rig_scene():
    """The scene of tests/test_gpu_function_kat.py's rig."""
    sc = scenes.torture(600, 48, 36, seed=9, n_materials=4, tex_size=16, hdri_size=(64, 32), smooth=True, n_lights=0)
    cam = sc.camera
    cam.bokeh, cam.aperture, cam.focus_distance = 1, 1.8, 3.0
    cam.rotation = abi.ErVec3(7.0, -11.0, 4.0)
    r = np.random.default_rng(4)
    sc.textures.append((abi._f32(r.random((8, 8, 2))), 8, 8, 2, 1))
    sc.textures.append((abi._f32(r.random((5, 7, 1))), 7, 5, 1, 1))
    sc._desc = None
    return sc


def _hd(r, n):
    hd = r.random((n, 20)).astype(np.float32)
    hd[:, 5] = np.where(r.random(n) < 0.1, 1.0, hd[:, 5] * 0.5)
    hd[:, 14:17] = r.normal(size=(n, 3))
    hd[:, 17:20] = r.normal(size=(n, 3))
    return hd


def _dirs(r, n):
    d = r.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def function_inputs(sc):
    """Input arrays of every function-level section on the rig scene `sc` (names = the driver's)."""
    inp = {}
    inp["rng_idx"] = np.array([0, 1, 2, 47, sc.x_res * sc.y_res - 1, 123456, 2**31 - 2], np.uint32)
    # camera rays: bokeh on, camera rotated
    r = np.random.default_rng(1)
    n = 500
    items = np.concatenate([r.integers(0, [sc.x_res, sc.y_res], (n, 2)).astype(np.float32), r.random((n, 5)).astype(np.float32)], 1)
    items[0, 2:] = 1.0                                           # next() can return exactly 1.0
    inp["cam_items"] = items
    # Tri::hit records: through a vertex, along an edge, back-facing (the origins lie on both sides), misses
    r = np.random.default_rng(2)
    n = 3000
    tri = r.integers(0, sc.tri_count, n)
    v = sc.vertices.reshape(-1, 3, 3)[tri]
    w = r.dirichlet([1, 1, 1], n).astype(np.float32)
    w[::10] = [1, 0, 0]
    w[::11, 2] = 0
    target = (v * w[:, :, None]).sum(1).astype(np.float32)
    origin = (target + r.normal(size=(n, 3)).astype(np.float32) * np.float32(0.7)).astype(np.float32)
    d = target - origin
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    inp["trihit_items"] = np.concatenate([ibits(tri.astype(np.int32)).reshape(-1, 1), origin, d], 1)
    # Disney: transmission == 1, L below the horizon, roughness / anisotropic at 0 and 1, un-normalised non-orthogonal frame
    r = np.random.default_rng(3)
    n = 2000
    hd, V, N, Lv = _hd(r, n), _dirs(r, n), _dirs(r, n), _dirs(r, n)
    Lv[::7] = -N[::7]
    rs = r.random((n, 3)).astype(np.float32)
    hd[1::40, 1], hd[2::40, 1], hd[3::40, 4], hd[4::40, 4] = 0.0, 1.0, 0.0, 1.0
    hd[5::40, 1], hd[5::40, 4] = 0.0, 1.0
    inp["disney_items"] = np.concatenate([hd, V, N, Lv], 1)
    inp["disney_rs"] = rs
    # spherical mappings: the six axis directions, the seam (z = +-0 and a hair either side of it at x < 0 and x > 0)
    r = np.random.default_rng(5)
    p = _dirs(r, 1500)
    p[:6] = [[0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1]]
    p[6:12] = [[1, 0, -0.0], [-1, 0, -0.0], [-1, 0, 1e-7], [-1, 0, -1e-7], [1, 0, 1e-7], [1, 0, -1e-7]]
    inp["sph_p"] = p
    grid = np.array([[u, v] for u in (0, 0.5, 1) for v in (0, 0.5, 1)], np.float32)
    inp["rev_uv"] = np.concatenate([r.random((1500, 2)).astype(np.float32), grid])
    # texture fetches: the 3-channel NO_FILTER, 2-channel and 1-channel BILINEAR textures and the HDRI, both entry points
    items = []
    n_tex = len(sc.textures)
    for tid in list(range(n_tex))[-3:] + [0, -1]:
        q = r.uniform(-2.5, 3.5, (400, 2)).astype(np.float32)
        for filtered in (0, 1):
            items.append(np.concatenate([np.full((400, 1), ibits(tid)), q, np.full((400, 1), np.float32(filtered))], 1))
    inp["texfetch_items"] = np.concatenate(items)
    return inp


def hdri_inputs(cdf, w, h):
    """The HDRI searches need the CDF the reference built: second job."""
    r = np.random.default_rng(6)
    vals = np.concatenate([r.random(3000).astype(np.float32), cdf[r.integers(0, w * h + 1, 300)], np.array([0.0, 1.0], np.float32)])
    xy = np.stack([r.integers(0, w, 600), r.integers(0, h, 600)], 1).astype(np.int32)
    xy[:4, 1] = 0                                                # row 0: sin(theta) = 0 -> inf / nan
    return {"hdri_search_vals": vals, "hdri_pdf_xy": xy}


def trace_rays(sc, seed=8, n=500):
    """4 n rays on the 300-triangle scene: n at vertices, n at edge midpoints, n into faces, n anywhere."""
    r = np.random.default_rng(seed)
    v = sc.vertices.reshape(-1, 3, 3)
    tri = r.integers(0, sc.tri_count, n)
    targets = [v[tri, r.integers(0, 3, n)],                                          # a vertex (shared in a welded mesh)
               ((v[tri, 0] + v[tri, 1]) * np.float32(0.5)).astype(np.float32),      # an edge
               (v[tri] * r.dirichlet([1, 1, 1], n).astype(np.float32)[:, :, None]).sum(1).astype(np.float32)]
    cam = np.array([sc.camera.position.x, sc.camera.position.y, sc.camera.position.z], np.float32)
    o, d = [], []
    for k, t in enumerate(targets):
        org = np.where((np.arange(n) % 2 == 0)[:, None], cam[None, :], (t + r.normal(size=(n, 3)) * 0.6).astype(np.float32)).astype(np.float32)
        o.append(org)
        d.append(t.astype(np.float32) - org)
    o.append(np.tile(cam[None, :], (n, 1)))
    rd = r.normal(size=(n, 3)).astype(np.float32)
    rd[:, 2] = np.abs(rd[:, 2]) + 0.5
    rd[::50, 0] = 0.0                                                                # axis-parallel components
    rd[25::50, 1] = 0.0
    d.append(rd)
    o, d = np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


_SHAPES = {"graze_pos": (-1, 3), "graze_allpos": (-1, 3), "rng_states": (-1, 16), "rng_values": (-1, 16), "cam_rays": (-1, 6), "trihit_rec": (-1, 17), "closest_pos": (-1, 3),
           "disney_eval": (-1, 3), "disney_sample": (-1, 3), "sph_uv": (-1, 2), "rev_p": (-1, 3), "texfetch": (-1, 3)}


def make_functions():
    out = {}
    rig = rig_scene()
    for k, v in scene_arrays(rig).items():
        out["rig_" + k] = v
    inp = function_inputs(rig)
    res = run_reference({**job_scene(rig), **inp})
    # the CDF: one array, whatever the six functions are (no transcendental in HDRI::generateCDF) -- checked, then used for the searches
    assert np.array_equal(res["libm"]["hdri_cdf"], res["er"]["hdri_cdf"])
    hin = hdri_inputs(res["libm"]["hdri_cdf"], rig.hdri[1], rig.hdri[2])
    res2 = run_reference({**job_scene(rig), **hin})
    inp.update(hin)
    trace, _, _, _ = load(TRACE_SCENE)          # its arrays are in that file already: not stored again
    o, d = trace_rays(trace)
    ro, rd = trace_rays(trace, seed=88, n=25)          # a reserve of the same kinds, to replace box-corner rays from
    res3 = run_reference({**job_scene(trace), "closest_o": np.concatenate([o, ro]), "closest_d": np.concatenate([d, rd])})
    # Box-corner rays: a ray through a vertex that is a corner of its leaf's box meets that box where entry and exit
    # parameter are mathematically EQUAL, and the reference's slab test (`tmin > tmax`) then keeps or drops the leaf on the rounding
    # of six products -- a tie decided by the reference's own tree, not by the scene.  Such rays (the reference's traversal and its
    # Tri::hit over every triangle disagree) are recorded apart, as graze_*: the oracle, which restates that tree, must reproduce
    # them; the HIP path has a tree of its own and must give what Tri::hit over every triangle gives.  Each is replaced, at its
    # index, by the next ray of the reserve (vertex-aimed ones come first there) on which the two agree.
    graze = np.nonzero(res3["libm"]["closest_tri"] != res3["libm"]["closest_alltri"])[0]
    assert np.array_equal(graze, np.nonzero(res3["er"]["closest_tri"] != res3["er"]["closest_alltri"])[0])
    n, nr = len(o), len(ro)
    main_graze = graze[graze < n]
    free = [k for k in range(n, n + nr) if k not in set(graze.tolist())]
    assert 0 < len(main_graze) <= len(free), (len(main_graze), len(free))
    src = np.arange(n)
    src[main_graze] = free[:len(main_graze)]
    inp["closest_o"], inp["closest_d"] = np.concatenate([o, ro])[src], np.concatenate([d, rd])[src]
    inp["graze_o"], inp["graze_d"], inp["graze_index"] = o[main_graze], d[main_graze], main_graze.astype(np.int32)
    for m in MODES:
        full = res3[m]
        res3[m] = {k: full[k].reshape(len(src) + nr, -1)[src].reshape(-1) for k in ("closest_tri", "closest_pos")}
        for k in ("tri", "pos", "alltri", "allpos"):
            res3[m]["graze_" + k] = full["closest_" + k].reshape(n + nr, -1)[main_graze].reshape(-1)
        assert np.array_equal(res3[m]["closest_tri"], full["closest_alltri"][src])
    for k, v in inp.items():
        out[k] = v
    for m in MODES:
        merged = {**res[m], **{k: v for k, v in res2[m].items() if k in ("hdri_search", "hdri_pdf")},
                  **res3[m]}
        for k, v in merged.items():
            out[f"{k}_{m}"] = v.reshape(_SHAPES[k]) if k in _SHAPES else v
    return out


# ---------------------------------------------------------------- Tri::hit under varied uvs and signs
TRIHIT_UV_SEED, TRIHIT_UV_RAYS = 19, 1000
TRI_ARRAYS = ("vertices", "normals", "tangents", "uvs", "tangent_sign")


def trihit_uv_scene():
    """the 300-triangle scene of the existing golden with the uvs and signs of tests/uv_scenes.py"""
    import uv_scenes
    trace, _, _, _ = load(TRACE_SCENE)
    return uv_scenes.varied(trace, TRIHIT_UV_SEED)


def make_trihit_uv():
    """1 000 rays aimed like function_inputs' (through a vertex, along an edge, from both sides, misses); the five per-triangle arrays
    Tri::hit reads are stored next to the outputs as rig_*"""
    sc = trihit_uv_scene()
    r = np.random.default_rng(12)
    n = TRIHIT_UV_RAYS
    tri = r.integers(0, sc.tri_count, n)
    tri[:70] = np.repeat(np.arange(7), 10)                       # uv_scenes.SPECIAL: ten rays at each
    v = sc.vertices.reshape(-1, 3, 3)[tri]
    w = r.dirichlet([1, 1, 1], n).astype(np.float32)
    w[::10] = [1, 0, 0]
    w[::11, 2] = 0
    target = (v * w[:, :, None]).sum(1).astype(np.float32)
    origin = (target + r.normal(size=(n, 3)).astype(np.float32) * np.float32(0.7)).astype(np.float32)
    d = target - origin
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    items = np.concatenate([ibits(tri.astype(np.int32)).reshape(-1, 1), origin, d], 1)
    res = run_reference({**job_scene(sc), "trihit_items": items})
    out = {"rig_" + k: getattr(sc, k) for k in TRI_ARRAYS}
    out["trihit_items"] = items
    for m in MODES:
        out["trihit_ok_" + m] = res[m]["trihit_ok"]
        out["trihit_rec_" + m] = res[m]["trihit_rec"].reshape(-1, 17)
    return out


# ---------------------------------------------------------------- whole path
def make_render(golden_name):
    sc, _, _, _ = load(golden_name)
    res = run_reference(job_scene(sc, SPP))
    out = {"spp": np.array([SPP], np.int64)}
    for m in MODES:
        assert res[m]["max_bounces"][0] == res["libm"]["max_bounces"][0]
        for p in PASSES:
            out[f"pass_{p}_{m}"] = res[m]["pass_" + p].reshape(sc.y_res, sc.x_res, 4)
        out[f"samples_{m}"] = res[m]["samples"]
        out[f"rng_{m}"] = res[m]["rng"]
    out["max_bounces"] = np.array([int(res["libm"]["max_bounces"][0])], np.int64)    # the reference's compiled-in MAXBOUNCES
    return out


FIXTURES = {"reference_functions": make_functions,
            "reference_cornell_32x32": lambda: make_render("cornell_32x32_4spp"),
            "reference_torture_300tri_32x24": lambda: make_render("torture_300tri_32x24_4spp"),
            "reference_trihit_uv": make_trihit_uv}
MAX_BYTES = 1 << 20      # of one committed file


def main(out_dir=HERE):
    if not available():
        raise SystemExit("oracle/_ref/ref_libm and ref_er are missing: `make -C oracle ref` on a machine that has the reference")
    for name, make in FIXTURES.items():
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **make())
        size = os.path.getsize(path)
        assert size < MAX_BYTES, (name, size)
        print(name, size, "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:2])
