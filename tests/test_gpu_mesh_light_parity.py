"""ER_FLAG_MESH_LIGHTS on the GPU against the oracle's mirror of it (oracle/er_oracle.cpp, rules: csrc/er_shade.h 2-7), on bits.

The oracle takes the emitter ORDER from the device (input triangle ids in table order: its own tree has another leaf order, and the
order decides which emitter a draw picks), builds weights, CDF and P itself in the float order csrc/er_lights.hip documents, and
answers the emitter shadow query by brute force over all triangles.  Every comparison here is on bits and has no exception budget:
the scene, mesh_light_scenes.lit_soup, is soup geometry (no coplanar shared edges, no exact ties).  The one Cornell-derived case keeps
the allowance the Cornell trace test of tests/test_gpu_function_level.py has for exact ties on shared wall edges, and no more.

What lit_soup exercises -- visible and occluded emitter samples, the skips, BRDF-sampled hits on emitters reached directly and through
opacity pass-throughs, Le from two textures, opacities beyond [0, 1] -- is counted on the CPU from the oracle's records over the very
pixels traced here (tests/test_mesh_light_scenes_cpu.py); the counts are printed here again from this run's oracle.

Left out: er_lights_scan_kernel with chunk >= 2 needs more than 1 048 576 triangles (1 024 workgroups of 1 024 slots), which is outside
a test of a few seconds."""
import functools

import numpy as np
import pytest

import mesh_light_scenes as mls
from elevenrender_amd import abi, render

from test_gpu_function_level import _rec_tuple
from test_gpu_mesh_lights import textured_scene

pytestmark = pytest.mark.gpu

MESH = abi.FLAG_MESH_LIGHTS
PLANES = ("beauty", "normal", "tangent", "bitangent")


@functools.lru_cache(maxsize=None)
def lit():
    return mls.lit_soup()


def gpu(sc, chunks, flags, max_bounces=mls.LIT_MAX_BOUNCES, **kw):
    rm = render.RenderingManager(render.RenderParameters(max_bounces=max_bounces, flags=flags, **kw))
    rm.start_rendering(sc)
    for n in chunks:
        rm.render(n)
    out = {p: rm.get_pass(p) for p in PLANES}
    out["samples"], out["rng"] = rm.read_samples(), rm.read_rng()
    out["order"] = rm.debug_light_table()[0]
    out["stream"] = rm.stream_info() if flags & abi.FLAG_STREAM else None
    rm.close()
    return out


_oracle_frames = {}


def oracle_frame(oracle_mod, sc, order, spp, flags=0, max_bounces=mls.LIT_MAX_BOUNCES):
    """the oracle's frame for one emitter order, rendered once per order (single-threaded) and left unchanged"""
    key = (id(sc), bytes(np.ascontiguousarray(order, np.int32)), spp, flags, max_bounces)
    if key not in _oracle_frames:
        orc = oracle_mod.Oracle(sc, math_mode=oracle_mod.MATH_ER, max_bounces=max_bounces, threads=1, flags=flags | MESH)
        orc.set_emitters(order)
        orc.render(spp)
        out = {p: orc.read_pass(abi.PASS_NAMES[p]) for p in PLANES}
        out["samples"], out["rng"] = orc.read_samples(), orc.read_rng()
        orc.close()
        for v in out.values():
            v.setflags(write=False)
        _oracle_frames[key] = out
    return _oracle_frames[key]


def assert_bit_equal(g, o, what, mask=None):
    shape = g["beauty"].shape[:2]
    for p in PLANES + ("samples", "rng"):
        x, y = np.asarray(g[p]), np.asarray(o[p])
        if p in PLANES:
            x, y = x.view(np.uint32)[..., :3], y.view(np.uint32)[..., :3]
        x, y = x.reshape(shape + (-1,)), y.reshape(shape + (-1,))
        if mask is not None:
            x, y = x[mask], y[mask]
        differing = int((x != y).sum())
        assert differing == 0, (what, p, differing)


@pytest.mark.parametrize("mis,max_bounces", mls.TRACE_CONFIGS)
def test_per_bounce_trace_on_lit_soup(oracle_mod, mis, max_bounces):
    """debug_trace_pixel against Oracle.trace_pixel: 200 pixels, two consecutive samples each after two rendered samples of history;
    every record field, light_occ included.  max_bounces 2 makes the last-bounce rule decide on every path."""
    sc = lit()
    rm = render.RenderingManager(render.RenderParameters(max_bounces=max_bounces, flags=MESH | mis | abi.FLAG_HOST_BUILD))
    rm.start_rendering(sc)
    order = rm.debug_light_table()[0]
    assert (order == mls.host_order(sc)).all()          # the order the CPU test counted the classes with
    pixels = mls.traced_pixels(sc)
    orc, traces = mls.oracle_traces(oracle_mod, sc, order, mis, max_bounces, pixels)
    rm.render(2)
    n_rec = n_bad = n_shadow = n_light = 0
    for idx, rep, o in traces:
        g = rm.debug_trace_pixel(idx, max_recs=32)
        assert len(g) == len(o), (idx, rep, len(g), len(o))
        for a, b in zip(g, o):
            n_rec += 1
            traced = a.shadow_occ >= 0                   # (the kernels skip an HDRI shadow ray whose outcomes add the same value)
            n_shadow += int(traced)
            n_light += int(a.light_occ >= 0)
            if _rec_tuple(a, traced) != _rec_tuple(b, traced):
                n_bad += 1
                if n_bad <= 3:
                    print("pixel", idx, "sample", rep, "bounce", a.bounce, _rec_tuple(a, traced), "!=", _rec_tuple(b, traced),
                          "oracle mesh fields", b.mesh_sample, b.mesh_k, b.mesh_le_tex, b.mesh_opacity, b.mesh_hit, b.mesh_d)
    counts = mls.class_counts(traces)
    print(f"lit_soup mis={mis} max_bounces={max_bounces}: {n_rec} records, {n_shadow} HDRI queries, {n_light} emitter queries, {n_bad} differ; classes {counts}")
    assert n_light == counts["visible"] + counts["occluded"] and n_light > 20
    assert n_bad == 0
    img, ref = rm.get_pass("beauty"), orc.read_pass(0)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()
    assert (rm.read_samples() == orc.read_samples()).all() and (rm.read_rng() == orc.read_rng()).all()
    rm.close()
    orc.close()


@pytest.mark.parametrize("builder", [abi.FLAG_HOST_BUILD, abi.FLAG_GPU_BUILD], ids=["host-build", "gpu-build"])
@pytest.mark.parametrize("schedule", [abi.FLAG_STREAM, abi.FLAG_WAVEFRONT, abi.FLAG_MEGAKERNEL], ids=["stream", "wavefront", "megakernel"])
def test_images_after_6_samples(oracle_mod, schedule, builder):
    sc = lit()
    g = gpu(sc, [6], MESH | schedule | builder)
    assert len(g["order"]) == len(mls.host_order(sc))
    assert_bit_equal(g, oracle_frame(oracle_mod, sc, g["order"], 6), f"schedule {schedule} builder {builder}")


def test_image_with_mis_in_two_calls(oracle_mod):
    sc = lit()
    g = gpu(sc, [2, 4], MESH | abi.FLAG_MIS | abi.FLAG_STREAM)
    assert_bit_equal(g, oracle_frame(oracle_mod, sc, g["order"], 6, flags=abi.FLAG_MIS), "ER_FLAG_MIS, default builder, two calls")


def test_rank_1_of_3_on_its_own_tiles(oracle_mod):
    sc = lit()
    g = gpu(sc, [6], MESH | abi.FLAG_HOST_BUILD, rank=1, world=3)
    tiles_x, tiles_y = -(-sc.x_res // 8), -(-sc.y_res // 8)
    own = np.array([[(tx + ty) % 3 == 1 for tx in range(tiles_x)] for ty in range(tiles_y)])
    mask = np.repeat(np.repeat(own, 8, 0), 8, 1)[:sc.y_res, :sc.x_res]
    assert 0.25 < mask.mean() < 0.45
    assert_bit_equal(g, oracle_frame(oracle_mod, sc, g["order"], 6), "rank 1 of 3", mask=mask)


# lit_soup's frame is a few pixels per CU, which by itself gets the 12-wave speculative form; the launcher's knobs (csrc/er_stream_host.cpp
# stream_choose_form) pick the others, as tests/test_gpu_stream_handoff.py does.  3 000 triangles >= ER_STREAM_SPEC_MIN_TRIS.
FORMS = {
    "form 2 (speculative), 12 waves": ({}, (2, 12), True),
    "form 2 (speculative), 16 waves": ({"ER_STREAM_WAVES": "16"}, (2, 16), True),
    "form 2, forced": ({"ER_STREAM_WAVES": "16", "ER_STREAM_SPEC_FORM": "1"}, (2, 16), True),
    "form 1 (keep rule)": ({"ER_STREAM_WAVES": "16", "ER_STREAM_SPEC_FORM": "0", "ER_STREAM_KEEP": "1"}, (1, 16), False),
}


@pytest.mark.parametrize("name", list(FORMS))
def test_streaming_forms(oracle_mod, name, monkeypatch):
    """ER_FLAG_MESH_LIGHTS changes an opaque bounce's draw count from 5 to 8, which is what a speculative sample's guessed RNG state is
    predicted from: the forms that start speculative samples, and the keep rule, against the oracle, with the speculation counters
    showing that speculative samples really started."""
    knobs, (form, waves), speculative = FORMS[name]
    for k in ("ER_STREAM_WAVES", "ER_STREAM_SPEC_FORM", "ER_STREAM_KEEP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    sc = lit()
    g = gpu(sc, [2, 4], MESH | abi.FLAG_STREAM)
    si = g["stream"]
    print(f"{name}: form {si['form']}, {si['waves']} waves; speculative samples started {si['spec_started']}, right {si['spec_right']}, wrong {si['spec_wrong']}")
    assert (si["form"], si["waves"]) == (form, waves), si
    if speculative:
        assert si["spec_started"] > 0 and si["spec_right"] > 0, si
    else:
        assert si["spec_started"] == 0, si
    assert_bit_equal(g, oracle_frame(oracle_mod, sc, g["order"], 6), name)


def test_cornell_derived_scene_agrees_with_the_mirror(oracle_mod):
    """textured_scene (the scene of tests/test_gpu_mesh_lights.py): the old scenes agree with the mirror too.  Cornell walls share edges,
    where two hits at exactly equal distance resolve by traversal order: at most 2 differing records and at least 0.999 of the pixels
    bit equal, the allowance of the Cornell trace test, and no more."""
    sc = textured_scene(48, 36)
    rm = render.RenderingManager(render.RenderParameters(max_bounces=5, flags=MESH))
    rm.start_rendering(sc)
    order = rm.debug_light_table()[0]
    pixels = mls.traced_pixels(sc)
    orc, traces = mls.oracle_traces(oracle_mod, sc, order, 0, 5, pixels)
    rm.render(2)
    n_rec = n_bad = n_light = 0
    for idx, rep, o in traces:
        g = rm.debug_trace_pixel(idx, max_recs=32)
        assert len(g) == len(o), (idx, rep, len(g), len(o))
        for a, b in zip(g, o):
            n_rec += 1
            n_light += int(a.light_occ >= 0)
            traced = a.shadow_occ >= 0
            n_bad += int(_rec_tuple(a, traced) != _rec_tuple(b, traced))
    print(f"textured_scene: {n_rec} records, {n_light} emitter queries, {n_bad} differ")
    assert n_light > 100 and n_bad <= 2
    rm.render(4)
    orc.render(4)
    same = np.ones((sc.y_res, sc.x_res), bool)
    for p, op in (("beauty", abi.PASS_BEAUTY), ("normal", abi.PASS_NORMAL)):
        same &= (rm.get_pass(p).view(np.uint32) == orc.read_pass(op).view(np.uint32)).all(-1)
    same &= (rm.read_rng() == orc.read_rng()).reshape(same.shape)
    print(f"textured_scene: {same.mean():.6f} of pixels bit equal after 6 samples and the traces")
    assert same.mean() >= 0.999
    rm.close()
    orc.close()
