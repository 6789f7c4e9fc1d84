"""The streaming schedule's hand-offs through LDS (csrc/er_stream.hip, ER_STREAM_LDS_HANDOFF).

A tracer wave hands a finished ray to the shader waves through the slot's LDS words -- the winner of a closest-hit ray in s_hit, a
certain shadow verdict as a flag of the slot's s_wait word -- and through the slot's record in device memory only for what is rare: a
second candidate or an overflow mark (hit2), the candidates of an ambiguous verdict (2 and 3).  The tracer's ring visit takes its new
rays first and begins them after the publish.  None of this may change anything readable: every case renders the same frame in the
streaming and in the wavefront schedule (which knows neither LDS words nor ring visits) and compares the planes, the sample counts, the
RNG states and every event counter, with 0 differing bits.
"""
import numpy as np
import pytest

from elevenrender_amd import abi, render, scenes

pytestmark = pytest.mark.gpu

PLANES = ("beauty", "denoise", "normal", "tangent", "bitangent")
COUNTS = ("paths", "bounce_samples", "rays", "shaded_hits", "hdri_samples")
COUNTS_INSTRUMENTED = ("node_visits", "tri_tests", "texel_fetches")      # (ER_FLAG_COUNTERS)
LIGHTS = abi.FLAG_POINT_LIGHTS | abi.FLAG_MIS
KNOBS = ("ER_STREAM_WAVES", "ER_STREAM_SPEC_FORM", "ER_STREAM_KEEP")      # read by er_render_begin (csrc/er_stream_host.cpp stream_choose_form)


def run(sc, chunks, flags, max_bounces=8, blocking=True, **kw):
    """One render, `chunks` calls of er_render_samples (blocking = False: all of them before a single er_wait)."""
    rm = render.RenderingManager(render.RenderParameters(max_bounces=max_bounces, flags=flags, **kw))
    rm.start_rendering(sc)
    for n in chunks:
        rm.render(n, blocking=blocking)
    if not blocking:
        rm.wait()
    out = {p: rm.get_pass(p) for p in PLANES}
    out["samples"], out["rng"], out["counters"] = rm.read_samples(), rm.read_rng(), rm.counters()
    out["stream"] = rm.stream_info() if flags & abi.FLAG_STREAM else None
    rm.close()
    return out


def assert_no_bit_differs(s, w, what, instrumented=False):
    for p in PLANES:
        differing = int((s[p].view(np.uint32) != w[p].view(np.uint32)).sum())
        assert differing == 0, (what, p, differing)
    assert (s["samples"] == w["samples"]).all(), what
    assert (s["rng"] == w["rng"]).all(), what
    for k in COUNTS + (COUNTS_INSTRUMENTED if instrumented else ()):
        assert s["counters"][k] == w["counters"][k], (what, k, s["counters"][k], w["counters"][k])


def soup_2000():
    return scenes.soup(2000, 64, 48, seed=31, hdri_size=(64, 32))


def with_lights(sc):
    sc.point_lights = scenes.point_lights(5, seed=3, lo=(-0.8, -0.8, 2.2), hi=(0.8, 0.8, 3.8))
    sc._desc = None
    return sc


@pytest.fixture(scope="module")
def wavefront_soup():
    """Case 1's frame in the wavefront schedule, whole and as rank 0's share of 2 and of 8, plain and with ER_FLAG_COUNTERS: rendered once."""
    sc = soup_2000()
    return {(world, count): run(sc, [1, 3], abi.FLAG_WAVEFRONT | count, rank=0, world=world) for world in (1, 2, 8) for count in (0, abi.FLAG_COUNTERS)}


# A 64 x 48 frame is a few pixels per CU, which by itself always gets the 12-wave speculative form: the launcher's A/B knobs pick the
# kernel's other forms for it, as test_gpu_parity.py does, and the form the launch reports is asserted.
FORMS = {
    "whole share, form 0, 16 waves": (1, {"ER_STREAM_WAVES": "16", "ER_STREAM_SPEC_FORM": "0", "ER_STREAM_KEEP": "0"}, (0, 16)),
    "whole share, form 0, 12 waves": (1, {"ER_STREAM_SPEC_FORM": "0", "ER_STREAM_KEEP": "0"}, (0, 12)),
    "rank 0 of 2, form 1 (keep rule)": (2, {"ER_STREAM_WAVES": "16", "ER_STREAM_SPEC_FORM": "0", "ER_STREAM_KEEP": "1"}, (1, 16)),
    "rank 0 of 8, form 2 (speculative)": (8, {}, (2, 12)),
    "rank 0 of 8, form 2, 16 waves": (8, {"ER_STREAM_WAVES": "16"}, (2, 16)),
}


@pytest.mark.parametrize("name", list(FORMS))
def test_soup_in_every_form_of_the_kernel(name, wavefront_soup, monkeypatch):
    """Case 1: scenes.soup(2000, 64, 48), 8 bounces, 4 samples in two calls; the whole frame in the plain form, rank 0's half in the form
    with the keep rule, rank 0's eighth in the speculative form (2 000 triangles >= the 1 000 that form asks for), each also with
    ER_FLAG_COUNTERS (the instrumented instances; in the speculative form the tracers then add to the slot's tallies at a publish)."""
    world, env, (form, waves) = FORMS[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = soup_2000()
    for count in (0, abi.FLAG_COUNTERS):
        s = run(sc, [1, 3], abi.FLAG_STREAM | count, rank=0, world=world)
        assert (s["stream"]["form"], s["stream"]["waves"]) == (form, waves), (name, s["stream"])
        assert_no_bit_differs(s, wavefront_soup[(world, count)], (name, count), instrumented=count != 0)
    assert s["counters"]["paths"] > 0


@pytest.mark.parametrize("world,form", [(1, 0), (8, 2)])
def test_soup_with_point_lights_and_mis(world, form, monkeypatch):
    """Case 2: the same soup with five point lights and MIS: a slot has a closest-hit ray and two shadow queries in flight together, so both
    occluded flags, the records' light line (stride 384) and the shadow record index >= slots are in use."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if form == 0:
        monkeypatch.setenv("ER_STREAM_WAVES", "16")
        monkeypatch.setenv("ER_STREAM_SPEC_FORM", "0")
        monkeypatch.setenv("ER_STREAM_KEEP", "0")
    sc = with_lights(soup_2000())
    s = run(sc, [1, 3], abi.FLAG_STREAM | LIGHTS, rank=0, world=world)
    w = run(sc, [1, 3], abi.FLAG_WAVEFRONT | LIGHTS, rank=0, world=world)
    assert s["stream"]["form"] == form, s["stream"]
    assert_no_bit_differs(s, w, ("lights", world))
    assert s["counters"]["rays"] > s["counters"]["bounce_samples"] > 0      # (shadow queries were traced)


def coincident_soup(copies, x_res=48, y_res=32):
    """scenes.soup's 300 triangles, every one present `copies` times in the same place."""
    v = np.concatenate([scenes.soup_geometry(300, seed=7)] * copies)
    n = len(v)
    normals, tangents = scenes.face_frame(v)
    uvs = np.tile(np.array([[0, 0], [1, 0], [0, 1]], np.float32), (n, 1, 1))
    cam = abi.default_camera()
    cam.position = abi.ErVec3(0.01, 0.02, -0.5)
    return abi.SceneData(v, normals, tangents, uvs, np.ones(n, np.float32), np.zeros(n, np.int32), [abi.default_material()],
                         hdri=scenes.sky_hdri(64, 32), camera=cam, x_res=x_res, y_res=y_res)


def rare_results(sc, n=4000):
    """What er_debug_trace_rays (the production traversal) says about n camera-like rays of the scene and about as many shadow queries along
    the same rays whose limit is the hit's own distance: closest results with two survivors / with overflow, shadow verdicts 2 / 3."""
    rng = np.random.default_rng(3)
    o = np.tile(np.array([[0.01, 0.02, -0.5]], np.float32), (n, 1))
    d = rng.normal(size=(n, 3)).astype(np.float32) * np.float32(0.35)
    d[:, 2] = 1.0
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    rm = render.RenderingManager(render.RenderParameters(max_bounces=8))
    rm.start_rendering(sc)
    tri, slot, pos, dist, info = rm.debug_trace_rays(o, d)
    hit = tri >= 0
    # no triangle exempt, the limit at the nearest triangles themselves: their intervals straddle it
    occ, sinfo = rm.debug_trace_rays(o[hit], d[hit], self_slots=np.full(int(hit.sum()), -1, np.int32), limits=dist[hit])
    rm.close()
    return {"hits": int(hit.sum()), "two": int((info[hit] == 1).sum()), "overflow": int((info[hit] == 2).sum()),
            "verdict2": int((sinfo == 2).sum()), "verdict3": int((sinfo == 3).sum())}


@pytest.mark.parametrize("copies", [2, 3])
def test_coincident_triangles_take_the_slot_record_path(copies):
    """Case 3: a soup of 300 triangles with every triangle present twice, 48 x 32, 4 samples.  Equal distances are what leaves a second
    candidate (hit2 >= 0, ST_HIT2) and an ambiguous shadow verdict (2) in the slot's record.  An overflow (hit2 = -2) and verdict 3 need
    THREE candidates whose distance intervals overlap, and an interval is 4e-6 of the distance wide: two copies cannot make one.  Measured
    with the rays below on MI355X: of 1 148 hits, two copies give 1 148 results with two survivors, 0 with overflow, 1 148 verdicts 2
    and 0 verdicts 3; three copies give 1 148 overflows and 1 148 verdicts 3.  So the scene is rendered a second time with every
    triangle present three times, and between them the two scenes must show every one of the four kinds before the images are
    compared.  (The kinds are shown with hand-made limits -- a shadow query along the camera ray whose limit is the hit's own distance --
    which says that the scene and the traversal can produce them, not how often the frame's own shadow rays do.)  The two schedules
    share the traversal, so ties resolve alike: 0 differing bits."""
    sc = coincident_soup(copies)
    kinds = rare_results(sc)
    print(f"{copies} copies: {kinds}")
    assert kinds["hits"] > 1000, kinds
    if copies == 2:
        assert kinds["two"] > 0 and kinds["verdict2"] > 0, kinds
    else:
        assert kinds["overflow"] > 0 and kinds["verdict3"] > 0, kinds
    for flags in (0, LIGHTS):
        if flags:
            with_lights(sc)
        s = run(sc, [4], abi.FLAG_STREAM | flags)
        w = run(sc, [4], abi.FLAG_WAVEFRONT | flags)
        assert_no_bit_differs(s, w, ("coincident", copies, flags))
        assert s["counters"]["shaded_hits"] > 0


def test_cornell_box_with_most_slots_and_lanes_idle():
    """Case 4: Cornell box, 16 x 16, 3 samples: 256 pixels on 256 x 1 024 slots and 12 triangles -- no slot ring is ever full and every ring
    visit of a tracer wave happens with most of its lanes idle."""
    sc = scenes.cornell(16, 16)
    s = run(sc, [3], abi.FLAG_STREAM, max_bounces=5)
    w = run(sc, [3], abi.FLAG_WAVEFRONT, max_bounces=5)
    assert_no_bit_differs(s, w, "cornell 16 x 16")
    assert s["counters"]["paths"] == 3 * 256


def test_three_asynchronous_calls_before_one_wait(wavefront_soup):
    """Case 5: three er_render_samples_async (1 + 1 + 2 samples) before a single er_wait on case 1's frame: three launches back to back, none
    of which may assume anything about the LDS words the one before it left."""
    s = run(soup_2000(), [1, 1, 2], abi.FLAG_STREAM, blocking=False)
    assert_no_bit_differs(s, wavefront_soup[(1, 0)], "three asynchronous calls")
