"""The streaming schedule's per-slot hand-off word (s_wait) and the results beside it, as a host-thread model under ThreadSanitizer.

tests/native/handoff_model.cpp: tracer threads publish RESULT, THEN COUNT (the winner of a closest-hit ray in the slot's s_hit word, a certain
shadow verdict as a flag of the add itself, the rare rest -- flagged -- in the slot's record; then the add of flags - 1 to the slot's s_wait
word, and the tracer whose add takes the count to zero appends the slot to the shade ring); shader threads read COUNT, THEN RESULT.  The
words a result travels through are plain memory, so ThreadSanitizer reports any hand-off that the add and the rings (csrc/er_ring.h, the
kernel's own functions) leave unordered, and every step of a slot expects its own values, so a consumer that sees a result older than its
count fails by value.  No GPU needed; no sanitizer is loaded into python: the model is a program of its own."""
import os
import platform
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "handoff_model.cpp")
KERNEL = os.path.join(ROOT, "elevenrender_amd", "csrc", "er_stream.hip")


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-pthread", "-DER_RING_HOST_MODEL"] + flags + [SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("handoff"), "handoff_model", ["-O2"])


@pytest.fixture(scope="module")
def model_tsan(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("handoff_tsan"), "handoff_model_tsan", ["-O1", "-g", "-fsanitize=thread"])


def _run(exe, *args, timeout=300):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    cmd = [exe] + [str(a) for a in args]
    if exe.endswith("_tsan"):
        cmd = ["setarch", platform.machine(), "-R"] + cmd      # (as tests/test_stream_protocol_cpu.py: g++ 11's runtime and address randomisation)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)


# slots, steps per slot, tracer threads, shader threads
CONFIGS = [(8, 400, 2, 2), (64, 100, 3, 1), (3, 2000, 2, 2), (1, 3000, 2, 1), (200, 30, 2, 2)]      # (at most four threads: waiters spin)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_no_consumer_sees_a_result_older_than_its_count(model, cfg):
    r = _run(model, *cfg)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert "stale results 0, wrong words 0, guards 0, rings empty" in r.stdout, r.stdout
    assert f"steps shaded {cfg[0] * cfg[1]} (want {cfg[0] * cfg[1]})" in r.stdout, r.stdout


def test_thread_sanitizer_finds_no_unordered_hand_off(model_tsan):
    for cfg in [(8, 100, 2, 2), (32, 40, 3, 1), (2, 500, 2, 2)]:
        r = _run(model_tsan, *cfg, timeout=600)
        assert "ThreadSanitizer" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == 0, (r.stdout, r.stderr[-2000:])


def test_the_model_has_teeth_count_before_result_is_caught(model):
    """Negative control, deterministic: one thread plays a tracer that adds to the count before it writes its result and a shader that
    reads in between; the model must call the result stale."""
    r = _run(model, "script")
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert re.search(r"the shader saw a stale result in [1-9]\d* steps", r.stdout), r.stdout


def test_model_and_kernel_agree_on_the_fields_of_the_word():
    """The model's constants are the kernel's, and the kernel asserts that they do not overlap."""
    src, mod = open(KERNEL).read(), open(SRC).read()
    for name, short in (("ST_FIN", "FIN"), ("ST_ESC", "ESC"), ("ST_AMB1", "AMB1"), ("ST_AMB2", "AMB2"), ("ST_OCC1", "OCC1"), ("ST_OCC2", "OCC2"),
                        ("ST_HIT2", "HIT2"), ("ST_COUNT_MASK", "COUNT_MASK")):
        k = re.search(rf"#define {name} (0x[0-9A-Fa-f]+)u", src)
        m = re.search(rf"\b{short} = (0x[0-9A-Fa-f]+)u", mod)
        assert k and m and int(k.group(1), 16) == int(m.group(1), 16), (name, k and k.group(1), m and m.group(1))
    assert "overlap neither each other nor the in-flight count" in src
    assert "st_lds_bytes(FORM, TOP_NODES) <= ST_LDS_LIMIT" in src
