"""The HDRI trig tables' host twin (csrc/er_hdri_trig.h, er_debug_hdri_trig_host) against er_math.h, without a GPU.

The table kernel and its host twin run the same `__host__ __device__` entry functions; here the host side is compared with the
oracle's build of er_math.h (oracle_math, mode 1) on the arguments the bounce step forms, for every row and column -- the edges
x = 0, width - 1, y = 0 (sine 0: the pdf of that row is inf) and height - 1 among them -- bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

from elevenrender_amd import abi

PIF = np.float32(3.14159265358979323846)
SIZES = [(1, 1), (2, 1), (6, 4), (7, 5), (64, 32), (2048, 1024)]


def host_table(w, h):
    cols, rows = np.zeros((w, 4), np.uint32), np.zeros((h, 6), np.uint32)
    up = C.POINTER(C.c_uint32)
    abi.check(abi.load().er_debug_hdri_trig_host(w, h, cols.ctypes.data_as(up), rows.ctypes.data_as(up)))
    return cols, rows


def er_math(L, kind, x):
    x = np.ascontiguousarray(x, np.float32)
    y, out = np.zeros_like(x), np.empty_like(x)
    P = C.POINTER(C.c_float)
    L.oracle_math(kind, 1, x.ctypes.data_as(P), y.ctypes.data_as(P), out.ctypes.data_as(P), x.size)
    return out


def trunc(x):
    return np.asarray(x, np.float32).astype(np.int32)      # (every value here is far inside int32: ermath::f2i truncates)


def limit_uv(u):
    return (u + (-(u > 1).astype(np.int32) - (u < 0).astype(np.int32)).astype(np.float32)).astype(np.float32)


def same(words, want):
    return (np.ascontiguousarray(words, np.uint32) == np.ascontiguousarray(want, np.float32).view(np.uint32)).all()


@pytest.mark.parametrize("w,h", SIZES)
def test_host_twin_agrees_with_er_math(oracle_mod, w, h):
    L = oracle_mod.lib()
    cols, rows = host_table(w, h)
    fw, fh = np.float32(w), np.float32(h)
    x, y = np.arange(w, dtype=np.int32), np.arange(h, dtype=np.int32)
    iu = limit_uv(trunc((x.astype(np.float32) / fw) * fw).astype(np.float32) / fw)
    iv = limit_uv(trunc((y.astype(np.float32) / fh) * fh).astype(np.float32) / fh)
    arg = ((iu * np.float32(2)) * PIF - PIF).astype(np.float32)
    iy = trunc(iv * fh)
    py = -er_math(L, 1, iv * PIF)
    assert same(cols[:, 0], er_math(L, 1, arg)) and same(cols[:, 1], -er_math(L, 0, arg)) and same(cols[:, 3], iu)
    assert (cols[:, 2].view(np.int32) == trunc(iu * fw)).all()
    assert same(rows[:, 0], py) and same(rows[:, 1], np.sqrt(np.float32(1) - py * py, dtype=np.float32)) and same(rows[:, 4], iv)
    assert (rows[:, 2].view(np.int32) == iy).all()
    assert same(rows[:, 3], er_math(L, 0, (iy.astype(np.float32) / fh) * PIF)) and same(rows[:, 5], er_math(L, 0, (y.astype(np.float32) / fh) * PIF))
    # the edges by value: column 0 looks along phi - pi = -pi, row 0 is the pole (sine exactly 0: hdri_pdf divides by it, inf)
    r = rows.view(np.float32)
    assert r[0, 0] == -1.0 and r[0, 1] == 0.0 and r[0, 3] == 0.0 and r[0, 5] == 0.0
    with np.errstate(divide="ignore"):
        assert np.isinf(np.float32(1.0) / (np.float32(2.0) * PIF * r[0, 3]))
    assert cols.view(np.float32)[0, 0] == -1.0 and cols[0, 2] == 0 and cols[w - 1, 2].view(np.int32) in (w - 1, w - 2)
    assert 0 <= rows[h - 1, 2].view(np.int32) <= h - 1


def test_host_twin_refuses_bad_arguments():
    lib = abi.load()
    assert lib.er_debug_hdri_trig_host(-1, 1, None, None) == abi.ER_ERR_INVALID_ARG
    assert lib.er_debug_hdri_trig_host(2, 0, None, None) == abi.ER_ERR_INVALID_ARG
    assert lib.er_debug_hdri_trig_host(0, 0, None, None) == abi.ER_OK
