"""CPU tests of the fixed-base tables (include/msm.h msm_fixed_*): the exported symbols, the evaluation's
signed digit function run on the host (msm_test_fixed_digits calls the kernel's own fixed_digit), the
table's shape (msm_test_fixed_plan: the creation's own fixed_plan) and the argument rules that return
before any device work."""
import ctypes
import random
import subprocess

import numpy as np
import pytest

import msm_amd as M

ENTRIES = ["msm_fixed_create", "msm_fixed_destroy", "msm_fixed_info", "msm_fixed_mul", "msm_fixed_mul_device",
           "msm_fixed_mul_create", "msm_fixed_mul_create_device"]
HOOKS = ["msm_test_fixed_digits", "msm_test_fixed_plan", "msm_test_fixed_bases"]
WIDTHS = list(range(2, 17))


def _bits(w):
    return sorted({b for b in (1, 2, w - 1, w, w + 1, 31, 32, 33, 64, 128, 253, 254, 255, 256) if b >= 1})


def test_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", M.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ENTRIES + HOOKS:
        assert name in exported, name
        assert hasattr(M.load(), name)


@pytest.mark.parametrize("w", WIDTHS)
def test_digits_sum_to_the_integer(w):
    half = 1 << (w - 1)
    for b in _bits(w):
        rnd = random.Random(1000 * w + b)
        values = [0, 1, half, half + 1, (1 << w) - 1, (1 << b) - 1]  # 2^b - 1: the carry ripples into the top window
        values += [1 << k for k in range(b)] + [rnd.getrandbits(b) for _ in range(200)]
        wn = -(-(b + 1) // w)
        for v in values:
            v &= (1 << b) - 1
            d, carry = M._test_fixed_digits(v, b, w)
            assert len(d) == wn, (w, b)  # the trip count depends on (b, w) alone
            assert carry == 0, (w, b, hex(v))  # nothing carries out of the top window
            assert all(-(half - 1) <= dj <= half for dj in d), (w, b, hex(v), d)
            assert sum(dj << (w * j) for j, dj in enumerate(d)) == v, (w, b, hex(v))


@pytest.mark.parametrize("w", WIDTHS)
def test_plan_is_the_stated_formula(w):
    for b in _bits(w) + [0]:
        for k in range(1, 9):
            wn = -(-((b or 256) + 1) // w)
            records = k * wn << (w - 1)
            if records * 128 > 256 << 20:
                with pytest.raises(M.MsmError) as e:
                    M._test_fixed_plan(k, w, b)
                assert e.value.code == -1
                continue
            assert M._test_fixed_plan(k, w, b) == {"window_bits": w, "scalar_bits": b or 256, "windows": wn,
                                                   "records": records, "bytes": records * 128}


def test_plan_limits():
    # auto width is 12: 22 windows of 2048 records, 5.5 MiB per base at 256 bits; 528 KiB at w = 8
    assert M._test_fixed_plan(1) == {"window_bits": 12, "scalar_bits": 256, "windows": 22, "records": 22 * 2048,
                                     "bytes": 5632 << 10}
    assert M._test_fixed_plan(1, 8)["bytes"] == 528 << 10
    # 17 windows of 2^15 records are 68 MiB per base at w = 16: three bases fit 256 MiB, four do not
    assert M._test_fixed_plan(3, 16, 256)["bytes"] == 3 * 68 << 20
    for k, w, b in ((4, 16, 256), (0, 8, 256), (9, 8, 256), (1, 1, 256), (1, 17, 256), (1, 8, 257), (9, 2, 1)):
        with pytest.raises(M.MsmError) as e:
            M._test_fixed_plan(k, w, b)
        assert e.value.code == -1, (k, w, b)


def test_digits_hook_argument_rules():
    L = M.load()
    sc = np.zeros(8, np.uint32)
    dg = np.zeros(257, np.int32)
    cnt, carry = ctypes.c_uint32(), ctypes.c_uint32()
    p = sc.ctypes.data_as(ctypes.c_void_p)
    dp = dg.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert L.msm_test_fixed_digits(p, 8, 256, 8, dp, ctypes.byref(cnt), ctypes.byref(carry)) == 0
    assert cnt.value == 33
    for sw, b, w in ((8, 0, 8), (8, 257, 8), (7, 256, 8), (8, 256, 1), (8, 256, 17)):
        assert L.msm_test_fixed_digits(p, sw, b, w, dp, ctypes.byref(cnt), ctypes.byref(carry)) == -1
    assert L.msm_test_fixed_digits(None, 8, 256, 8, dp, ctypes.byref(cnt), ctypes.byref(carry)) == -1


def test_argument_rules_return_before_device_work():
    L = M.load()
    vp = ctypes.c_void_p
    sc = np.zeros((4, 8), np.uint32)
    pts = np.zeros((4, 32), np.uint32)
    s, p = sc.ctypes.data_as(vp), pts.ctypes.data_as(vp)
    inf = M.FixedInfo()
    # a null table, and a token no creation handed out
    for t in (None, vp(0x7FFFFFF0)):
        h = vp(0xDEAD)
        assert L.msm_fixed_mul(t, s, 4, None, p) == -1
        assert L.msm_fixed_mul_device(t, s, 4, None, None, p) == -1
        assert L.msm_fixed_mul_create(t, s, 4, None, 1, ctypes.byref(h)) == -1
        assert h.value is None  # the create entries clear *out
        h = vp(0xDEAD)
        assert L.msm_fixed_mul_create_device(t, s, 4, None, 1, None, ctypes.byref(h)) == -1
        assert h.value is None
        assert L.msm_fixed_info(t, ctypes.byref(inf)) == -1
        assert L.msm_fixed_destroy(t) == -1
        # ... and no handle to build a table from
        h = vp(0xDEAD)
        assert L.msm_fixed_create(t, None, 8, 256, None, ctypes.byref(h)) == -1
        assert h.value is None
    assert L.msm_fixed_create(vp(1), None, 8, 256, None, None) == -1
    assert L.msm_fixed_mul_create(vp(1), s, 4, None, 1, None) == -1
    assert L.msm_fixed_mul_create_device(vp(1), s, 4, None, 1, None, None) == -1
    # the flags the entries do not take
    for opts in (M._opts(None, scalar_type="u32"), M._opts(None, scalar_type="u256"), M._opts(None, devices=[0]),
                 M._opts(13, windows=(0, 2)), M._opts(13, windows=(0, 2, 2))):
        assert L.msm_fixed_mul(vp(1), s, 4, opts, p) == -1
        h = vp(0xDEAD)
        assert L.msm_fixed_create(vp(1), None, 8, 256, opts, ctypes.byref(h)) == -1
