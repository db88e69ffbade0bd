"""The host side of msm_fr_inverse*, msm_fr_scan* and msm_fr_tensor* (include/msm.h): the symbols, every
refusal that precedes device work, csrc/fr.cuh's fr_inv through its hook against Python integers, and the
scan's launch plan (spans partition [0, m) in order, none is empty, at most `cap` of them).  No GPU needed."""
import ctypes
import random

import numpy as np
import pytest

import msm_amd as M

R = M.FR_MODULUS
RR = 1 << 256
R_INV = pow(RR, -1, R)
SUM, EXCL = M.MSM_FR_SCAN_SUM, M.MSM_FR_SCAN_EXCLUSIVE

ENTRIES = ("msm_fr_inverse", "msm_fr_inverse_device", "msm_fr_scan", "msm_fr_scan_device", "msm_fr_tensor",
           "msm_fr_tensor_device")
HOOKS = ("msm_test_fr_inv", "msm_test_fr_scan_constants", "msm_test_fr_scan_plan", "msm_test_fr_scan_device",
         "msm_test_fr_inverse_device")


def _u32(vals):
    return np.ascontiguousarray(M.scalars_to_wire(vals))


A2 = _u32([3, 4])
C1 = _u32([5])
OUT = np.zeros((4, 8), np.uint32)
SCALAR_FLAGS = [M.MSM_FLAG_SCALAR_BITS, M.MSM_FLAG_SCALAR_TYPE, M.MSM_FLAG_SCALAR_FIELD, M.MSM_FLAG_DEVICES,
                M.MSM_FLAG_WINDOWS]


# ---- ABI ------------------------------------------------------------------------------------------------
def test_entries_and_hooks_are_exported():
    L = M.load()
    for name in ENTRIES + HOOKS:
        assert isinstance(getattr(L, name), ctypes._CFuncPtr), name
    for name in ("fr_inverse", "fr_cumprod", "fr_cumsum", "fr_tensor"):
        assert name in M.__all__ and callable(getattr(M, name))
    assert (SUM, EXCL) == (1, 2)


def _inverse(a=A2, c=None, m=2, fi=0, fo=0, opts=None, out=OUT, dev=False):
    L = M.load()
    args = (None if a is None else a.ctypes.data, None if c is None else c.ctypes.data, m, fi, fo, opts)
    o = None if out is None else out.ctypes.data
    return L.msm_fr_inverse_device(*args, None, o) if dev else L.msm_fr_inverse(*args, o)


def _scan(a=A2, c=None, m=2, flags=0, fi=0, fo=0, opts=None, out=OUT, dev=False):
    L = M.load()
    args = (None if a is None else a.ctypes.data, None if c is None else c.ctypes.data, m, flags, fi, fo, opts)
    o = None if out is None else out.ctypes.data
    return L.msm_fr_scan_device(*args, None, o) if dev else L.msm_fr_scan(*args, o)


def _tensor(lo=A2, hi=A2, k=2, c=None, fo=0, opts=None, out=OUT, dev=False):
    L = M.load()
    args = (None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data, k,
            None if c is None else c.ctypes.data, fo, opts)
    o = None if out is None else out.ctypes.data
    return L.msm_fr_tensor_device(*args, None, o) if dev else L.msm_fr_tensor(*args, o)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_refusals_before_device_work(dev):
    for kw in (dict(fi=2), dict(fo=2), dict(fi=0xffffffff), dict(a=None), dict(out=None), dict(m=1 << 32)):
        assert _inverse(dev=dev, **kw) == -1, kw
        assert _scan(dev=dev, **kw) == -1, kw
        assert _scan(dev=dev, flags=SUM | EXCL, **kw) == -1, kw
    for flags in (4, 8, 1 << 31, SUM | 4, 0xffffffff):  # a flag word refuses unknown bits
        assert _scan(dev=dev, flags=flags) == -1, flags
    assert _scan(dev=dev, flags=SUM, c=C1) == -1          # a sum has no first factor
    assert _scan(dev=dev, flags=SUM | EXCL, c=C1) == -1
    assert _scan(dev=dev, flags=SUM, c=C1, m=0) == -1     # ... whatever the length
    for kw in (dict(k=32), dict(k=0xffffffff), dict(fo=2), dict(lo=None), dict(hi=None), dict(out=None)):
        assert _tensor(dev=dev, **kw) == -1, kw
    assert _tensor(dev=dev, lo=None, hi=None, k=0, out=None) == -1  # k = 0 still stores one element


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("flag", SCALAR_FLAGS)
def test_option_flags_fr_opts_ok_rejects(flag, dev):
    o = M.MsmOpts(0, 0, -1, flag)
    o.scalar_bits = 64
    assert _inverse(dev=dev, opts=ctypes.byref(o)) == -1
    assert _scan(dev=dev, opts=ctypes.byref(o)) == -1
    assert _tensor(dev=dev, opts=ctypes.byref(o)) == -1
    assert _inverse(dev=dev, opts=ctypes.byref(o), m=0) == -1  # the options are checked first


def test_device_pointer_rules_are_decided_from_the_values():
    L = M.load()
    base = 1 << 20

    def inv(a, out, m=4):
        return L.msm_fr_inverse_device(a, None, m, 0, 0, None, None, out)

    def scan(a, out, m=4, flags=0):
        return L.msm_fr_scan_device(a, None, m, flags, 0, 0, None, None, out)

    for call in (inv, scan, lambda a, out: scan(a, out, flags=SUM)):
        assert call(base + 4, base + 4096) == -1    # a misaligned
        assert call(base, base + 4096 + 8) == -1    # out misaligned
        assert call(base, base + 32) == -1          # out one element into a
        assert call(base, base - 32) == -1          # out ending inside a
        assert call(base, base + 96) == -1          # a's last element is out's first
    assert L.msm_fr_tensor_device(A2.ctypes.data, A2.ctypes.data, 2, None, 0, None, None, base + 4) == -1


def test_host_mont_inputs_at_or_above_r_are_refused_before_any_upload():
    good = M.scalars_to_wide([5, R - 1], "fr_mont").view(np.uint32).reshape(-1, 8)
    for bad_value in (R, R + 1, RR - 1):
        bad = good.copy()
        bad[1] = np.frombuffer(bad_value.to_bytes(32, "little"), dtype="<u4")
        assert _inverse(a=bad, fi=1) == -1
        assert _scan(a=bad, fi=1) == -1
        assert _scan(a=bad, fi=1, flags=SUM) == -1


def test_zero_length_calls_return_ok_without_a_gpu():
    for dev in (False, True):
        assert _inverse(m=0, dev=dev) == 0
        assert _inverse(a=None, out=None, c=C1, m=0, dev=dev) == 0
        for flags in (0, SUM, EXCL, SUM | EXCL):
            assert _scan(m=0, flags=flags, dev=dev) == 0
            assert _scan(a=None, out=None, m=0, flags=flags, dev=dev) == 0
    assert not OUT.any()
    empty = np.zeros((0, 8), np.uint32)
    assert M.fr_inverse(empty).shape == (0, 8)
    assert M.fr_cumprod(empty, first=3).shape == (0, 8)
    assert M.fr_cumsum(empty, exclusive=True).shape == (0, 8)


def test_python_argument_rules():
    with pytest.raises(ValueError):
        M.fr_inverse([1], form="mont")
    with pytest.raises(ValueError):
        M.fr_tensor([(1, 2)], out_form="mont")
    with pytest.raises(M.MsmError):
        M.fr_tensor([(1, 2)] * 32)
    with pytest.raises(ValueError):
        M.fr_cumsum([1, 2], out=np.zeros((2, 8), np.uint32))


# ---- fr_inv -----------------------------------------------------------------------------------------------
def _inv_values():
    rnd = random.Random(20250607)
    return [0, 1, 2, R - 1, R - 2, RR % R] + [rnd.randrange(R) for _ in range(2000)]


def test_fr_inv_against_python_integers():
    """The hook takes and gives Montgomery form: for the value v the memory is v R, and the result v^-1 R."""
    vals = _inv_values()
    got = M._test_fr_inv([v * RR % R for v in vals])
    assert got == [pow(v, -1, R) * RR % R if v else 0 for v in vals]
    # and read the other way, the memory itself as a value: a -> a^-1 R^2 (the inverse of a R^-1, times R)
    got = M._test_fr_inv(vals)
    assert got == [pow(a, -1, R) * RR * RR % R if a else 0 for a in vals]
    assert all(v < R for v in got)


def test_fr_inv_times_its_argument_is_one():
    vals = [a for a in _inv_values() if a]
    inv = M._test_fr_inv(vals)
    assert M._test_fr_op("mont_mul", inv, vals) == [RR % R] * len(vals)  # 1 in Montgomery form
    assert M._test_fr_op("mont_mul", vals, inv) == [RR % R] * len(vals)


def test_fr_inv_refuses_a_value_at_or_above_r():
    for bad in (R, R + 1, RR - 1):
        with pytest.raises(M.MsmError) as e:
            M._test_fr_inv([1, bad])
        assert e.value.code == -1
    assert M._test_fr_inv([]) == []


def test_constants():
    c = M._test_fr_scan_constants()
    t = M._test_fr_constants()
    assert c["e"] >= 1 and c["tile"] == c["e"] * t["threads"]
    assert c["scan_cap"] == 1024 and c["scan_cap"] % t["threads"] == 0
    assert c["inverse_cap"] == t["combine_cap"]
    assert c["tensor_max_k"] == 31 and t["pow_steps"] == 16
    # the chain of one inversion: a fixed 4-bit window over the 63 nibbles of r - 2
    nibbles = [((R - 2) >> (4 * i)) & 15 for i in range(63)]
    assert (R - 2) >> 252 == 0 and nibbles[62] != 0
    assert c["inv_squarings"] == 4 * 62 + 1
    assert c["inv_products"] == 13 + sum(1 for w in nibbles[:62] if w)


# ---- the scan's plan ----------------------------------------------------------------------------------------
def _plan_sizes(tile, cap):
    return [1, tile - 1, tile, tile + 1, cap * tile - 1, cap * tile, cap * tile + 1, (cap + 1) * tile + 1,
            2 * cap * tile + 1, (1 << 32) - 1]


def _check_plan(m, cap):
    c = M._test_fr_scan_constants()
    pl = M._test_fr_scan_plan(m, cap)
    tile = pl["tile"]
    assert (pl["e"], tile) == (c["e"], c["tile"])
    ntiles = -(-m // tile)
    tps, grid = pl["tiles_per_span"], pl["grid"]
    assert tps == -(-ntiles // min(ntiles, cap)) and grid == -(-ntiles // tps)
    assert 1 <= grid <= cap
    span = tps * tile
    # span b is [b span, min((b + 1) span, m)): in order, adjoining, the first at 0, the last ending at m ...
    assert (grid - 1) * span < m <= grid * span       # ... and none empty: the last one starts below m
    # the tiles of the last span: at least one, the last of them ragged or whole
    last = m - (grid - 1) * span
    assert 1 <= -(-last // tile) <= tps


def test_scan_plan_sweep():
    c = M._test_fr_scan_constants()
    tile, cap = c["tile"], c["scan_cap"]
    for cp in (cap, 1, 2, 3):
        for m in _plan_sizes(tile, cp):
            if m < 1 << 32:
                _check_plan(m, cp)
    rnd = random.Random(77)
    for _ in range(500):
        m = rnd.randrange(1, 1 << rnd.randrange(1, 33))
        _check_plan(m, rnd.choice((cap, cap, 1, 2, 3, rnd.randrange(1, cap + 1))))
    assert M._test_fr_scan_plan(0, cap)["grid"] == 0


def test_scan_plan_spans_listed_at_small_sizes():
    """The spans written out: a partition of [0, m) in order."""
    c = M._test_fr_scan_constants()
    tile = c["tile"]
    for cap in (1, 2, 3):
        for m in _plan_sizes(tile, cap)[:-1]:
            pl = M._test_fr_scan_plan(m, cap)
            span = pl["tiles_per_span"] * tile
            spans = [(b * span, min((b + 1) * span, m)) for b in range(pl["grid"])]
            assert spans[0][0] == 0 and spans[-1][1] == m
            assert all(lo < hi for lo, hi in spans)
            assert all(spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1))


def test_scan_plan_refuses_bad_arguments():
    L = M.load()
    out = (ctypes.c_uint32 * 4)()
    assert L.msm_test_fr_scan_plan(5, 0, out) == -1
    assert L.msm_test_fr_scan_plan(1 << 32, 4, out) == -1
    assert L.msm_test_fr_scan_plan(5, 4, None) == -1
    assert L.msm_test_fr_scan_constants(None) == -1
