"""Narrow-scalar MSMs on a resident-bases handle, the host-only part (include/msm.h
MSM_FLAG_SCALAR_BITS): the launch geometry of a b-bit scalar (msm_test_narrow_plan) against the rule
restated in _narrow_model, the signed recode over it, the entries that refuse the flag, and the
narrow wire format.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import msm_amd as M
from _narrow_model import auto_width, edge_scalars, geometry, offsets, recode

WIDTHS = range(4, 21)
N = 4097


@pytest.mark.parametrize("c", WIDTHS)
def test_plan_is_balanced_over_the_scalars_own_bits(c):
    for b in range(1, 254):
        p = M._test_narrow_plan(N, b, c)
        widths = [p["q"] + 1] * p["nhi"] + [p["q"]] * (p["windows"] - p["nhi"])
        assert p["nhi"] < p["windows"], (b, c)
        assert sum(widths) == max(b + 1, 4), (b, c)
        assert max(widths) - min(widths) <= 1, (b, c)
        assert max(widths) == p["c"] <= c, (b, c)
        assert p["words"] == -(-b // 32), (b, c)
        assert widths == geometry(b, c), (b, c)
        assert p["packed"] == 1, (b, c)


@pytest.mark.parametrize("c", WIDTHS)
def test_254_bits_and_more_are_the_plain_plan(c):
    plain = M.launch_plan(N, window_size=c)
    for b in (254, 255, 256):
        p = M._test_narrow_plan(N, b, c)
        assert (p["c"], p["windows"], p["words"]) == (plain["c"], plain["windows"], 8), (b, c)
        assert p["windows"] == M.window_count(c)


def test_auto_width_is_the_sizes_usual_choice_or_17_for_dense_buckets():
    for n in (1, 300, N, 1 << 16, 1 << 18, 1 << 20):
        c0 = M.get_best_window_size(n)
        for b in range(1, 254):
            c = auto_width(n, b, c0)
            assert M._test_narrow_plan(n, b, 0) == M._test_narrow_plan(n, b, c), (n, b)
        assert M._test_narrow_plan(n, 256, 0)["c"] == M.launch_plan(n)["c"]
    # the measured rows (profiles/bases_narrow_sweep.jsonl): one 17-bit window for 16-bit scalars,
    # 17 + 16 bits for 32-bit ones, and the usual width where the buckets are not dense
    p = M._test_narrow_plan(1 << 20, 16, 0)
    assert (p["c"], p["windows"]) == (17, 1)
    p = M._test_narrow_plan(1 << 20, 32, 0)
    assert (p["c"], p["windows"], p["nhi"]) == (17, 2, 1)
    assert M._test_narrow_plan(1 << 20, 253, 0) == M._test_narrow_plan(1 << 20, 253, 16)
    assert M._test_narrow_plan(1 << 16, 128, 0) == M._test_narrow_plan(1 << 16, 128, 16)
    assert M._test_narrow_plan(1 << 20, 16, 16)["windows"] == 2  # an explicit width is kept


def test_plan_argument_errors():
    for b in (0, 257, 1 << 31):
        with pytest.raises(M.MsmError) as e:
            M._test_narrow_plan(N, b, 16)
        assert e.value.code == -1, b
    for c in (3, 21):
        with pytest.raises(M.MsmError) as e:
            M._test_narrow_plan(N, 64, c)
        assert e.value.code == -2, c


@pytest.mark.parametrize("c", WIDTHS)
def test_signed_recode_reproduces_the_scalar_with_no_carry_out(c):
    for b in range(1, 254):
        widths = geometry(b, c)
        offs = offsets(widths)
        for s in edge_scalars(b, c):
            digits, carry = recode(s, widths)
            assert carry == 0, (b, c, s)
            assert sum(d << o for d, o in zip(digits, offs)) == s, (b, c, s)
            assert all(-(1 << (w - 1)) < d <= 1 << (w - 1) for d, w in zip(digits, widths)), (b, c, s)


def test_edge_scalars_reach_every_windows_carry_edge():
    widths = geometry(64, 16)
    assert widths == [13] * 5
    es = edge_scalars(64, 16)
    assert (1 << 64) - 1 in es and 1 << 63 in es
    for off in offsets(widths)[:-1]:
        assert {4095 << off, 4096 << off, 4097 << off} <= set(es)


# ---- the flag belongs to msm_bases_compute* ---------------------------------------------------------
def _flagged(bits=64):
    o = M.MsmOpts(0, 0, -1, M.MSM_FLAG_SCALAR_BITS)
    o.scalar_bits = bits
    return o


def test_other_entries_refuse_the_flag_before_any_device_work():
    L = M.load()
    n = 4
    pts = np.ascontiguousarray(M.gen_points(n))
    sc = np.ascontiguousarray(M.gen_scalars(n))
    out = np.zeros(16, np.uint32)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    o = _flagged()
    pp = (ctypes.c_void_p * 1)(pts.ctypes.data)
    ss = (ctypes.c_void_p * 1)(sc.ctypes.data)
    assert L.msm_compute(pts.ctypes.data, sc.ctypes.data, n, ctypes.byref(o), op) == -1
    # (host addresses: the flag is refused before either pointer is looked at)
    assert L.msm_compute_device(pts.ctypes.data, sc.ctypes.data, n, ctypes.byref(o), None, op) == -1
    assert L.msm_compute_shared(pts.ctypes.data, ctypes.cast(ss, ctypes.c_void_p), n, 1, ctypes.byref(o), op) == -1
    assert L.msm_compute_many(ctypes.cast(pp, ctypes.c_void_p), ctypes.cast(ss, ctypes.c_void_p), n, 1,
                              ctypes.byref(o), op) == -1
    assert L.msm_compute_cocompute(pts.ctypes.data, sc.ctypes.data, n, ctypes.byref(o), 0.5, 1, op) == -1
    assert L.msm_compute_cocompute(pts.ctypes.data, sc.ctypes.data, n, ctypes.byref(o), 0.0, 1, op) == -1
    h = ctypes.c_void_p()
    assert L.msm_bases_create(pts.ctypes.data, n, ctypes.byref(o), 1, ctypes.byref(h)) == -1
    assert not h.value
    assert L.msm_bases_create_device(pts.ctypes.data, n, ctypes.byref(o), 1, None, ctypes.byref(h)) == -1
    part = np.zeros(32, np.uint32)
    assert L.msm_compute_partial(pts.ctypes.data, sc.ctypes.data, n, ctypes.byref(o),
                                 part.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) == -1


def test_opts_carry_the_width():
    o = M._opts(16, scalar_bits=64)._obj
    assert o.flags & M.MSM_FLAG_SCALAR_BITS and o.scalar_bits == 64
    assert M.MsmOpts.scalar_bits.offset == 28 and ctypes.sizeof(M.MsmOpts) == 40
    assert not M._opts(16)._obj.flags & M.MSM_FLAG_SCALAR_BITS
    assert M.MSM_FLAG_SCALAR_BITS == 16


# ---- the wire format --------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 8, 31, 32, 33, 64, 65, 128, 224, 225, 253, 256])
def test_scalars_to_wire_round_trips_and_refuses_wide_values(b):
    vals = [0, 1, (1 << b) - 1, 1 << (b - 1), 0x1234567 % (1 << b)]
    w = M.scalars_to_wire(vals, scalar_bits=b)
    words = -(-b // 32)
    assert w.shape == (len(vals), words) and w.dtype == np.uint32
    assert [M.wire_to_int(r) for r in w] == vals
    # zero-extended to 8 words it is the 8-word format of the same values
    full = np.zeros((len(vals), 8), np.uint32)
    full[:, 8 - words:] = w
    assert (full == M.scalars_to_wire(vals)).all()
    # arrays pass through in the narrow shape
    assert M.scalars_to_wire(w.reshape(-1), scalar_bits=b).shape == (len(vals), words)
    assert M.scalars_to_wire([], scalar_bits=b).shape == (0, words)
    for bad in (1 << b, (1 << b) + 5, -1):
        with pytest.raises(ValueError):
            M.scalars_to_wire([1, bad], scalar_bits=b)
