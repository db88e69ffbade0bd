"""Resident prepared bases, the host-only part: the fold geometry of shifted levels
(msm_test_bases_plan against a Python restatement of DESIGN.md §9's rule, tests/_bases_model.py),
the carry argument behind it, and the argument checks of the msm_bases_* entries.  No GPU needed."""
import ctypes
import random

import numpy as np
import pytest

import msm_amd as M
from _bases_model import cut, fold, geometry, recode
from oracle import oracle as O

WIDTHS = range(4, 21)
LEVELS = range(1, 9)


@pytest.mark.parametrize("c", WIDTHS)
def test_plan_matches_the_rule(c):
    for k in LEVELS:
        got = M._test_bases_plan(1000, k, c)
        Wc, S = fold(c, k)
        assert got == {"c": c, "windows": Wc, "chunk_bits": S, "points": 1000 * k}, (c, k)
        assert k * S >= 256
        if k == 1:
            assert Wc == M.window_count(c)
        else:
            _, off = geometry(c)
            assert S == off[Wc] - 1 and Wc < M.window_count(c)
            assert Wc == 1 or k * (off[Wc - 1] - 1) < 256  # the smallest such window count


def test_plan_examples():
    # the worked examples of DESIGN.md §9
    for c, k, Wc, S in ((16, 2, 9, 143), (15, 2, 9, 134), (15, 4, 5, 74), (13, 8, 3, 38)):
        p = M._test_bases_plan(1 << 18, k, c)
        assert (p["windows"], p["chunk_bits"]) == (Wc, S)
    assert M.window_count(16) == 17  # unfolded


def test_plan_auto_width_and_bad_arguments():
    for n in (1, 1 << 16, 1 << 20):
        for k in (2, 4):
            p = M._test_bases_plan(n, k, 0)
            assert 4 <= p["c"] <= 16 and (p["windows"], p["chunk_bits"]) == fold(p["c"], k)
    out = np.zeros(4, np.uint32)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    L = M.load()
    assert L.msm_test_bases_plan(10, 0, 16, op) == -1
    assert L.msm_test_bases_plan(10, 9, 16, op) == -1
    assert L.msm_test_bases_plan(10, 2, 3, op) == -2
    assert L.msm_test_bases_plan(10, 2, 21, op) == -2


@pytest.mark.parametrize("c", WIDTHS)
def test_no_digit_at_or_above_the_fold(c):
    """A chunk keeps one bit less than windows [0, Wc) hold, so even the largest chunk, with every
    carry, leaves nothing for window Wc: no carry out, no bits above."""
    for k in range(2, 9):
        Wc, S = fold(c, k)
        for v in ((1 << S) - 1, 1 << (S - 1), (1 << (S - 1)) + 1, (1 << (S - 1)) - 1):
            digits, carry, rest = recode(v, c, Wc)
            assert carry == 0 and rest == 0, (c, k, v)
            bits, off = geometry(c)
            assert sum(d << off[w] for w, d in enumerate(digits)) == v
            assert all(-(1 << (bits[w] - 1)) < d <= 1 << (bits[w] - 1) for w, d in enumerate(digits))


def test_chunks_reassemble_the_scalar():
    rnd = random.Random(5)
    scalars = [(1 << 256) - 1, O.R_ORDER - 1, 0, 1] + [rnd.getrandbits(256) for _ in range(50)]
    for c in WIDTHS:
        for k in range(2, 9):
            _, S = fold(c, k)
            for s in scalars:
                v = cut(s, k, S)
                assert all(x < 1 << S for x in v)
                assert sum(x << (j * S) for j, x in enumerate(v)) == s


# ---- argument checks of the entries: the same answers with and without a device ------------------
def _opts(**kw):
    o = M.MsmOpts()
    for k, v in kw.items():
        setattr(o, k, v)
    return ctypes.byref(o)


def _create(pts, n, opts, levels):
    h = ctypes.c_void_p()
    rc = M.load().msm_bases_create(pts.ctypes.data_as(ctypes.c_void_p), n, opts, levels, ctypes.byref(h))
    return rc, h.value


def test_entry_argument_checks():
    L = M.load()
    have_gpu = L.msm_init() == 0
    pts = O.gen_points(4, k0=3, step=2)
    sc = np.zeros((4, 8), np.uint32)
    out = np.zeros(16, np.uint32)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    scp = sc.ctypes.data_as(ctypes.c_void_p)
    # rejected before any device work, device or not
    assert _create(pts, 4, None, 9) == (-1, None)
    assert _create(pts, 4, _opts(flags=M.MSM_FLAG_DEVICES), 1) == (-1, None)
    assert _create(pts, 4, _opts(flags=M.MSM_FLAG_WINDOWS, window_bits=16, window_lo=0, window_hi=2), 1) == (-1, None)
    assert L.msm_bases_create(None, 4, None, 1, ctypes.byref(ctypes.c_void_p())) == -1
    assert L.msm_bases_create(pts.ctypes.data_as(ctypes.c_void_p), 4, None, 1, None) == -1
    # null and unknown handles
    for h in (None, 12345):
        assert L.msm_bases_compute(h, scp, None, op) == -1
        assert L.msm_bases_compute_device(h, scp, None, None, op) == -1
        assert L.msm_bases_compute_many(h, scp, 1, None, op) == -1
        assert L.msm_bases_compute_many_device(h, scp, 1, None, None, op) == -1
        assert L.msm_bases_info(h, ctypes.byref(M.BasesInfo())) == -1
        assert L.msm_bases_destroy(h) == -1
    # a well-formed creation needs a device
    rc, h = _create(pts, 4, _opts(window_bits=13, device=-1), 2)
    if not have_gpu:
        assert (rc, h) == (-6, None)
        with pytest.raises(M.MsmError) as e:
            M.Bases.from_wire(pts)
        assert e.value.code == -6
        return
    assert rc == 0 and h
    try:
        # the two rejected flags and a mismatched width at compute
        assert L.msm_bases_compute(h, scp, _opts(flags=M.MSM_FLAG_DEVICES, device=-1), op) == -1
        assert L.msm_bases_compute(h, scp, _opts(flags=M.MSM_FLAG_WINDOWS, window_bits=13, window_hi=2, device=-1),
                                   op) == -1
        assert L.msm_bases_compute(h, scp, _opts(window_bits=14, device=-1), op) == -1
        assert L.msm_bases_compute(h, scp, _opts(window_bits=13, device=-1), op) == 0
        assert L.msm_bases_compute(h, None, None, op) == -1
    finally:
        assert L.msm_bases_destroy(h) == 0
    assert L.msm_bases_destroy(h) == -1
