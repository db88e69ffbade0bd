"""The dense-bucket accumulation of narrow-scalar launches, the host-only part: which launches are
dense, their entries per unit lane and the unit kernel's grid bound (msm_test_dense_plan) against
the rule restated in _dense_model, the bound as a property of any bucket sizes, and the plans of the
8-word launches, which the path leaves alone.  No GPU needed."""
import numpy as np
import pytest

import msm_amd as M
from _dense_model import (DENSE_K, DENSE_MAX_KEYS, DENSE_MIN, dense_plan, entries_per_lane, pipelined_window,
                          segment_map, size_vectors, unit_bound)

SIZES = (1, 127 * 8, 128 * 8, 4097, 1 << 16, 1 << 18, 1 << 20)
WIDTHS = (0,) + tuple(range(4, 21))


def _usual_width(n, pipelined):
    best = M.get_best_window_size(n)
    return pipelined_window(n, best) if pipelined else best


@pytest.mark.parametrize("nm,pipelined", [(1, False), (1, True), (2, True), (4, True)])
@pytest.mark.parametrize("n", SIZES)
def test_plan_matches_the_model(n, nm, pipelined):
    c0 = _usual_width(n, pipelined)
    seen = set()
    for c in WIDTHS:
        for b in range(1, 254):
            got = M._test_dense_plan(n, nm, pipelined, b, c)
            want = dense_plan(n, nm, b, c, c0)
            assert {k: got[k] for k in want} == want, (n, nm, b, c)
            if got["dense"]:
                assert got["K"] == DENSE_K, (n, nm, b, c)
                assert got["E"] % 4 == 0 and 4 <= got["E"] <= 64
                assert got["nkeys"] <= DENSE_MAX_KEYS
            seen.add(got["dense"])
    # (the narrowest widest window is 3 bits, 4 buckets: T = 5 or 9 bits at c = 4)
    assert seen == ({0, 1} if n >= DENSE_MIN * 4 else {0}), n


def test_the_threshold_sits_at_dense_min_entries_per_bucket():
    # b = 1..2 is one 4-bit window of 8 buckets: 127 entries per bucket is not dense, 128 is
    for b in (1, 2):
        assert M._test_dense_plan(127 * 8 + 7, scalar_bits=b)["dense"] == 0
        assert M._test_dense_plan(128 * 8, scalar_bits=b)["dense"] == 1
    # bytes in one 9-bit window of 256 buckets
    assert M._test_dense_plan((DENSE_MIN << 8) - 1, scalar_bits=8)["dense"] == 0
    assert M._test_dense_plan(DENSE_MIN << 8, scalar_bits=8)["dense"] == 1
    # an explicit width is kept and served: b = 16 at c = 16 is 9 + 8 bits
    p = M._test_dense_plan(1 << 20, scalar_bits=16, window_size=16)
    assert (p["dense"], p["nkeys"]) == (1, 2 * 256)
    # the auto width's one 17-bit window for 16-bit scalars is not dense, nor is any 8-word launch
    assert M._test_dense_plan(1 << 20, scalar_bits=16)["dense"] == 0
    for b in (254, 255, 256):
        assert M._test_dense_plan(1 << 20, scalar_bits=b)["dense"] == 0
    # a key space past the one-workgroup segment map takes the existing path
    p = M._test_dense_plan(1 << 24, scalar_bits=253, window_size=14)
    assert p["nkeys"] > DENSE_MAX_KEYS and p["dense"] == 0


def test_entries_per_lane_fill_whole_rounds():
    # 2^20 bytes: 4,096 + 256 units at E = 4 are more than the 4,096 resident waves, E = 8 fits
    p = M._test_dense_plan(1 << 20, scalar_bits=8)
    assert (p["E"], p["units"]) == (8, (1 << 20) // 512 + 256)
    assert M._test_dense_plan(1 << 18, scalar_bits=8)["E"] == 4
    # past one round at E = 64: whole rounds
    m_max, nkeys = 1 << 30, 8
    E = entries_per_lane(m_max, nkeys)
    rounds = -(-unit_bound(m_max, nkeys, 64) // 4096)
    assert rounds > 1 and unit_bound(m_max, nkeys, E) <= rounds * 4096
    assert E == 4 or unit_bound(m_max, nkeys, E - 4) > rounds * 4096


SHAPES = [(4096, 1, 1, 0), (4096, 1, 8, 4), (4097, 4, 2, 0), (1 << 16, 1, 16, 16), (1 << 18, 1, 8, 0),
          (1 << 20, 2, 8, 0), (1 << 20, 1, 12, 0)]


@pytest.mark.parametrize("n,nm,b,c", SHAPES)
def test_grid_bound_holds_for_any_bucket_sizes(n, nm, b, c):
    p = M._test_dense_plan(n, nm, nm > 1, b, c)
    assert p["dense"] == 1
    S, nkeys = 64 * p["E"], p["nkeys"]
    m_max = n * (nkeys >> (M._test_narrow_plan(n, b, c)["c"] - 1))  # W * n
    for sizes in size_vectors(nkeys, m_max, S, seed=b):
        m = int(sizes.sum())
        assert m <= m_max
        seg_base, unit_key = segment_map(sizes, S)
        live = int(seg_base[-1])
        assert live == len(unit_key) <= m // S + int(np.count_nonzero(sizes)) <= p["units"], (n, nm, b, c)


def test_the_8_word_plans_are_what_they_were():
    keys = ("c", "windows", "run_length", "chunk_len", "msms_per_launch", "coarse_bins", "skew_floor")
    assert tuple(M.launch_plan(1 << 17)[k] for k in keys) == (16, 17, 16, 8, 1, 32, 12)
    assert tuple(M.launch_plan(1 << 20)[k] for k in keys) == (16, 17, 64, 8, 1, 256, 56)
    assert tuple(M.launch_plan((1 << 20) + 1)[k] for k in keys) == (16, 17, 68, 8, 1, 256, 56)
    assert M.launch_plan(1 << 20, 2, True)["run_length"] == 64
    # a narrow launch that is not dense keeps its run length too: b = 8 at 4,097 terms
    assert M._test_dense_plan(4097, scalar_bits=8) == {"dense": 0, "E": 0, "nkeys": 256, "units": 0, "K": 16}
