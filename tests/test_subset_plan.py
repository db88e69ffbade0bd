"""Subset MSMs on a resident-bases handle, the host-only part (include/msm.h
msm_bases_compute_subset*): the launch plan of a subset (msm_test_subset_plan) counts levels * m
terms while its entry width follows the handle's levels * n records, and the argument rules that
need no device.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import msm_amd as M

WIDTHS = range(4, 21)
LEVELS = range(1, 9)


def _packed(levels, n_handle, fb):
    """MsmDims::packed restated: the entry (record << 1 | sign) and its fb-bit fine key share one u32."""
    return int(levels * n_handle <= 1 << (31 - fb))


@pytest.mark.parametrize("c", WIDTHS)
def test_subset_plan_counts_terms_and_indexes_records(c):
    for levels in LEVELS:
        for n_handle, m in ((5000, 64), (5000, 4999), ((1 << 17) + 1, 300), (3, 3)):
            for indexed, first in ((False, 1), (True, 0)) + (((False, 0),) if levels > 1 else ()):
                if not indexed and first + m > n_handle:
                    m = n_handle - first
                p = M._test_subset_plan(n_handle, levels, c, first, m, indexed)
                where = (c, levels, n_handle, m, indexed, first)
                assert p["n"] == levels * m, where
                assert p["stride"] == n_handle, where
                assert p["sub"] == (2 if indexed else 1), where
                assert p["packed"] == _packed(levels, n_handle, p["fb"]), where
        # duplicates allowed: an index list longer than the handle
        p = M._test_subset_plan(3, levels, c, 0, 257, True)
        assert (p["n"], p["stride"], p["packed"]) == (levels * 257, 3, 1)


def test_wide_window_on_a_large_handle_is_unpacked_although_m_is_tiny():
    n_handle, c = (1 << 20) + 8, 16
    for indexed, first, m in ((False, (1 << 20) - 24, 32), (True, 0, 64)):
        p = M._test_subset_plan(n_handle, 1, c, first, m, indexed)
        assert p["n"] == m and p["stride"] == n_handle
        assert 1 << (31 - p["fb"]) < n_handle  # the case exists: the records outgrow the packed entry
        assert p["packed"] == 0 == _packed(1, n_handle, p["fb"])
    # the same m on a handle of exactly the records a packed entry still reaches
    fb = p["fb"]
    assert M._test_subset_plan(1 << (31 - fb), 1, c, 0, m, True)["packed"] == 1
    assert M._test_subset_plan((1 << (31 - fb)) + 1, 1, c, 0, m, True)["packed"] == 0
    # and through the levels: 8 levels of 2^17 + 1 records
    p = M._test_subset_plan((1 << 17) + 1, 8, c, 0, m, True)
    assert p["packed"] == _packed(8, (1 << 17) + 1, p["fb"])


@pytest.mark.parametrize("c", WIDTHS)
def test_prefix_of_an_unfolded_handle_is_the_plain_plan(c):
    """The range [0, m) of a levels = 1 handle takes the existing path with n := m: no subset
    variant, and the entries index m records only."""
    for n_handle, m in ((5000, 64), ((1 << 20) + 8, 64), (4097, 4097)):
        p = M._test_subset_plan(n_handle, 1, c, 0, m, False)
        assert (p["sub"], p["stride"], p["n"]) == (0, 0, m)
        assert p["packed"] == _packed(1, m, p["fb"])


def test_subset_argument_rules_without_a_device():
    out = np.zeros(5, np.uint32)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    L = M.load()

    def plan(n_handle, levels, c, first, m, indexed):
        return L.msm_test_subset_plan(n_handle, levels, c, first, m, indexed, op)

    assert plan(100, 1, 13, 0, 100, 0) == 0
    assert plan(100, 1, 13, 0, 101, 0) == -1       # first + m > n
    assert plan(100, 2, 13, 1, 100, 0) == -1
    assert plan(100, 1, 13, 100, 1, 0) == -1
    assert plan(100, 1, 13, 101, 0, 0) == -1
    assert plan(100, 1, 13, 100, 0, 0) == 0        # the empty range at the end
    assert plan(100, 1, 13, 1 << 63, 1 << 63, 0) == -1  # no wrap-around
    assert plan(100, 1, 13, 1, 5, 1) == -1         # first beside an index list
    assert plan(100, 1, 13, 0, 5, 1) == 0
    assert plan(0, 1, 13, 0, 5, 1) == -1           # no base to index
    assert plan(0, 1, 13, 0, 0, 1) == 0
    for levels in (1, 2, 8):                       # levels * m < 2^30, as at creation
        lim = (1 << 30) // levels
        assert plan(100, levels, 16, 0, lim, 1) == -1
        assert plan(100, levels, 16, 0, 1 << 40, 1) == -1
    assert plan(100, 0, 13, 0, 5, 0) == -1 and plan(100, 9, 13, 0, 5, 0) == -1
    assert plan(100, 2, 3, 0, 5, 0) == -2 and plan(100, 1, 21, 1, 5, 0) == -2


def test_subset_entries_reject_null_and_unknown_handles():
    L = M.load()
    sc = np.zeros((4, 8), np.uint32)
    scp = sc.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros(16, np.uint32)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    sub = M.Subset(0, 4, None)
    sp = ctypes.byref(sub)
    ptrs = (ctypes.c_void_p * 1)(scp)
    pp = ctypes.cast(ptrs, ctypes.c_void_p)
    for h in (None, 12345):
        assert L.msm_bases_compute_subset(h, sp, scp, None, op) == -1
        assert L.msm_bases_compute_subset_device(h, sp, scp, None, None, op) == -1
        assert L.msm_bases_compute_subset_many(h, sp, pp, 1, None, op) == -1
        assert L.msm_bases_compute_subset_many_device(h, sp, pp, 1, None, None, op) == -1
    assert L.msm_bases_compute_subset(12345, None, scp, None, op) == -1
    assert ctypes.sizeof(M.Subset) == 24  # include/msm.h msm_subset_t: two u64 and a pointer
