"""GPU tests of subset MSMs on a resident-bases handle (include/msm.h msm_bases_compute_subset*,
msm_amd.Bases.compute_subset*): a contiguous range or an index list of the handle's bases, bit-exact
against the oracle on the gathered points (small sizes) or the closed form over k G bases (where the
size needs it) -- never against another entry of the library."""
import functools
import random

import numpy as np
import pytest

import msm_amd as M
from _bases_model import fold
from _closed_form import as_xy, scalar_dot
from oracle import oracle as O

pytestmark = pytest.mark.gpu

I4 = O.sqrt_mod(O.P - 1)            # sqrt(-1): (I4, 0) has order 4
SPECIAL = [(0, 1), (0, O.P - 1), (I4, 0), (O.P - I4, 0)]
WIDTHS = (4, 13, 15, 16, 17)
LEVELS = (1, 2, 3, 8)
N = 4097


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


def _projective(pts, i, z):
    x, y = (O.be_words_to_int(pts[i, 8 * j: 8 * j + 8]) for j in range(2))
    for j, v in enumerate((x * z % O.P, y * z % O.P, x * y % O.P * z % O.P, z)):
        pts[i, 8 * j: 8 * j + 8] = O.int_to_be_words(v)


@functools.lru_cache(maxsize=None)
def _points(n):
    """n wire points: multiples of G, with (from n = 16) the small-order points, z != 1 records,
    duplicates and a point beside its negation; below that a projective point."""
    pts = O.gen_points(n, k0=3, step=7).copy()
    if n >= 16:
        pts[1:5] = O.affine_to_wire(SPECIAL)
        pts[6] = pts[5]                                             # a duplicate
        x, y = (O.be_words_to_int(pts[7, 8 * j: 8 * j + 8]) for j in range(2))
        pts[8] = O.affine_to_wire([O.aff_neg((x, y))])[0]           # 7 and 8: a point and its negation
        _projective(pts, 9, 12345678901)
        _projective(pts, n - 1, O.P - 2)
        _projective(pts, 2, 77)                                     # the order-2 point, projective
    else:
        _projective(pts, 0, 5)
    pts.setflags(write=False)
    return pts


def _special_scalars():
    """The edge scalars of every (width, levels) pair the parity tests use."""
    vals = [0, 1, O.R_ORDER - 1, (1 << 256) - 1]
    for c in WIDTHS:
        for k in LEVELS[1:]:
            _, S = fold(c, k)
            vals += [(1 << S) - 1, 1 << S, (1 << S) + 1]
            vals += [(1 << (j * S)) - 1 for j in range(2, k) if j * S <= 256]
    return sorted(set(vals))


@functools.lru_cache(maxsize=None)
def _scalars(m, seed=0):
    """m scalars: random 256-bit and canonical values in turn, then (from m = 16) every edge scalar
    that fits; a single scalar is the all-ones one (every chunk of every fold at its maximum)."""
    rnd = random.Random(2000 + 31 * m + seed)
    ss = [rnd.getrandbits(256) if i % 2 else rnd.randrange(O.R_ORDER) for i in range(m)]
    if m >= 16:
        for i, v in enumerate(_special_scalars()[:m - 10]):
            ss[10 + i] = v
    elif m == 1:
        ss[0] = (1 << 256) - 1
    w = O.ints_to_be_words(ss)
    w.setflags(write=False)
    return w


def _oracle(pts, sc):
    return O.msm(np.ascontiguousarray(pts), np.ascontiguousarray(sc), window=10, threads=8)


RANGES = ((0, 1), (0, 4096), (0, 4097), (1, 4096), (4096, 1), (255, 257))


@functools.lru_cache(maxsize=None)
def _range_expected(first, m):
    return _oracle(_points(N)[first:first + m], _scalars(m))


@functools.lru_cache(maxsize=None)
def _index_cases():
    """name -> (handle points, indices, scalars, expected), expected by the oracle on the gathered points."""
    rnd = np.random.RandomState(7)
    pts = _points(N)
    cases = {}
    for m in (1, 257, 4097):
        idx = rnd.randint(0, N, size=m).astype(np.uint32)
        if m > 1:
            idx[m // 2] = idx[0]     # repeats for certain,
            idx[1] = N - 1           # the last record,
            idx[2:12] = np.arange(10)  # and the special points
        cases[f"random{m}"] = (N, idx, _scalars(m))
    cases["reversed"] = (N, np.arange(N - 1, -1, -1, dtype=np.uint32), _scalars(N))
    cases["all_last"] = (N, np.full(N, N - 1, np.uint32), _scalars(N))
    # one point N times with one scalar: every window is one bucket, which takes the skew joins
    s = random.Random(3).randrange(O.R_ORDER)
    cases["all_last_one_scalar"] = (N, np.full(N, N - 1, np.uint32), O.ints_to_be_words([s] * N))
    cases["more_terms_than_bases"] = (3, rnd.randint(0, 3, size=257).astype(np.uint32), _scalars(257))
    out = {}
    for name, (n, idx, sc) in cases.items():
        hp = pts if n == N else _points(n)
        out[name] = (hp, idx, sc, _oracle(hp[idx], sc))
    return out


# ---- range form -------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", LEVELS)
def test_range_parity_with_oracle(levels):
    pts = _points(N)
    for c in WIDTHS:
        with M.Bases.from_wire(pts, levels=levels, window_size=c) as b:
            for first, m in RANGES:
                sc, exp = _scalars(m), _range_expected(first, m)
                assert b.compute_subset(sc, first=first, window_size=c) == exp, (levels, c, first, m)
                assert b.compute_subset_device(_dev(sc), first=first) == exp, (levels, c, first, m)


# ---- indexed form -----------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("case", ["random1", "random257", "random4097", "reversed", "all_last",
                                  "all_last_one_scalar", "more_terms_than_bases"])
def test_indexed_parity_with_oracle(case, levels):
    hp, idx, sc, exp = _index_cases()[case]
    d_idx, d_sc = _dev(idx), _dev(sc)
    for c in WIDTHS:
        with M.Bases.from_wire(hp, levels=levels, window_size=c) as b:
            assert b.compute_subset(sc, indices=idx, window_size=c) == exp, (case, levels, c)
            assert b.compute_subset_device(d_sc, indices=d_idx) == exp, (case, levels, c)


# ---- level and chunk boundaries (closed form) -------------------------------------------------------
def _closed(k0, step, idx, sc):
    ks = k0 + step * np.asarray(idx, dtype=np.uint64)
    return O.scalar_mul(O.G, scalar_dot(ks, sc) % O.R_ORDER)


@pytest.mark.parametrize("c", [None, 17])
def test_level_boundary_inside_a_chunk_and_a_chunk_boundary_inside_a_level(c):
    # levels * m = 18,000 positions: level 1 starts at 9,000, inside scatter chunk 0, and chunk 1
    # starts at 16,384, inside level 1; c = 17 takes the 32-bit digit codes
    n, m, first, k0, step = 12000, 9000, 1000, 5, 3
    pts = O.gen_points(n, k0=k0, step=step)
    sc = M.gen_scalars(m, seed=41)
    idx = np.random.RandomState(11).randint(0, n, size=m).astype(np.uint32)
    idx[:3] = (n - 1, 0, n - 1)
    exp_range = _closed(k0, step, first + np.arange(m), sc)
    exp_index = _closed(k0, step, idx, sc)
    with M.Bases.from_wire(pts, levels=2, window_size=c) as b:
        assert b.compute_subset(sc, first=first) == exp_range
        assert b.compute_subset_device(_dev(sc), first=first) == exp_range
        assert b.compute_subset(sc, indices=idx) == exp_index
        assert b.compute_subset_device(_dev(sc), indices=_dev(idx)) == exp_index


# ---- unpacked entries with high records -------------------------------------------------------------
def test_small_subsets_of_a_handle_past_the_packed_entry_range():
    """2^20 + 8 records at c = 16 (fine bits 11): a record index past 2^20 does not fit beside the
    fine key in one word, however few terms the MSM has -- the entry width follows the records."""
    n, k0, step = (1 << 20) + 8, 9, 2
    pts = M.gen_points(n, k0=k0, step=step)
    idx = np.random.RandomState(5).randint(0, n, size=64).astype(np.uint32)
    idx[-8:] = np.arange(n - 8, n)         # the last 8 records
    idx[0] = (1 << 20) - 1
    sc64, sc32 = M.gen_scalars(64, seed=51), M.gen_scalars(32, seed=52)
    first = (1 << 20) - 24
    with M.Bases.from_wire(pts, levels=1) as b:
        assert b.compute_subset(sc64, indices=idx, window_size=16) == _closed(k0, step, idx, sc64)
        assert b.compute_subset_device(_dev(sc64), indices=_dev(idx), window_size=16) == _closed(k0, step, idx, sc64)
        exp = _closed(k0, step, first + np.arange(32), sc32)
        assert b.compute_subset(sc32, first=first, window_size=16) == exp
        assert b.compute_subset_device(_dev(sc32), first=first, window_size=16) == exp


# ---- the `many` entries -----------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("flags", [0, M.MSM_FLAG_SERIAL])
def test_many_entries(levels, flags):
    n, m, count, k0, step = 3000, 1000, 5, 2, 5  # five MSMs: a short last launch
    pts = O.gen_points(n, k0=k0, step=step)
    rnd = np.random.RandomState(23)
    idxs = [rnd.randint(0, n, size=m).astype(np.uint32) for _ in range(count)]
    scs = [M.gen_scalars(m, seed=200 + i) for i in range(count)]
    scs[3] = np.zeros((m, 8), np.uint32)   # an all-zero vector: the identity
    exp = [_closed(k0, step, ix, s) for ix, s in zip(idxs, scs)]
    assert exp[3] == (0, 1)
    d_idxs, d_scs = [_dev(ix) for ix in idxs], [_dev(s) for s in scs]
    with M.Bases.from_wire(pts, levels=levels) as b:
        assert [as_xy(r) for r in b.compute_subset_many(scs, indices=idxs, flags=flags)] == exp
        assert [as_xy(r) for r in b.compute_subset_many_device(d_scs, indices=d_idxs, flags=flags)] == exp
        # all five MSMs over one index vector: the same pointer five times
        exp1 = [_closed(k0, step, idxs[1], s) for s in scs]
        assert [as_xy(r) for r in b.compute_subset_many(scs, indices=[idxs[1]] * count, flags=flags)] == exp1
        assert [as_xy(r) for r in b.compute_subset_many_device(d_scs, indices=[d_idxs[1]] * count, flags=flags)] == exp1
        # and over one range
        expr = [_closed(k0, step, 1999 + np.arange(m), s) for s in scs]
        assert [as_xy(r) for r in b.compute_subset_many(scs, first=1999, flags=flags)] == expr
        assert [as_xy(r) for r in b.compute_subset_many_device(d_scs, first=1999, flags=flags)] == expr
        assert b.compute_subset_many([]).shape == (0, 16)
        assert b.compute_subset_many_device([], indices=[]).shape == (0, 16)


# ---- replayed graphs take each call's own indices ---------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2])
def test_successive_device_calls_with_new_index_tensors(levels):
    n, m, k0, step = 5000, 2000, 7, 4
    pts = O.gen_points(n, k0=k0, step=step)
    rnd = np.random.RandomState(31)
    with M.Bases.from_wire(pts, levels=levels) as b:
        keep = []
        for r in range(3):  # one plan, so one captured graph: new index and scalar buffers each time
            idx = rnd.randint(0, n, size=m).astype(np.uint32)
            sc = M.gen_scalars(m, seed=300 + r)
            d_idx, d_sc = _dev(idx), _dev(sc)
            keep += [d_idx, d_sc]  # kept alive: the next tensors get new addresses
            assert b.compute_subset_device(d_sc, indices=d_idx) == _closed(k0, step, idx, sc), r
            assert b.compute_subset(sc, indices=idx) == _closed(k0, step, idx, sc), r


# ---- errors -----------------------------------------------------------------------------------------
def _invalid(call):
    with pytest.raises(M.MsmError) as e:
        call()
    assert e.value.code == -1


@pytest.mark.parametrize("levels", [1, 2])
def test_out_of_range_indices(levels):
    n, m, k0, step = 1000, 300, 3, 2
    pts = O.gen_points(n, k0=k0, step=step)
    sc = M.gen_scalars(m, seed=61)
    good = np.random.RandomState(3).randint(0, n, size=m).astype(np.uint32)
    exp = _closed(k0, step, good, sc)
    d_sc, d_good = _dev(sc), _dev(good)
    with M.Bases.from_wire(pts, levels=levels) as b:
        for bad_value in (n, (1 << 32) - 1):
            bad = good.copy()
            bad[m - 1] = bad_value
            _invalid(lambda: b.compute_subset(sc, indices=bad))
            assert b.compute_subset(sc, indices=good) == exp          # the very next call is exact
            # on the device the kernel that reads the indices substitutes: an error, never a fault
            _invalid(lambda: b.compute_subset_device(d_sc, indices=_dev(bad)))
            assert b.compute_subset_device(d_sc, indices=d_good) == exp
            assert b.compute_subset(sc, indices=good) == exp
        # a range past the end, and `first` beside an index list
        _invalid(lambda: b.compute_subset(sc, first=n - m + 1))
        _invalid(lambda: b.compute_subset_device(d_sc, first=n - m + 1))
        _invalid(lambda: b.compute_subset(sc, first=1, indices=good))
        assert b.compute_subset(sc, first=n - m) == _closed(k0, step, n - m + np.arange(m), sc)


def test_bad_device_index_in_a_pipelined_call_leaves_the_slots_clean():
    """One MSM of a `many` call has a bad index while skewed launches are in flight behind it: the
    call fails, and the same call with good indices is exact right after (no stale skew flags)."""
    n, m, count, k0, step = 3000, 1000, 6, 2, 5
    pts = O.gen_points(n, k0=k0, step=step)
    s = random.Random(9).randrange(O.R_ORDER)
    skew_sc = O.ints_to_be_words([s] * m)
    idxs = [np.full(m, n - 1 - i, np.uint32) for i in range(count)]   # one base m times each
    exp = [_closed(k0, step, ix, skew_sc) for ix in idxs]
    bad = idxs[0].copy()
    bad[5] = n
    d_sc = _dev(skew_sc)
    d_idxs = [_dev(ix) for ix in idxs]
    with M.Bases.from_wire(pts) as b:
        _invalid(lambda: b.compute_subset_many_device([d_sc] * count, indices=[_dev(bad)] + d_idxs[1:]))
        assert [as_xy(r) for r in b.compute_subset_many_device([d_sc] * count, indices=d_idxs)] == exp
        _invalid(lambda: b.compute_subset_many([skew_sc] * count, indices=idxs[:-1] + [bad]))
        assert [as_xy(r) for r in b.compute_subset_many([skew_sc] * count, indices=idxs)] == exp


def test_closed_handle_and_empty_subsets():
    n = 500
    pts = O.gen_points(n, k0=6, step=1)
    sc = M.gen_scalars(8, seed=8)
    idx = np.arange(8, dtype=np.uint32)
    none = np.zeros((0, 8), np.uint32)
    b = M.Bases.from_wire(pts, levels=2)
    assert b.compute_subset(none) == (0, 1)                                     # m = 0: the identity
    assert b.compute_subset(none, first=n) == (0, 1)
    assert b.compute_subset(none, indices=np.zeros(0, np.uint32)) == (0, 1)
    assert b.compute_subset_device(_dev(sc), m=0) == (0, 1)
    assert [as_xy(r) for r in b.compute_subset_many([none, none])] == [(0, 1)] * 2
    assert b.compute_subset(sc, indices=idx) == _closed(6, 1, idx, sc)
    b.close()
    for call in (lambda: b.compute_subset(sc), lambda: b.compute_subset(sc, indices=idx),
                 lambda: b.compute_subset_device(_dev(sc), indices=_dev(idx)),
                 lambda: b.compute_subset_many([sc], first=1),
                 lambda: b.compute_subset_many_device([_dev(sc)], indices=[_dev(idx)])):
        _invalid(call)


# ---- no cross-talk with the full entries ------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2])
def test_subset_between_two_full_computes(levels):
    n, m, k0, step = 6000, 777, 4, 9
    pts = O.gen_points(n, k0=k0, step=step)
    full, sc = M.gen_scalars(n, seed=71), M.gen_scalars(m, seed=72)
    idx = np.random.RandomState(13).randint(0, n, size=m).astype(np.uint32)
    exp_full = _closed(k0, step, np.arange(n), full)
    with M.Bases.from_wire(pts, levels=levels) as b:
        assert b.compute(full) == exp_full
        assert b.compute_subset(sc, indices=idx) == _closed(k0, step, idx, sc)
        assert b.compute(full) == exp_full
        assert b.compute_subset(sc, first=5000) == _closed(k0, step, 5000 + np.arange(m), sc)
        assert b.compute_subset(sc) == _closed(k0, step, np.arange(m), sc)       # the prefix: the plain path
        assert b.compute_device(_dev(full)) == exp_full
