"""GPU tests of narrow-scalar MSMs on a resident-bases handle (include/msm.h MSM_FLAG_SCALAR_BITS,
msm_amd.Bases.compute*(scalar_bits=b)): scalars of ceil(b / 32) words over the launch geometry of a
b-bit scalar, bit-exact against the oracle on the same scalars zero-extended to 8 words -- never
against another entry of the library."""
import functools
import random

import numpy as np
import pytest

import msm_amd as M
from _closed_form import as_xy
from _narrow_model import auto_width, edge_scalars
from oracle import oracle as O
from test_gpu_subset import _dev, _points

pytestmark = pytest.mark.gpu

N = 4097  # one past the recode workgroup's span: two workgroups, the second with one scalar; odd
# two workgroups and even (paired 4-B code stores), the second of 38 scalars: at one and two words
# (four scalars per lane) its last lane holds two, at three words and more every lane is full
N_EVEN = 4134
BITS = (1, 2, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 224, 225, 253, 254, 256)
WIDTHS = (None, 4, 13, 16, 17)  # 17 takes the 32-bit digit codes


def _auto(b):
    return auto_width(N, b, M.get_best_window_size(N))


def _words(b):
    return -(-b // 32)


def _wire(vals, b):
    w = M.scalars_to_wire(vals, scalar_bits=b)
    w.setflags(write=False)
    return w


def _extend(w):
    """Narrow wire scalars zero-extended to the 8-word format."""
    full = np.zeros((w.shape[0], 8), np.uint32)
    full[:, 8 - w.shape[1]:] = w
    return full


def _oracle(pts, w):
    return O.msm(np.ascontiguousarray(pts), _extend(w), window=10, threads=8)


@functools.lru_cache(maxsize=None)
def _scalars(b, m=N, seed=0):
    """m b-bit scalars: random values, then (from m = 16) 0, 1, 2^b - 1, 2^(b-1) and the carry edges
    of every window of every width the tests run; a single scalar is 2^b - 1."""
    rnd = random.Random(5000 + 97 * b + 13 * m + seed)
    ss = [rnd.getrandbits(b) for _ in range(m)]
    if m >= 16:
        edges = set()
        if b <= 253:
            for c in WIDTHS:
                edges.update(edge_scalars(b, c or _auto(b)))
        else:
            edges.update((0, 1, (1 << b) - 1, 1 << (b - 1)))
        for i, v in enumerate(sorted(edges)[:m - 10]):
            ss[10 + i] = v
    elif m == 1:
        ss[0] = (1 << b) - 1
    return _wire(ss, b)


@functools.lru_cache(maxsize=None)
def _expected(b, seed=0, n=N):
    return _oracle(_points(n), _scalars(b, n, seed))


# ---- parity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", BITS)
def test_parity_with_oracle(b):
    for n in (N, N_EVEN):
        sc, exp = _scalars(b, n), _expected(b, n=n)
        assert sc.shape == (n, _words(b))
        d_sc = _dev(sc)
        with M.Bases.from_wire(_points(n), levels=1) as h:
            for c in WIDTHS:
                assert h.compute(sc, window_size=c, scalar_bits=b) == exp, (b, n, c)
                assert h.compute_device(d_sc, window_size=c, scalar_bits=b) == exp, (b, n, c)


@pytest.mark.parametrize("n", [1, 2])
def test_tiny_handles(n):
    pts = _points(n)
    with M.Bases.from_wire(pts, levels=1) as h:
        for b in BITS:
            sc = _scalars(b, n)
            exp = _oracle(pts, sc)
            for c in WIDTHS:
                assert h.compute(sc, window_size=c, scalar_bits=b) == exp, (n, b, c)
                assert h.compute_device(_dev(sc), window_size=c, scalar_bits=b) == exp, (n, b, c)


# ---- every entry ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _entry_case(b):
    """Five scalar vectors (a short last launch), a range, an index list with repeats, and the
    oracle's results for each."""
    pts = _points(N)
    scs = [_scalars(b, N, seed) for seed in range(5)]
    full = [_expected(b, seed) for seed in range(5)]
    first, m = 255, 1001
    sub = [_scalars(b, m, seed) for seed in range(5)]
    rng = [_oracle(pts[first:first + m], s) for s in sub]
    idx = np.random.RandomState(b).randint(0, N, size=m).astype(np.uint32)
    idx[m // 2] = idx[0]
    idx[1] = N - 1
    idx[2:12] = np.arange(10)
    idx.setflags(write=False)
    ind = [_oracle(pts[idx], s) for s in sub]
    return scs, full, first, sub, rng, idx, ind


@pytest.mark.parametrize("flags", [0, M.MSM_FLAG_SERIAL])
@pytest.mark.parametrize("b", [8, 33, 64, 128, 253])
def test_every_entry(b, flags):
    scs, full, first, sub, rng, idx, ind = _entry_case(b)
    d_scs, d_sub, d_idx = [_dev(s) for s in scs], [_dev(s) for s in sub], _dev(idx)
    with M.Bases.from_wire(_points(N), levels=1) as h:
        assert [as_xy(r) for r in h.compute_many(scs, flags=flags, scalar_bits=b)] == full
        assert [as_xy(r) for r in h.compute_many_device(d_scs, flags=flags, scalar_bits=b)] == full
        assert h.compute_subset(sub[0], first=first, scalar_bits=b) == rng[0]
        assert h.compute_subset_device(d_sub[1], first=first, scalar_bits=b) == rng[1]
        assert h.compute_subset(sub[2], indices=idx, scalar_bits=b) == ind[2]
        assert h.compute_subset_device(d_sub[3], indices=d_idx, scalar_bits=b) == ind[3]
        assert [as_xy(r) for r in h.compute_subset_many(sub, first=first, flags=flags, scalar_bits=b)] == rng
        assert [as_xy(r) for r in h.compute_subset_many_device(d_sub, first=first, flags=flags,
                                                               scalar_bits=b)] == rng
        assert [as_xy(r) for r in h.compute_subset_many(sub, indices=idx, flags=flags, scalar_bits=b)] == ind
        assert [as_xy(r) for r in h.compute_subset_many_device(d_sub, indices=d_idx, flags=flags,
                                                               scalar_bits=b)] == ind
        # the prefix [0, m) of a levels = 1 handle: the plain launch on its first m records
        assert h.compute_subset(sub[4], scalar_bits=b) == _oracle(_points(N)[:sub[4].shape[0]], sub[4])


def test_device_scalars_that_are_only_word_aligned():
    """A slice of a larger tensor: 4 bytes past a 16-byte boundary, read word by word."""
    import torch

    with M.Bases.from_wire(_points(N), levels=1) as h:
        for b in (32, 64):
            sc = _scalars(b)
            buf = torch.zeros(sc.size + 1, dtype=torch.int32, device="cuda")
            buf[1:] = _dev(sc).reshape(-1)
            assert buf[1:].data_ptr() % 16 == 4
            assert h.compute_device(buf[1:], scalar_bits=b) == _expected(b), b


# ---- the plan key and the replayed graph's inputs ---------------------------------------------------
def test_successive_calls_with_other_widths_on_one_handle():
    full = M.gen_scalars(N, seed=77)
    exp_full = O.msm(_points(N), full, window=10, threads=8)
    with M.Bases.from_wire(_points(N), levels=1) as h:
        keep = []
        for b, seed in ((64, 0), (64, 1), (33, 0), (1, 0), (2, 0), (3, 0), (64, 2)):
            sc = _scalars(b, N, seed)
            d = _dev(sc)
            keep.append(d)  # kept alive: the next tensor gets a new address
            assert h.compute_device(d, scalar_bits=b) == _expected(b, seed), (b, seed)
            assert h.compute(sc, scalar_bits=b) == _expected(b, seed), (b, seed)
        assert h.compute(full) == exp_full
        assert h.compute_device(_dev(full)) == exp_full
        assert h.compute(_scalars(64), scalar_bits=64) == _expected(64)
        # 8 words declared as 256 bits: the plain call
        assert h.compute(full, scalar_bits=256) == exp_full


# ---- giant buckets ----------------------------------------------------------------------------------
def test_all_scalars_in_one_bucket():
    pts = _points(N)
    ones = _wire([1] * N, 1)
    s = random.Random(4).getrandbits(64) | 1 << 63
    same = _wire([s] * N, 64)
    with M.Bases.from_wire(pts, levels=1) as h:
        for c in WIDTHS:
            assert h.compute(ones, window_size=c, scalar_bits=1) == _oracle(pts, ones), c
            assert h.compute_device(_dev(same), window_size=c, scalar_bits=64) == _oracle(pts, same), c


# ---- folded handles run narrow calls unfolded -------------------------------------------------------
@pytest.mark.parametrize("levels", [2, 3])
def test_narrow_calls_on_a_folded_handle(levels):
    full = M.gen_scalars(N, seed=78)
    exp_full = O.msm(_points(N), full, window=10, threads=8)
    idx = _entry_case(64)[5]
    with M.Bases.from_wire(_points(N), levels=levels, window_size=15) as h:
        assert h.info["levels"] == levels
        for b in (1, 64, 129, 253):
            for c in (None, 4, 13, 15, 16, 17):  # any width: the level-0 records do not depend on it
                assert h.compute(_scalars(b), window_size=c, scalar_bits=b) == _expected(b), (b, c)
            assert h.compute_device(_dev(_scalars(b)), scalar_bits=b) == _expected(b), b
        sub = _entry_case(64)[3]
        assert h.compute_subset(sub[0], first=255, scalar_bits=64) == _entry_case(64)[4][0]
        assert h.compute_subset(sub[2], indices=idx, scalar_bits=64) == _entry_case(64)[6][2]
        assert h.compute(full) == exp_full  # folded, as before
        assert h.compute(full, scalar_bits=256) == exp_full
        with pytest.raises(M.MsmError):  # the 8-word call keeps the handle's width
            h.compute(full, window_size=13, scalar_bits=254)


# ---- errors -----------------------------------------------------------------------------------------
def _invalid(call):
    with pytest.raises(M.MsmError) as e:
        call()
    assert e.value.code == -1


def test_excess_bits():
    b, count = 33, 5
    scs = [_scalars(b, N, seed) for seed in range(count)]
    exp = [_expected(b, seed) for seed in range(count)]
    bad = scs[-1].copy()
    bad[N - 1, 0] |= 2  # bit 33
    d_scs = [_dev(s) for s in scs]
    with M.Bases.from_wire(_points(N), levels=1) as h:
        _invalid(lambda: h.compute_many(scs[:-1] + [bad], scalar_bits=b))
        assert [as_xy(r) for r in h.compute_many(scs, scalar_bits=b)] == exp  # the very next call is exact
        _invalid(lambda: h.compute(bad, scalar_bits=b))
        # on the device the recode masks the bit: an error, and the slot left clean
        _invalid(lambda: h.compute_many_device(d_scs[:-1] + [_dev(bad)], scalar_bits=b))
        assert [as_xy(r) for r in h.compute_many_device(d_scs, scalar_bits=b)] == exp
        _invalid(lambda: h.compute_device(_dev(bad), scalar_bits=b))
        assert h.compute_device(d_scs[0], scalar_bits=b) == exp[0]
        _invalid(lambda: h.compute_subset_device(_dev(bad), scalar_bits=b))
        assert h.compute(scs[1], scalar_bits=b) == exp[1]
        # the first scalar of the first vector, and every excess bit of the word
        bad0 = scs[0].copy()
        bad0[0, 0] = 0xfffffffe
        _invalid(lambda: h.compute_many_device([_dev(bad0)] + d_scs[1:], scalar_bits=b))
        assert [as_xy(r) for r in h.compute_many_device(d_scs, scalar_bits=b)] == exp


def test_width_out_of_range():
    sc = _scalars(64)
    with M.Bases.from_wire(_points(N), levels=1) as h:
        for b in (0, 257):
            _invalid(lambda: h.compute(sc, scalar_bits=b))
            _invalid(lambda: h.compute_device(_dev(sc), scalar_bits=b))
            _invalid(lambda: h.compute_many([sc], scalar_bits=b))
            _invalid(lambda: h.compute_subset(sc[:10], first=3, scalar_bits=b))
        assert h.compute(sc, scalar_bits=64) == _expected(64)


# ---- profile ----------------------------------------------------------------------------------------
def test_profile_reports_the_launchs_windows():
    with M.Bases.from_wire(_points(N), levels=1) as h:
        M.set_profiling(True)
        try:
            for b, c in ((64, 16), (64, None), (8, 4), (253, 13), (129, 17)):
                assert h.compute(_scalars(b), window_size=c, scalar_bits=b) == _expected(b)
                plan = M._test_narrow_plan(N, b, c or 0)
                prof = M.last_profile()
                assert prof["windows"] == plan["windows"], (b, c)
                assert prof["window_bits"] == plan["c"], (b, c)
        finally:
            M.set_profiling(False)
