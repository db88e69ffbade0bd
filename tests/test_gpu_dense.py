"""GPU tests of the dense-bucket accumulation (k_dense_segments / k_dense_units / k_dense_fold): the
narrow-scalar launches whose buckets hold 128 entries or more, bit-exact against the oracle (small
shapes: points with small-order points, duplicates and a negation pair) or the closed form over
gen_points (large shapes) on the same scalars zero-extended to 8 words -- never against another
entry of the library.  With E = 4 a unit's segment is 256 entries; the sizes below sit on its edges."""
import functools
import random
import statistics
import time

import numpy as np
import pytest

import msm_amd as M
from _closed_form import as_xy, closed_form
from _dense_model import segment_map, size_vectors
from _narrow_model import edge_scalars
from oracle import oracle as O
from test_gpu_subset import _dev, _points

pytestmark = pytest.mark.gpu

N = 4096
K0, STEP = 3, 5          # the large shapes' points: (K0 + i STEP) G
BIG = 1 << 18


def _extend(w):
    full = np.zeros((w.shape[0], 8), np.uint32)
    full[:, 8 - w.shape[1]:] = w
    return full


def _wire(vals, b):
    w = M.scalars_to_wire([int(v) for v in vals], scalar_bits=b)
    w.setflags(write=False)
    return w


def _oracle(pts, w):
    return O.msm(np.ascontiguousarray(pts), _extend(w), window=10, threads=8)


def _dense(n, b, c=0, nm=1, pipelined=False):
    return M._test_dense_plan(n, nm, pipelined, b, c)["dense"] == 1


@pytest.fixture(scope="module")
def small():
    with M.Bases.from_wire(_points(N), levels=1) as h:
        yield h


@pytest.fixture(scope="module")
def big():
    """A levels-1 handle of 2^18 generated points, made from device-resident points (kept for the
    8-word entry that takes them on every call)."""
    d_pts = _dev(M.gen_points(BIG, k0=K0, step=STEP))
    with M.Bases.from_device(d_pts, BIG, levels=1) as h:
        yield h, d_pts


def _ones(k, n=N):
    return _wire([1] * k + [0] * (n - k), 1)


# ---- segment edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 255, 256, 257, 512, 513, 4096])
def test_segment_edges(small, k):
    assert _dense(N, 1)
    sc = _ones(k)
    exp = _oracle(_points(N), sc)
    assert small.compute(sc, scalar_bits=1) == exp
    assert small.compute_device(_dev(sc), scalar_bits=1) == exp


def test_empty_keys_and_lone_entries(small):
    """b = 3 is one 4-bit window, value v in bucket v - 1: buckets 0 and 2 full, bucket 1 empty,
    bucket 4 one entry."""
    assert _dense(N, 3)
    rnd = random.Random(31)
    vals = [rnd.choice((0, 1, 1, 3, 3, 4, 6, 7)) for _ in range(N)]
    vals[1234] = 5
    assert vals.count(2) == 0 and vals.count(5) == 1 and vals.count(1) > 512 and vals.count(3) > 512
    sc = _wire(vals, 3)
    exp = _oracle(_points(N), sc)
    assert small.compute(sc, scalar_bits=3) == exp
    assert small.compute_device(_dev(sc), scalar_bits=3) == exp


# ---- signed digits over several windows ---------------------------------------------------------------
def test_three_signed_windows(small):
    """b = 8 at width 4: three 3-bit windows, 1,024 entries per bucket."""
    assert _dense(N, 8, 4) and M._test_dense_plan(N, 1, False, 8, 4)["nkeys"] == 12
    rnd = random.Random(32)
    vals = [rnd.getrandbits(8) for _ in range(N)]
    for i, v in enumerate(edge_scalars(8, 4)):
        vals[10 + i] = v
    sc = _wire(vals, 8)
    exp = _oracle(_points(N), sc)
    assert small.compute(sc, window_size=4, scalar_bits=8) == exp
    assert small.compute_device(_dev(sc), window_size=4, scalar_bits=8) == exp


def test_16_bits_at_width_16(big):
    """An explicit width is kept: 9 + 8 bits, signed digits, on the first 2^16 bases."""
    h, _ = big
    n = 1 << 16
    assert _dense(n, 16, 16)
    sc = np.random.RandomState(33).randint(0, 1 << 16, size=(n, 1)).astype(np.uint32)
    edges = edge_scalars(16, 16)
    sc[10:10 + len(edges), 0] = edges
    exp = closed_form(K0, STEP, _extend(sc))
    assert h.compute_subset(sc, window_size=16, scalar_bits=16) == exp
    assert h.compute_subset_device(_dev(sc), window_size=16, scalar_bits=16) == exp


# ---- fold depth ---------------------------------------------------------------------------------------
def test_one_bucket_of_more_partials_than_fold_lanes(big):
    h, _ = big
    n = (1 << 17) + 1
    p = M._test_dense_plan(n, 1, False, 1, 0)
    assert p["dense"] == 1 and n // (64 * p["E"]) > 256
    sc = np.ones((n, 1), np.uint32)
    exp = closed_form(K0, STEP, _extend(sc))
    assert h.compute_subset(sc, scalar_bits=1) == exp
    assert h.compute_subset_device(_dev(sc), scalar_bits=1) == exp


def test_all_equal_bytes(big):
    h, _ = big
    assert _dense(BIG, 8)
    sc = np.full((BIG, 1), 0xA5, np.uint32)
    exp = closed_form(K0, STEP, _extend(sc))
    assert h.compute(sc, scalar_bits=8) == exp
    assert h.compute_device(_dev(sc), scalar_bits=8) == exp


# ---- batches ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch_case():
    scs = [_ones(k) for k in (4096, 257, 0, 1000, 1)]
    return scs, [_oracle(_points(N), s) for s in scs]


@pytest.mark.parametrize("flags", [0, M.MSM_FLAG_SERIAL])
def test_batches(small, flags):
    """Five vectors: a launch of four and a short last one; then a call with no entry at all."""
    assert _dense(N, 1, 0, 4, True)
    scs, exp = _batch_case()
    d_scs = [_dev(s) for s in scs]
    assert [as_xy(r) for r in small.compute_many(scs, flags=flags, scalar_bits=1)] == exp
    assert [as_xy(r) for r in small.compute_many_device(d_scs, flags=flags, scalar_bits=1)] == exp
    zero = [scs[2]] * 5
    assert [as_xy(r) for r in small.compute_many(zero, flags=flags, scalar_bits=1)] == [exp[2]] * 5
    assert [as_xy(r) for r in small.compute_many_device([d_scs[2]] * 5, flags=flags, scalar_bits=1)] == [exp[2]] * 5
    assert [as_xy(r) for r in small.compute_many_device(d_scs, flags=flags, scalar_bits=1)] == exp


# ---- subsets ------------------------------------------------------------------------------------------
def test_subsets(small):
    first, m = 255, 2048
    assert _dense(m, 1)
    pts = _points(N)
    rnd = np.random.RandomState(34)
    sc = rnd.randint(0, 2, size=(m, 1)).astype(np.uint32)
    exp = _oracle(pts[first:first + m], sc)
    assert small.compute_subset(sc, first=first, scalar_bits=1) == exp
    assert small.compute_subset_device(_dev(sc), first=first, scalar_bits=1) == exp
    idx = rnd.randint(0, N, size=m).astype(np.uint32)
    idx[m // 2] = idx[0]
    idx[2:12] = 7  # ten copies of one base
    exp = _oracle(pts[idx], sc)
    assert small.compute_subset(sc, indices=idx, scalar_bits=1) == exp
    assert small.compute_subset_device(_dev(sc), indices=_dev(idx), scalar_bits=1) == exp


# ---- replay -------------------------------------------------------------------------------------------
def test_replay_with_other_bucket_sizes_and_other_plans():
    """One handle, one call after the other: the segment map is rebuilt by every launch, and a
    launch that is not dense, or the 8-word one, between two dense ones disturbs neither."""
    n = 4097
    pts = _points(n)
    assert _dense(n, 1) and _dense(n, 2) and not _dense(n, 8)
    rnd = np.random.RandomState(35)
    full = M.gen_scalars(n, seed=79)
    steps = [(1, _ones(1000, n)),
             (8, rnd.randint(0, 256, size=(n, 1)).astype(np.uint32)),
             (None, full),
             (1, rnd.randint(0, 2, size=(n, 1)).astype(np.uint32)),
             (1, _ones(4097, n)),
             (2, rnd.randint(0, 4, size=(n, 1)).astype(np.uint32))]
    exp = [O.msm(pts, sc if b is None else _extend(sc), window=10, threads=8) for b, sc in steps]
    keep = []
    with M.Bases.from_wire(pts, levels=1) as h:
        for (b, sc), e in zip(steps, exp):
            d = _dev(sc)
            keep.append(d)  # kept alive: the next tensor gets a new address
            assert h.compute_device(d, scalar_bits=b) == e, b
            assert h.compute(sc, scalar_bits=b) == e, b


# ---- the device-side range error ----------------------------------------------------------------------
def test_range_error_leaves_the_slot_clean(small):
    good = _ones(700)
    exp = _oracle(_points(N), good)
    bad = np.array(good)
    bad[N - 1, 0] = 2  # bit 1 of a 1-bit scalar
    d_good = _dev(good)
    for call in (lambda: small.compute_device(_dev(bad), scalar_bits=1),
                 lambda: small.compute_many_device([d_good, _dev(bad), d_good], scalar_bits=1)):
        with pytest.raises(M.MsmError) as e:
            call()
        assert e.value.code == -1
        assert small.compute_device(d_good, scalar_bits=1) == exp
    assert [as_xy(r) for r in small.compute_many_device([d_good] * 3, scalar_bits=1)] == [exp] * 3


# ---- profiling ----------------------------------------------------------------------------------------
def test_profiles_cover_the_three_kernels(small):
    """Mode 1 (eager, an event per phase) reports E as the run length; mode 2 brackets the
    accumulation inside the replayed graph: ev_acc0 before the segment map, ev_acc1 after the fold."""
    sc = _ones(3000)
    exp = _oracle(_points(N), sc)
    d_sc = _dev(sc)
    plan = M._test_dense_plan(N, 1, False, 1, 0)
    try:
        M.set_profiling(1)
        assert small.compute_device(d_sc, scalar_bits=1) == exp
        prof = M.last_profile()
        assert prof["run_length"] == plan["E"] == 4
        assert 0 < prof["accumulate"] < prof["device_total"]
        assert prof["entries"] == 3000
        M.set_profiling(2)
        for _ in range(2):  # the capture, then a replay
            assert small.compute_device(d_sc, scalar_bits=1) == exp
            prof = M.last_profile()
            assert 0 < prof["accumulate"] < prof["device_total"]
    finally:
        M.set_profiling(0)
    assert small.compute_device(d_sc, scalar_bits=1) == exp


# ---- the prologue alone -------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys,m,S", [(1, 1000, 64), (8, 4096, 256), (12, 3 * 4096, 256), (256, 1 << 18, 256),
                                       (512, 1 << 20, 768), (4096, 1 << 20, 256), (1 << 13, 1 << 21, 768)])
def test_segment_map_against_the_model(nkeys, m, S):
    for sizes in size_vectors(nkeys, m, S, seed=nkeys):
        bucket_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
        seg_base, unit_key = M._test_dense_segments(bucket_start, S)
        want_base, want_key = segment_map(sizes, S)
        live = int(want_base[-1])
        assert np.array_equal(seg_base, want_base)
        assert np.array_equal(unit_key[:live], want_key)
        assert np.all(unit_key[live:] == 0xFFFFFFFF)  # nothing written past the live units


# ---- the condition the parent fails -------------------------------------------------------------------
def test_bytes_at_2p18_beat_the_8_word_entries(big):
    """b = 8, n = 2^18, random bytes, device-resident, levels-1 handle: the median of five awaited
    narrow calls (after a warm-up) is below the median of five 8-word calls on the same scalars
    zero-extended, both the handle's 8-word call (1.069 ms against the narrow call's 1.512 before the
    dense accumulation: profiles/bases_narrow_sweep.jsonl) and msm_compute_device, which prepares the
    points as well.  No margin."""
    h, d_pts = big
    assert _dense(BIG, 8)
    sc = np.random.RandomState(36).randint(0, 256, size=(BIG, 1)).astype(np.uint32)
    sc8 = _extend(sc)
    exp = closed_form(K0, STEP, sc8)
    d_sc, d_sc8 = _dev(sc), _dev(sc8)

    def median_ms(fn):
        assert fn() == exp  # warm-up: graph capture, allocations
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            res = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
            assert res == exp
        return statistics.median(ts)

    narrow = median_ms(lambda: h.compute_device(d_sc, scalar_bits=8))
    extended = median_ms(lambda: h.compute_device(d_sc8))
    entry = median_ms(lambda: M.compute_msm_device(d_pts, d_sc8, BIG))
    print(f"b = 8 at 2^18 awaited: narrow {narrow:.3f} ms, 8-word on the handle {extended:.3f} ms, "
          f"msm_compute_device {entry:.3f} ms")
    assert narrow < extended
    assert narrow < entry
