"""GPU tests of the vector tables (include/msm.h msm_fixed_create_vector; k_vector_build, k_vector_eval,
k_vector_fold): Q_i = sum_(j<k) s_ij B_j for 9 <= k <= 4096, bit-exact.

Every expected record comes from the C oracle: row i is the oracle's MSM of the row's k terms, written as
the canonical wire record.  The shapes are the smallest that meet every path: one full part and a ragged
one, parts of one base, a wave's edges (63, 64, 65 rows), several blocks, both staging paths (8-word and
narrow scalars), one to three fold passes, and two slabs."""
import ctypes
import functools
import random

import numpy as np
import pytest

import msm_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

P = O.P
NSRC = 40
MS = [1, 63, 64, 65, 200]
IDENT = O.affine_to_wire([(0, 1)])[0]
# (name, k, forced G): k = 9 at G = 8 is one full part and a ragged part of one base; k = 17 takes the
# rule's G (1 at these m); k = 130 reads a handle of 40 bases through indices that repeat and are unordered
CONFIGS = {"k9_g8": (9, 8), "k17": (17, 0), "k130_indexed": (130, 0)}
WIDTHS = [(2, 256), (5, 251), (8, 64), (5, 1), (8, 256), (2, 64)]


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def _src_wire():
    pts = M.gen_points(NSRC, k0=5, step=11)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _src():
    return M.Bases.from_wire(_src_wire(), levels=1)


@functools.lru_cache(maxsize=None)
def _indices(name):
    k = CONFIGS[name][0]
    if name == "k130_indexed":
        rnd = random.Random(130)
        return tuple(rnd.randrange(NSRC) for _ in range(k))
    return tuple(range(3, 3 + k))


@pytest.fixture
def group():
    """Sets the bases per part for one test and restores the rule."""
    yield M._test_vector_group
    M._test_vector_group(0)


def _rows(k, b, m, seed):
    """m rows of k scalars below 2^b as Python ints: random ones, and the special rows at the lanes and
    blocks the sizes in MS end on."""
    rnd = random.Random(seed)
    top = (1 << b) - 1
    rows = [[rnd.getrandbits(b) for _ in range(k)] for _ in range(m)]
    for i in (0, 65, 130):          # all zero: the identity, nothing gathered
        if i < m:
            rows[i] = [0] * k
    for i in (1, 64, 198):          # 2^b - 1 everywhere: a carry through every window into the top one
        if i < m:
            rows[i] = [top] * k
    for i in (2, 62, 199):          # one scalar, in the last base (the ragged part's last)
        if i < m:
            rows[i] = [0] * (k - 1) + [rnd.getrandbits(b) | 1]
    return rows


def _expect(wire_bases, rows):
    """The oracle's MSM of every row over the k bases, as wire records."""
    k = wire_bases.shape[0]
    out = []
    for row in rows:
        assert len(row) == k
        out.append(O.msm(wire_bases, O.ints_to_be_words(row), window=4, threads=1))
    return O.affine_to_wire(out)


def _call(t, rows, b):
    flat = [s for r in rows for s in r]
    return t.mul(flat) if b == 256 else t.mul(flat, scalar_bits=b)


# ---- shapes, window widths, scalar widths, special rows -----------------------------------------------
@pytest.mark.parametrize("w,b", WIDTHS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_rows_match_the_oracle(name, w, b, group):
    k, forced = CONFIGS[name]
    idx = np.array(_indices(name), np.uint32)
    bases = _src_wire()[idx]
    rows = _rows(k, b, max(MS), seed=1000 * k + 10 * w + b)
    want = _expect(bases, rows)
    assert np.array_equal(want[0], IDENT) and np.array_equal(want[65], IDENT)
    group(forced)
    plan = M._test_vector_plan(k, w, b, 200, (b + 31) // 32)
    assert (plan["G"], plan["P"]) == ((8, 2) if forced else (1, k))
    with _src().vector_table(indices=idx, window_bits=w, scalar_bits=b) as t:
        inf = t.info
        assert (inf["bases"], inf["window_bits"], inf["scalar_bits"]) == (k, w, b)
        assert inf["windows"] == -(-(b + 1) // w) and inf["records"] == k * inf["windows"] << (w - 1)
        for m in MS:
            got = _call(t, rows[:m], b)
            assert got.shape == (m, 32) and np.array_equal(got, want[:m]), (name, w, b, m)


def test_a_narrow_call_on_a_wide_table(group):
    k, m = 17, 65
    idx = np.array(_indices("k17"), np.uint32)
    rows = _rows(k, 64, m, seed=64)
    want = _expect(_src_wire()[idx], rows)
    flat = [s for r in rows for s in r]
    with _src().vector_table(indices=idx, window_bits=5, scalar_bits=256) as t:
        for forced in (0, 8, 3):
            group(forced)
            assert np.array_equal(t.mul(flat, scalar_bits=64), want), forced
            assert np.array_equal(t.mul(flat), want), forced  # the same integers as 8-word scalars
    # an 8-word call on a 64-bit table is read at the table's width
    with _src().vector_table(indices=idx, window_bits=5, scalar_bits=64) as t64:
        assert np.array_equal(t64.mul(flat), want)
        with pytest.raises(M.MsmError) as e:
            t64.mul(M.scalars_to_wire([1] * k, scalar_bits=65), scalar_bits=65)
        assert e.value.code == -1


def test_auto_width_and_a_range():
    k, m = 12, 70
    rows = _rows(k, 64, m, seed=12)
    with _src().vector_table(first=7, count=k, scalar_bits=64) as t:
        assert t.info["window_bits"] == 12 and t.info["windows"] == 6  # the widest that fits: 18 MiB
        assert np.array_equal(_call(t, rows, 64), _expect(_src_wire()[7:7 + k], rows))


# ---- parts that cancel and parts that coincide --------------------------------------------------------
def test_cancelling_and_equal_parts(group):
    pts = [O.words_xy(r) for r in _src_wire()[:17]]
    pts[8] = ((P - pts[0][0]) % P, pts[0][1])  # -B_0, in the second part of eight
    pts[9] = pts[1]                             # B_1 again
    pts[16] = pts[2]                            # and B_2 again, in the ragged part
    wire = O.affine_to_wire(pts)
    rnd = random.Random(8)
    s = [rnd.getrandbits(256) for _ in range(4)]
    rows = [
        [s[0]] + [0] * 7 + [s[0]] + [0] * 8,                  # P' + (-P'): the identity out of the fold
        [0, s[1]] + [0] * 7 + [s[1]] + [0] * 7,               # P' + P': the fold doubles
        [0, 0, s[2]] + [0] * 13 + [s[2]],                     # the same across the ragged part
        [s[0], s[1], s[2]] + [0] * 5 + [s[0], s[1]] + [0] * 6 + [s[2]],
        [s[3]] * 17,
    ]
    want = _expect(wire, rows)
    assert np.array_equal(want[0], IDENT)
    assert O.words_xy(want[1]) == O.c_scalar_mul(pts[1], 2 * s[1] % O.R_ORDER)
    with M.Bases.from_wire(wire, levels=1) as b, b.vector_table(window_bits=5) as t:
        for forced in (8, 1, 4):
            group(forced)
            assert np.array_equal(_call(t, rows, 256), want), forced


# ---- three fold passes --------------------------------------------------------------------------------
def test_three_fold_passes():
    k, m, b, w = 600, 3, 64, 4
    plan = M._test_vector_plan(k, w, b, m, 2)
    assert (plan["G"], plan["P"], plan["passes"]) == (1, 600, 3)  # 600 -> 38 -> 3 -> 1
    assert plan["bytes"] == 600 * 17 * 8 * 128                    # about 10 MiB
    wire = M.gen_points(k, k0=9, step=2)
    rows = _rows(k, b, m, seed=600)
    rows[0] = [random.Random(6).getrandbits(b) for _ in range(k)]  # (no special row among three)
    with M.Bases.from_wire(wire, levels=1) as bs, bs.vector_table(window_bits=w, scalar_bits=b) as t:
        assert np.array_equal(_call(t, rows, b), _expect(wire, rows))


# ---- two slabs ----------------------------------------------------------------------------------------
def test_slabs_give_the_same_records():
    k, m = 17, 200
    idx = np.array(_indices("k17"), np.uint32)
    rows = _rows(k, 256, m, seed=17)
    with _src().vector_table(indices=idx, window_bits=8) as t:
        whole = _call(t, rows, 256)
        try:
            M._test_vector_slab(400_000)
            assert M._test_vector_plan(k, 8, 256, m, 8)["slab_rows"] == 128  # 128 + 72 rows
            slabbed = _call(t, rows, 256)
            M._test_vector_slab(1)
            assert M._test_vector_plan(k, 8, 256, m, 8)["slab_rows"] == 64   # four slabs
            four = _call(t, rows, 256)
        finally:
            M._test_vector_slab(0)
    assert np.array_equal(slabbed, whole) and np.array_equal(four, whole)
    assert np.array_equal(whole, _expect(_src_wire()[idx], rows))


# ---- entries ------------------------------------------------------------------------------------------
def test_entries_agree(group):
    import torch

    k, m = 17, 130
    idx = np.array(_indices("k17"), np.uint32)
    rows = _rows(k, 256, m, seed=171)
    sc = O.ints_to_be_words([s for r in rows for s in r]).reshape(m, k, 8)
    want = _expect(_src_wire()[idx], rows)
    msm_sc = M.gen_scalars(m, seed=3)
    with _src().vector_table(indices=idx, window_bits=5) as t:
        for forced in (0, 8):
            group(forced)
            assert np.array_equal(t.mul(sc), want)
            d_out = torch.zeros((m, 32), dtype=torch.int32, device="cuda")
            t.mul_device(_dev(sc), d_out)
            assert np.array_equal(_host(d_out), want)
        # narrow scalars in a slice that is only 4-byte aligned: the word-by-word staging
        vals = [[s & ((1 << 128) - 1) for s in r] for r in rows]
        narrow = M.scalars_to_wire([s for r in vals for s in r], scalar_bits=128)
        d_pad = _dev(np.concatenate([np.zeros(1, np.uint32), narrow.reshape(-1)]))
        d_out = torch.zeros((m, 32), dtype=torch.int32, device="cuda")
        t.mul_device(d_pad.data_ptr() + 4, d_out, m=m, scalar_bits=128)
        assert np.array_equal(_host(d_out), _expect(_src_wire()[idx], vals))
        # created handles: the handle the returned records make, level by level
        with M.Bases.from_wire(want, levels=2, window_size=13) as ref:
            recs = [M._test_bases_records(ref, j) for j in range(2)]
            info = ref.info
        exp = O.msm(want, msm_sc, window=10, threads=8)
        for make in (lambda: t.mul_bases(sc, levels=2, window_size=13),
                     lambda: t.mul_bases_device(_dev(sc), m, levels=2, window_size=13)):
            with make() as nb:
                assert nb.info == info
                for j in range(2):
                    assert np.array_equal(M._test_bases_records(nb, j), recs[j]), j
                assert nb.compute(msm_sc) == exp


def test_a_stray_bit_fails_the_device_call_and_the_table_lives():
    k, m, bits = 17, 100, 33
    idx = np.array(_indices("k17"), np.uint32)
    rows = _rows(k, bits, m, seed=33)
    sc = M.scalars_to_wire([s for r in rows for s in r], scalar_bits=bits).copy()
    bad = sc.copy()
    bad[70 * k + 16, 0] |= 2  # bit 33 of row 70's last scalar
    L, vp = M.load(), ctypes.c_void_p
    with _src().vector_table(indices=idx, window_bits=5, scalar_bits=64) as t:
        out = np.full((m, 32), 0xFFFFFFFF, np.uint32)
        rc = L.msm_fixed_mul(t._h, bad.ctypes.data_as(vp), m, M._opts(None, scalar_bits=bits), out.ctypes.data_as(vp))
        assert rc == -1 and np.all(out == 0xFFFFFFFF)  # the host entry: before any work
        d_out = _dev(np.zeros((m, 32), np.uint32))
        with pytest.raises(M.MsmError) as e:
            t.mul_device(_dev(bad), d_out, scalar_bits=bits)  # the device entry: after the launch
        assert e.value.code == -1
        with pytest.raises(M.MsmError) as e:
            t.mul_bases_device(_dev(bad), m, scalar_bits=bits)
        assert e.value.code == -1
        t.mul_device(_dev(sc), d_out, scalar_bits=bits)
        assert np.array_equal(_host(d_out), _expect(_src_wire()[idx], rows))


@pytest.mark.parametrize("k", [1, 8])
def test_small_tables_are_the_fixed_tables(k):
    rnd = random.Random(k)
    rows = [[rnd.getrandbits(64) for _ in range(k)] for _ in range(70)]
    idx = list(range(k, 0, -1))
    with _src().vector_table(indices=idx, window_bits=6, scalar_bits=64) as tv, \
            _src().fixed_table(indices=idx, window_bits=6, scalar_bits=64) as tf:
        assert tv.info == tf.info
        with tv._records_handle() as rv, tf._records_handle() as rf:
            assert np.array_equal(M._test_bases_records(rv, 0), M._test_bases_records(rf, 0))
        got = _call(tv, rows, 64)
        assert np.array_equal(got, _call(tf, rows, 64))
        assert np.array_equal(got, _expect(_src_wire()[idx], rows))


def test_creation_errors():
    b = _src()
    for kw in ({"first": 0, "count": 0}, {"first": 0, "count": NSRC + 1}, {"indices": [NSRC]},
               {"indices": [0] * 4097}, {"first": 0, "count": 9, "window_bits": 1},
               {"first": 0, "count": 9, "window_bits": 17}, {"first": 0, "count": 9, "scalar_bits": 257},
               {"indices": [0] * 4096, "window_bits": 4}):
        with pytest.raises(M.MsmError) as e:
            b.vector_table(**kw)
        assert e.value.code == -1, kw
    with pytest.raises(M.MsmError):  # msm_fixed_create keeps its limit
        b.fixed_table(first=0, count=9)


# ---- guard mode ---------------------------------------------------------------------------------------
def test_guard_bands_stay_clean(group):
    L = M.load()
    k, m = 17, 130
    idx = np.array(_indices("k17"), np.uint32)
    rows = _rows(k, 256, m, seed=5)
    sc = O.ints_to_be_words([s for r in rows for s in r]).reshape(m, k, 8)
    want = _expect(_src_wire()[idx], rows)
    msm_sc = M.gen_scalars(m, seed=5)
    _src.cache_clear()  # the shutdown below frees every live handle's records
    try:
        L.msm_shutdown()
        M._test_guard(True)
        assert "vx_part" in M._test_guard_names() and "sub_idx" in M._test_guard_names()
        with M.Bases.from_wire(_src_wire(), levels=1) as b:
            M._test_guard_release()  # every buffer at this call's own size
            with b.vector_table(indices=idx, window_bits=5) as t:
                assert M._test_guard_check() == []
                for forced in (0, 8):
                    group(forced)
                    M._test_guard_release()
                    assert np.array_equal(t.mul(sc), want)
                    assert M._test_guard_check() == []
                    M._test_guard_release()
                    d_out = _dev(np.zeros((m, 32), np.uint32))
                    t.mul_device(_dev(sc), d_out)
                    assert np.array_equal(_host(d_out), want)
                    assert M._test_guard_check() == []
                M._test_vector_slab(400_000)  # slabs of 128 and 2 rows
                M._test_guard_release()
                assert np.array_equal(t.mul(sc), want)
                assert M._test_guard_check() == []
                M._test_vector_slab(0)
                for make in (lambda: t.mul_bases(sc, levels=2), lambda: t.mul_bases_device(_dev(sc), m, levels=2)):
                    M._test_guard_release()
                    with make() as nb:
                        assert M._test_guard_check() == []
                        assert nb.compute(msm_sc) == O.msm(want, msm_sc, window=10, threads=8)
                narrow = M.scalars_to_wire([1] * (m * k), scalar_bits=33).copy()
                narrow[1000, 0] |= 2  # a failing call: the error word's guards too
                with pytest.raises(M.MsmError):
                    t.mul_device(_dev(narrow), d_out, scalar_bits=33)
                assert M._test_guard_check() == []
                with pytest.raises(M.MsmError):
                    t.mul_bases_device(_dev(narrow), m, scalar_bits=33)
                assert M._test_guard_check() == []
            # a table of odd shape with a ragged part, built into buffers of exactly its size
            M._test_guard_release()
            group(8)
            with b.vector_table(first=1, count=9, window_bits=3, scalar_bits=31) as t3:
                assert M._test_guard_check() == []
                r3 = _rows(9, 31, 65, seed=31)
                assert np.array_equal(_call(t3, r3, 31), _expect(_src_wire()[1:10], r3))
                assert M._test_guard_check() == []
    finally:
        M._test_vector_slab(0)
        L.msm_shutdown()
        M._test_guard(False)
