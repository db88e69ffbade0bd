"""GPU tests of resident prepared bases (include/msm.h msm_bases_*, msm_amd.Bases): the records
of every level (k_shift_bases) against the oracle's multiples, the scalar cut (k_split_scalars)
against Python slicing, bit-exact parity of folded and unfolded MSMs with the oracle and the closed
form, and the handles' lifetime and error rules."""
import functools
import random

import numpy as np
import pytest

import _fp29_model as F
import msm_amd as M
from _bases_model import check_record_bounds, cut, decode_record, expected_record_values, fold
from _closed_form import as_xy, closed_form
from oracle import oracle as O

pytestmark = pytest.mark.gpu

I4 = O.sqrt_mod(O.P - 1)            # sqrt(-1): (I4, 0) has order 4
SPECIAL = [(0, 1), (0, O.P - 1), (I4, 0), (O.P - I4, 0)]
WIDTHS = (4, 13, 15, 16, 17)
LEVELS = (1, 2, 3, 4, 8)


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


def _projective(pts, i, z):
    x, y = (O.be_words_to_int(pts[i, 8 * j: 8 * j + 8]) for j in range(2))
    for j, v in enumerate((x * z % O.P, y * z % O.P, x * y % O.P * z % O.P, z)):
        pts[i, 8 * j: 8 * j + 8] = O.int_to_be_words(v)


@functools.lru_cache(maxsize=None)
def _points(n):
    """n wire points: multiples of G, with (from n = 255) the small-order points, z != 1 records,
    duplicates and a point beside its negation; at n <= 2 a projective point (and the order-4 one)."""
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
        if n == 2:
            pts[1] = O.affine_to_wire([(I4, 0)])[0]
    pts.setflags(write=False)
    return pts


def _affine(pts):
    out = []
    for row in pts:
        x, y, _, z = (O.be_words_to_int(row[8 * j: 8 * j + 8]) for j in range(4))
        zi = O.inv(z)
        out.append((x * zi % O.P, y * zi % O.P))
    return out


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
def _scalars(n):
    """n scalars: random 256-bit and canonical values, then every edge scalar (as many as fit), with
    equal scalars on the duplicate and on the negated pair."""
    rnd = random.Random(1000 + n)
    ss = [rnd.getrandbits(256) if i % 2 else rnd.randrange(O.R_ORDER) for i in range(n)]
    sp = _special_scalars()
    if n >= 16:
        room = n - 10
        for i, v in enumerate(sp[:room]):
            ss[10 + i] = v
        ss[6] = ss[5]
        ss[8] = ss[7]
    w = O.ints_to_be_words(ss)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _expected(n):
    return O.msm(_points(n), _scalars(n), window=10, threads=8)


# ---- records ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_records_of_every_level(n):
    pts = _points(n)
    aff = _affine(pts)
    with M.Bases.from_wire(pts, levels=3, window_size=13) as b:
        inf = b.info
        Wc, S = fold(13, 3)
        assert (inf["n"], inf["levels"], inf["window_bits"], inf["windows"], inf["chunk_bits"]) == (n, 3, 13, Wc, S)
        assert inf["bytes"] == 3 * n * 128
        lv = [M._test_bases_records(b, j) for j in range(3)]
    ref, err, _ = M._test_records(F.PT_FMT_WIRE, pts)
    assert err == 0 and np.array_equal(lv[0], ref)        # level 0: k_prepare_points' own records
    cur = aff
    for j in range(3):
        if j:
            cur = [O.scalar_mul(p, 1 << S) for p in cur]  # 2^(jS) P
        for i in range(n):
            vals, limbs = decode_record(lv[j][i])
            assert vals == expected_record_values(cur[i]), (j, i)
            check_record_bounds(limbs)
    # every limb of a level's record, from the record below it through k_shift_bases' lane model: the
    # first and last lanes of a wave, of a workgroup, and of the ragged last workgroup
    masks = M._test_wide_masks()
    for j in (1, 2):
        for i in sorted({i for i in (0, 1, 63, 64, 254, 255, n - 1) if i < n}):
            model = F.shift_lane([int(x) for x in lv[j - 1][i]], S, masks)
            assert lv[j][i].tolist() == model, (j, i, lv[j - 1][i].tolist(), lv[j][i].tolist(), model)
    if n >= 16:  # the small-order points reach the identity after two doublings: its record
        assert all(decode_record(lv[1][i])[0] == expected_record_values((0, 1)) for i in (1, 2, 3, 4))


def test_records_of_deep_levels_and_device_points():
    # eight levels from device-resident points; S = 35 at c = 4
    n = 40
    pts = _points(n)
    _, S = fold(4, 8)
    with M.Bases.from_device(_dev(pts), n, levels=8, window_size=4) as b:
        top = M._test_bases_records(b, 7)
    for i, p in enumerate(_affine(pts)):
        vals, limbs = decode_record(top[i])
        assert vals == expected_record_values(O.scalar_mul(p, 1 << (7 * S))), i
        check_record_bounds(limbs)


# ---- the scalar cut ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 257])
@pytest.mark.parametrize("k", [2, 3, 8])
def test_split_scalars(n, k):
    for c in (13, 16, 4):
        _, S = fold(c, k)
        sc = _scalars(257)[10:10 + n] if n < 257 else _scalars(257)
        sc = np.ascontiguousarray(sc).copy()
        sc[0] = O.int_to_be_words((1 << 256) - 1)
        got = M._test_split_scalars(sc, k, S)
        ints = O.be_words_to_ints(sc)
        exp = [cut(s, k, S)[j] for j in range(k) for s in ints]  # element j n + i
        assert O.be_words_to_ints(got) == exp, (c, k, n)


# ---- parity with the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("n", [1, 2, 257, 4097])
def test_parity_with_oracle(n, levels):
    pts = _points(n)
    for c in WIDTHS:
        if n <= 2 and levels > 1:  # too few points for the shared edge scalars: this pair's own
            _, S = fold(c, levels)
            ss = [(1 << S) + 1, (1 << min((levels - 1) * S, 256)) - 1] if n == 2 else [(1 << 256) - 1]
            sc = O.ints_to_be_words(ss)
            exp = O.msm(pts, sc, window=8)
        else:
            sc, exp = _scalars(n), _expected(n)
        with M.Bases.from_wire(pts, levels=levels, window_size=c) as b:
            assert b.compute(sc, window_size=c) == exp, (n, levels, c)
            assert b.compute_device(_dev(sc)) == exp, (n, levels, c)


# ---- parity with the closed form --------------------------------------------------------------------
def test_folded_launch_crosses_a_scatter_chunk():
    n = 8193  # 16,386 virtual points: two k_part_scatter chunks
    pts = M.gen_points(n, k0=5, step=3)
    sc = M.gen_scalars(n, seed=77)
    with M.Bases.from_wire(pts, levels=2) as b:
        assert b.compute(sc) == closed_form(5, 3, sc)


@pytest.mark.parametrize("levels", [1, 2])
def test_many_points(levels):
    n = (1 << 16) + 77
    pts = M.gen_points(n, k0=4, step=9)
    sc = M.gen_scalars(n, seed=13)
    with M.Bases.from_wire(pts, levels=levels) as b:
        assert b.compute(sc) == closed_form(4, 9, sc)
        assert b.compute_device(_dev(sc)) == closed_form(4, 9, sc)


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("flags", [0, M.MSM_FLAG_SERIAL])
def test_many_entries(levels, flags):
    n, count = 3000, 5  # five MSMs: not a multiple of the MSMs per launch
    pts = M.gen_points(n, k0=2, step=5)
    scs = [M.gen_scalars(n, seed=100 + i) for i in range(count)]
    scs[3] = np.zeros((n, 8), np.uint32)  # an all-zero vector: the identity
    exp = [closed_form(2, 5, s) for s in scs]
    assert exp[3] == (0, 1)
    d_pts, d_scs = _dev(pts), [_dev(s) for s in scs]
    shared = [as_xy(r) for r in M.compute_msm_shared_device(d_pts, d_scs, n)]
    assert shared == exp
    with M.Bases.from_device(d_pts, n, levels=levels) as b:
        assert [as_xy(r) for r in b.compute_many_device(d_scs, flags=flags)] == exp
        assert [as_xy(r) for r in b.compute_many(scs, flags=flags)] == exp
        assert [b.compute_device(s) for s in d_scs] == exp
        assert b.compute_many([]).shape == (0, 16) and b.compute_many_device([]).shape == (0, 16)


def test_all_equal_scalars_take_the_skew_joins():
    n = 4097
    pts = M.gen_points(n, k0=1, step=1)
    s = random.Random(3).randrange(O.R_ORDER)
    sc = O.ints_to_be_words([s] * n)
    with M.Bases.from_wire(pts, levels=2) as b:
        assert b.compute(sc) == closed_form(1, 1, sc)


def test_empty_base_vector():
    with M.Bases.from_wire(np.zeros((0, 32), np.uint32), levels=2) as b:
        assert b.info["n"] == 0
        assert b.compute(np.zeros((0, 8), np.uint32)) == (0, 1)


# ---- lifetime and errors ----------------------------------------------------------------------------
def test_two_handles_and_an_existing_entry_between():
    na, nb = 1500, 2600
    pa, pb = M.gen_points(na, k0=3, step=2), M.gen_points(nb, k0=8, step=5)
    sa, sb = M.gen_scalars(na, seed=1), M.gen_scalars(nb, seed=2)
    ea, eb = closed_form(3, 2, sa), closed_form(8, 5, sb)
    d_pb, d_sb = _dev(pb), _dev(sb)
    with M.Bases.from_wire(pa, levels=2) as a, M.Bases.from_wire(pb, levels=1) as b:
        for _ in range(2):
            assert a.compute(sa) == ea
            assert b.compute(sb) == eb
            # an existing entry in between: it prepares its own records in the context's buffer
            assert as_xy(M.compute_msm_shared_device(d_pb, [d_sb], nb)[0]) == eb
            assert M.compute_msm_wire(pa, sa) == ea
        assert a.compute(sa) == ea and b.compute(sb) == eb


def test_concurrent_computes_on_one_handle():
    from concurrent.futures import ThreadPoolExecutor

    n = 2000
    pts = M.gen_points(n, k0=7, step=4)
    scs = [M.gen_scalars(n, seed=60 + i) for i in range(4)]
    exp = [closed_form(7, 4, s) for s in scs]
    with M.Bases.from_wire(pts, levels=2) as b, ThreadPoolExecutor(4) as pool:
        for _ in range(3):  # the calls serialise on the device context; each keeps its own result
            assert list(pool.map(b.compute, scs)) == exp


def test_bad_points_fail_creation_only():
    n = 300
    pts = M.gen_points(n, k0=3, step=2)
    sc = M.gen_scalars(n, seed=4)
    bad = pts.copy()
    bad[257, 24:32] = 0  # z = 0
    with pytest.raises(M.MsmError) as e:
        M.Bases.from_wire(bad, levels=2)
    assert e.value.code == -4
    bad = pts.copy()
    bad[3, 8:16] = O.int_to_be_words(O.P)  # y = p
    with pytest.raises(M.MsmError) as e:
        M.Bases.from_device(_dev(bad), n)
    assert e.value.code == -3
    with M.Bases.from_wire(pts) as b:  # and the next creation is clean
        assert b.compute(sc) == closed_form(3, 2, sc)


def test_use_after_close_and_create_again():
    n = 500
    pts = M.gen_points(n, k0=6, step=1)
    sc = M.gen_scalars(n, seed=8)
    exp = closed_form(6, 1, sc)
    b = M.Bases.from_wire(pts, levels=2)
    assert b.compute(sc) == exp
    b.close()
    b.close()
    for call in (lambda: b.compute(sc), lambda: b.compute_device(_dev(sc)), lambda: b.compute_many([sc]),
                 lambda: b.compute_many_device([_dev(sc)]), lambda: b.info):
        with pytest.raises(M.MsmError) as e:
            call()
        assert e.value.code == -1
    with M.Bases.from_wire(pts, levels=2) as b2:
        assert b2.compute(sc) == exp
    with pytest.raises(M.MsmError) as e:
        b2.compute(sc)
    assert e.value.code == -1


def test_shutdown_frees_live_handles():
    n = 400
    pts = M.gen_points(n, k0=2, step=3)
    sc = M.gen_scalars(n, seed=21)
    exp = closed_form(2, 3, sc)
    b = M.Bases.from_wire(pts, levels=2)
    assert b.compute(sc) == exp
    M.load().msm_shutdown()  # frees the records; the library re-creates what a later call needs
    with pytest.raises(M.MsmError) as e:
        b.compute(sc)
    assert e.value.code == -1
    b.close()  # harmless: the handle is gone already
    del b
    with M.Bases.from_wire(pts, levels=2) as b2:
        assert b2.compute(sc) == exp
    assert M.compute_msm_wire(pts, sc) == exp


def test_creation_limits():
    pts = M.gen_points(8)
    for lv in (9, 100):
        with pytest.raises(M.MsmError) as e:
            M.Bases.from_wire(pts, levels=lv)
        assert e.value.code == -1
    with M.Bases.from_wire(pts, levels=2, window_size=13) as b:
        with pytest.raises(M.MsmError) as e:
            b.compute(M.gen_scalars(8), window_size=14)
        assert e.value.code == -1
        assert b.compute(M.gen_scalars(8), window_size=13) == b.compute(M.gen_scalars(8))
