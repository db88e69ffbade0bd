"""GPU tests of the pairwise combinations of bases handles (include/msm.h msm_bases_combine*,
k_combine_sum, k_combine_one, k_combine_joint): R_i = a_i A_i +- b_i B_i, word for word.

Expected values at any m without a scalar multiplication per point: the bases are P_i = k_i G
(k_i = K0 + i STEP), A_i = P_i and B_i = P_(OFF + i), and the scalars are chosen so that
a_i k_i + b_i k_(OFF + i) = T_i = A0 + i B0 mod r: the result is gen_points(m, k0=A0, step=B0).  Adding a
multiple of r (below 2^256) to a scalar leaves the point and exercises unreduced scalars.  Special points
and scalars go against the oracle's own scalar multiplication and addition."""
import ctypes
import functools
import random

import numpy as np
import pytest

import msm_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

P, R = O.P, O.R_ORDER
I4 = O.sqrt_mod(P - 1)  # sqrt(-1): (I4, 0) has order 4
K0, STEP = 3, 7
A0, B0 = 11, 5
OFF = 1024              # B_i = P_(OFF + i)
MMAX = 1000
N = OFF + MMAX + 76     # the main handle's bases
SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000]  # lane, wave and k_fixed_normalise's 8-block group edges
IDENT = O.affine_to_wire([(0, 1)])[0]
SPECIALS = [0, 1, 2, R - 1, R, R + 1, 1 << 255, (1 << 256) - 1]


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _k(i):
    return K0 + i * STEP


def _words(ints):
    return O.ints_to_be_words(list(ints))


def _affine(rec):
    return (O.be_words_to_int(rec[:8]), O.be_words_to_int(rec[8:16]))


def _lift(s, i):
    """s + j r for every third i, below 2^256: the same point from an unreduced scalar."""
    if i % 3 == 2:
        s += (1 + i % 27) * R
    assert s < 1 << 256
    return s


@functools.lru_cache(maxsize=None)
def _bases():
    pts = M.gen_points(N, k0=K0, step=STEP)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _expected():
    pts = M.gen_points(MMAX, k0=A0, step=B0)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _main():
    return M.Bases.from_wire(_bases(), levels=1)


@functools.lru_cache(maxsize=None)
def _one_scalars():
    """(b_i with A_i + b_i B_i = T_i G, a_i with a_i A_i + B_i = T_i G), i < MMAX."""
    bs = [_lift((A0 + i * B0 - _k(i)) * pow(_k(OFF + i), -1, R) % R, i) for i in range(MMAX)]
    as_ = [_lift((A0 + i * B0 - _k(OFF + i)) * pow(_k(i), -1, R) % R, i) for i in range(MMAX)]
    return _words(bs), _words(as_)


@functools.lru_cache(maxsize=None)
def _joint_scalars():
    """(a_i random 256-bit, b_i with a_i A_i + b_i B_i = T_i G), i < MMAX."""
    rnd = random.Random(1001)
    as_ = [rnd.getrandbits(256) for _ in range(MMAX)]
    bs = [_lift((A0 + i * B0 - a * _k(i)) * pow(_k(OFF + i), -1, R) % R, i) for i, a in enumerate(as_)]
    return _words(as_), _words(bs)


def _oracle(As, Bs, a, b, sub=False):
    """a_i A_i +- b_i B_i by the oracle, as wire records (a, b: ints per point, None for ones)."""
    out = []
    for i, (pa, pb) in enumerate(zip(As, Bs)):
        ta = pa if a is None else O.c_scalar_mul(pa, a[i])
        tb = pb if b is None else O.c_scalar_mul(pb, b[i])
        out.append(O.aff_add(ta, O.aff_neg(tb) if sub else tb))
    return O.affine_to_wire(out)


# ---- sizes at the lane, wave and normalise-group edges, every form -------------------------------------
@pytest.mark.parametrize("m", SIZES)
def test_sum(m):
    got = _main().combine(b_first=OFF, m=m)
    assert got.shape == (m, 32) and got.dtype == np.uint32
    # P_i + P_(OFF + i) = (2 K0 + OFF STEP + 2 i STEP) G: x, y, t = x y, z = 1, every coordinate canonical
    assert np.array_equal(got, M.gen_points(m, k0=2 * K0 + OFF * STEP, step=2 * STEP))


@pytest.mark.parametrize("m", SIZES)
def test_difference(m):
    # P_(2 i + 5) - P_i = (5 + i) STEP G: an indexed side against a range side
    idx = np.arange(m, dtype=np.uint32) * 2 + 5
    got = _main().combine(a_indices=idx, sub=True, m=m)
    assert np.array_equal(got, M.gen_points(m, k0=5 * STEP, step=STEP))
    # and the other way round with the roles swapped: -(P_i - P_(2 i + 5))
    back = _main().combine(b_indices=idx, sub=True, m=m)
    assert [_affine(r) for r in back] == [O.aff_neg(_affine(r)) for r in got]


@pytest.mark.parametrize("m", SIZES)
def test_one_scalar_side(m):
    bs, as_ = _one_scalars()
    assert np.array_equal(_main().combine(b=bs[:m], b_first=OFF), _expected()[:m])
    assert np.array_equal(_main().combine(a=as_[:m], b_first=OFF), _expected()[:m])


@pytest.mark.parametrize("m", SIZES)
def test_joint(m):
    as_, bs = _joint_scalars()
    assert np.array_equal(_main().combine(a=as_[:m], b=bs[:m], b_first=OFF), _expected()[:m])


def test_subtracted_scalar_terms():
    """MSM_COMBINE_SUB with scalars: b_i -> r - b_i gives the same points."""
    m = 257
    as_, bs = _joint_scalars()
    neg = _words([(R - O.be_words_to_int(w) % R) % R for w in bs[:m]])
    assert np.array_equal(_main().combine(a=as_[:m], b=neg, b_first=OFF, sub=True), _expected()[:m])
    bs1, as1 = _one_scalars()
    neg1 = _words([(R - O.be_words_to_int(w) % R) % R for w in bs1[:m]])
    assert np.array_equal(_main().combine(b=neg1, b_first=OFF, sub=True), _expected()[:m])
    # a only, B subtracted: a_i A_i - B_i with B_i = -P = (r - k) G as a point of its own
    a_aff = [_affine(r) for r in _bases()[:64]]
    b_aff = [_affine(r) for r in _bases()[OFF:OFF + 64]]
    a_int = [O.be_words_to_int(w) for w in as1[:64]]
    assert np.array_equal(_main().combine(a=as1[:64], b_first=OFF, sub=True), _oracle(a_aff, b_aff, a_int, None, True))


# ---- special scalars on 64 bases, against the oracle --------------------------------------------------
@functools.lru_cache(maxsize=None)
def _aff64():
    return ([_affine(r) for r in _bases()[:64]], [_affine(r) for r in _bases()[OFF:OFF + 64]])


def test_special_scalar_pairings():
    As, Bs = _aff64()
    a = [SPECIALS[l % 8] for l in range(64)]
    b = [SPECIALS[(l % 8 + l // 8) % 8] for l in range(64)]  # every pairing once
    for sub in (False, True):
        got = _main().combine(a=a, b=b, b_first=OFF, m=64, sub=sub)
        assert np.array_equal(got, _oracle(As, Bs, a, b, sub)), sub
        assert np.array_equal(_main().combine(a=a, b_first=OFF, m=64, sub=sub), _oracle(As, Bs, a, None, sub))
        assert np.array_equal(_main().combine(b=b, b_first=OFF, m=64, sub=sub), _oracle(As, Bs, None, b, sub))
    got = _main().combine(a=a, b=b, b_first=OFF, m=64)
    for l in range(64):
        if a[l] in (0, R) and b[l] in (0, R):
            assert np.array_equal(got[l], IDENT)


def test_single_bits():
    """2^k for every k: in a alone, in b alone and in both (the joint ladder), and alone on a one-sided
    call."""
    As, Bs = _aff64()
    bits = [1 << k for k in range(256)]
    idx = np.arange(256, dtype=np.uint32) % 64
    A4, B4 = [As[i] for i in idx], [Bs[i] for i in idx]
    zeros = [0] * 256
    for a, b in ((bits, zeros), (zeros, bits), (bits, bits)):
        got = _main().combine(a=a, b=b, a_indices=idx, b_indices=idx + OFF)
        assert np.array_equal(got, _oracle(A4, B4, a, b))
    got = _main().combine(a=bits, a_indices=idx, b_indices=idx + OFF)
    assert np.array_equal(got, _oracle(A4, B4, bits, None))


# ---- special points -----------------------------------------------------------------------------------
def test_special_points_in_every_form():
    g, h = _affine(_bases()[5]), _affine(_bases()[9])
    q4r = O.aff_add((I4, 0), _affine(_bases()[2]))  # order 4 r
    assert O.c_scalar_mul(q4r, R) == (I4, 0) or O.c_scalar_mul(q4r, R) == (P - I4, 0)
    pts = [(0, 1), (0, P - 1), (I4, 0), (P - I4, 0), q4r, g, O.aff_neg(g), h]
    ia = np.repeat(np.arange(8, dtype=np.uint32), 8)  # every point as A against every point as B:
    ib = np.tile(np.arange(8, dtype=np.uint32), 8)    # A = B, A = -B and both sides special included
    As, Bs = [pts[i] for i in ia], [pts[i] for i in ib]
    rnd = random.Random(88)
    ks = [0, 1, 2, 3, 4, R - 1, (1 << 255) + 3, (1 << 256) - 1]
    a = [ks[(l + l // 8) % 8] for l in range(64)]
    b = [rnd.choice(ks + [rnd.getrandbits(256)]) for _ in range(64)]
    with M.Bases.from_wire(O.affine_to_wire(pts), levels=1) as s:
        for sub in (False, True):
            kw = dict(a_indices=ia, b_indices=ib, sub=sub)
            assert np.array_equal(s.combine(**kw), _oracle(As, Bs, None, None, sub)), sub
            assert np.array_equal(s.combine(a=a, **kw), _oracle(As, Bs, a, None, sub)), sub
            assert np.array_equal(s.combine(b=b, **kw), _oracle(As, Bs, None, b, sub)), sub
            assert np.array_equal(s.combine(a=a, b=b, **kw), _oracle(As, Bs, a, b, sub)), sub
        diff = s.combine(a_indices=ia, b_indices=ib, sub=True)
        for l in range(64):
            if ia[l] == ib[l]:  # A = B with SUB
                assert np.array_equal(diff[l], IDENT), l
        assert np.array_equal(s.combine(a_indices=ia, b_indices=ib)[5 * 8 + 6], IDENT)  # g + (-g)
        # ones as scalars: the joint table's A + B is then the whole answer, a doubling where A = B
        ones = [1] * 64
        assert np.array_equal(s.combine(a=ones, b=ones, a_indices=ia, b_indices=ib),
                              s.combine(a_indices=ia, b_indices=ib))


def test_bases_given_with_z_not_one():
    n = 140
    pts = np.concatenate([_bases()[:70], _bases()[OFF:OFF + 70]]).copy()
    rnd = random.Random(70)
    for i in (0, 1, 63, 64, 69, 70, 133, 139):
        x, y = _affine(pts[i])
        z = rnd.randrange(2, P)
        pts[i] = np.concatenate([O.int_to_be_words(x * z % P), O.int_to_be_words(y * z % P),
                                 O.int_to_be_words(x * y % P * z % P), O.int_to_be_words(z)])
    as_, bs = _joint_scalars()
    with M.Bases.from_wire(pts, levels=1) as b:
        assert n == b.info["n"]
        assert np.array_equal(b.combine(a=as_[:70], b=bs[:70], b_first=70), _expected()[:70])
        assert np.array_equal(b.combine(b=_one_scalars()[0][:70], b_first=70), _expected()[:70])
        assert np.array_equal(b.combine(b_first=70, m=70), _main().combine(b_first=OFF, m=70))


def test_a_folded_source_is_read_at_level_0():
    as_, bs = _joint_scalars()
    pts = np.concatenate([_bases()[:150], _bases()[OFF:OFF + 150]])
    with M.Bases.from_wire(pts, levels=2, window_size=13) as b2:
        assert b2.info["levels"] == 2
        assert np.array_equal(b2.combine(a=as_[:150], b=bs[:150], b_first=150), _expected()[:150])
        assert np.array_equal(b2.combine(b=_one_scalars()[0][:150], b_first=150), _expected()[:150])
        assert np.array_equal(b2.combine(b_first=150, m=150), _main().combine(b_first=OFF, m=150))


def test_two_handles_of_different_sizes():
    as_, bs = _joint_scalars()
    with M.Bases.from_wire(_bases()[:300], levels=1) as ha, M.Bases.from_wire(_bases()[OFF:OFF + 130], levels=2, window_size=13) as hb:
        # A a range of the larger handle, B an index list into the smaller one
        idx = np.arange(100, dtype=np.uint32) + 20
        got = ha.combine(hb, a=as_[20:120], b=bs[20:120], a_first=20, b_indices=idx)
        assert np.array_equal(got, _expected()[20:120])
        assert np.array_equal(ha.combine(hb, a_first=20, b_first=20, m=100), _main().combine(a_first=20, b_first=OFF + 20, m=100))
        # the roles the other way round: hb's points as A
        got = hb.combine(ha, a=bs[:130], b=as_[:130])
        assert np.array_equal(got, _expected()[:130])
        # an index that only the larger handle has
        with pytest.raises(M.MsmError) as e:
            ha.combine(hb, b_indices=np.array([0, 130], np.uint32))
        assert e.value.code == -1
        with pytest.raises(M.MsmError) as e:
            ha.combine(hb, b_first=31, m=100)
        assert e.value.code == -1


# ---- narrow scalars -----------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 8, 33, 64, 128, 253, 254])
def test_narrow_scalars_equal_the_wide_call(bits):
    m = 257
    rnd = random.Random(bits)
    a = [rnd.getrandbits(bits) for _ in range(m)]
    b = [rnd.getrandbits(bits) for _ in range(m)]
    a[0], a[1], a[64], a[256] = (1 << bits) - 1, 0, 1 << (bits - 1), (1 << bits) - 1
    b[0], b[1], b[64], b[255] = (1 << bits) - 1, 0, 1 << (bits - 1), (1 << bits) - 1
    h = _main()
    na, nb = M.scalars_to_wire(a, scalar_bits=bits), M.scalars_to_wire(b, scalar_bits=bits)
    assert na.shape == (m, (bits + 31) // 32)
    got = h.combine(a=na, b=nb, b_first=OFF, scalar_bits=bits)
    assert np.array_equal(got, h.combine(a=_words(a), b=_words(b), b_first=OFF))
    assert np.array_equal(got[1], IDENT)
    for i in (0, 64, 256):
        pa, pb = _affine(_bases()[i]), _affine(_bases()[OFF + i])
        assert _affine(got[i]) == O.aff_add(O.c_scalar_mul(pa, a[i]), O.c_scalar_mul(pb, b[i]))
    for sub in (False, True):
        assert np.array_equal(h.combine(a=na, b_first=OFF, scalar_bits=bits, sub=sub),
                              h.combine(a=_words(a), b_first=OFF, sub=sub))
        assert np.array_equal(h.combine(b=nb, b_first=OFF, scalar_bits=bits, sub=sub),
                              h.combine(b=_words(b), b_first=OFF, sub=sub))


def test_a_bit_above_the_width_is_refused():
    m, bits = 257, 33
    L = M.load()
    vp = ctypes.c_void_p
    rnd = random.Random(33)
    sa = M.scalars_to_wire([rnd.getrandbits(bits) for _ in range(m)], scalar_bits=bits).copy()
    sb = M.scalars_to_wire([rnd.getrandbits(bits) for _ in range(m)], scalar_bits=bits).copy()
    bad = sa.copy()
    bad[200, 0] |= 2  # bit 33
    with M.Bases.from_wire(_bases()[:300], levels=1) as ha, M.Bases.from_wire(_bases()[OFF:OFF + 300], levels=1) as hb:
        exp = ha.combine(hb, a=sa, b=sb, scalar_bits=bits)
        d_out = _dev(np.zeros((m, 32), np.uint32))
        for kw in (dict(a=bad, b=sb), dict(a=sa, b=bad), dict(a=bad), dict(b=bad)):
            # the host entries: before any work
            out = np.full((m, 32), 0xFFFFFFFF, np.uint32)
            cb, keep, _ = ha._combine_args(hb, kw.get("a"), kw.get("b"), 0, 0, None, None, m, False, bits, True)
            rc = L.msm_bases_combine(ha._h, ctypes.byref(cb), M._opts(None, scalar_bits=bits), out.ctypes.data_as(vp))
            assert rc == -1 and np.all(out == 0xFFFFFFFF)
            with pytest.raises(M.MsmError) as e:
                ha.combined(hb, scalar_bits=bits, **kw)
            assert e.value.code == -1
            # the device entries: after the launch
            dkw = {k: _dev(v) for k, v in kw.items()}
            with pytest.raises(M.MsmError) as e:
                ha.combine_device(d_out, hb, scalar_bits=bits, **dkw)
            assert e.value.code == -1
            with pytest.raises(M.MsmError) as e:
                ha.combined_device(hb, scalar_bits=bits, **dkw)
            assert e.value.code == -1
        # a broadcast scalar's stray bit
        with pytest.raises(M.MsmError) as e:
            ha.combine_device(d_out, hb, a=_dev(bad[200:201]), b=_dev(sb), a_broadcast=True, scalar_bits=bits)
        assert e.value.code == -1
        assert M._test_guard_check() == []
        # and both handles still work
        ha.combine_device(d_out, hb, a=_dev(sa), b=_dev(sb), scalar_bits=bits)
        assert np.array_equal(_host(d_out), exp)
        msm_sc = M.gen_scalars(300, seed=5)
        assert ha.compute(msm_sc) == O.msm(_bases()[:300], msm_sc, window=10, threads=8)
        assert hb.compute(msm_sc) == O.msm(_bases()[OFF:OFF + 300], msm_sc, window=10, threads=8)


# ---- subsets ------------------------------------------------------------------------------------------
def test_subset_forms_mix():
    as_, bs = _joint_scalars()
    h = _main()
    m = 130
    ia, ib = np.arange(m, dtype=np.uint32) + 7, np.arange(m, dtype=np.uint32) + OFF + 7
    exp = _expected()[7:7 + m]
    a, b = as_[7:7 + m], bs[7:7 + m]
    assert np.array_equal(h.combine(a=a, b=b, a_first=7, b_first=OFF + 7), exp)       # range x range
    assert np.array_equal(h.combine(a=a, b=b, a_first=7, b_indices=ib), exp)          # range x indexed
    assert np.array_equal(h.combine(a=a, b=b, a_indices=ia, b_first=OFF + 7), exp)    # indexed x range
    assert np.array_equal(h.combine(a=a, b=b, a_indices=ia, b_indices=ib), exp)       # indexed x indexed
    one = _one_scalars()[0][7:7 + m]
    assert np.array_equal(h.combine(b=one, a_first=7, b_indices=ib), exp)
    assert np.array_equal(h.combine(b=one, a_indices=ia, b_first=OFF + 7), exp)
    assert np.array_equal(h.combine(a_indices=ia, b_indices=ib), h.combine(a_first=7, b_first=OFF + 7, m=m))
    # the handle's last base on both sides
    last = h.combine(a_first=N - 1, b_first=N - 1, m=1)
    assert _affine(last[0]) == O.c_point_double(_affine(_bases()[N - 1]))


def test_indices_repeat_and_m_exceeds_n():
    as_, bs = _joint_scalars()
    rnd = random.Random(400)
    with M.Bases.from_wire(np.concatenate([_bases()[:100], _bases()[OFF:OFF + 100]]), levels=1) as h:
        j = np.array([rnd.randrange(100) for _ in range(400)], np.uint32)  # repeats, m = 400 > n = 200
        j[:4] = [99, 0, 99, 0]
        got = h.combine(a=as_[j], b=bs[j], a_indices=j, b_indices=j + 100)
        assert np.array_equal(got, _expected()[j])
        assert np.array_equal(h.combine(a_indices=j, b_indices=j + 100),
                              _main().combine(a_indices=j, b_indices=j + OFF))


def test_bad_indices_fail_as_stray_bits_do():
    h = _main()
    L = M.load()
    vp = ctypes.c_void_p
    m = 130
    as_, bs = _joint_scalars()
    good = np.arange(m, dtype=np.uint32)
    bad = good.copy()
    bad[77] = N
    d_out = _dev(np.zeros((m, 32), np.uint32))
    for kw in (dict(a_indices=bad), dict(b_indices=bad), dict(a_indices=bad, b_indices=good)):
        for sc in (dict(), dict(b=bs[:m]), dict(a=as_[:m], b=bs[:m])):
            out = np.full((m, 32), 0xFFFFFFFF, np.uint32)
            cb, keep, _ = h._combine_args(None, sc.get("a"), sc.get("b"), 0, 0, kw.get("a_indices"), kw.get("b_indices"),
                                          m, False, None, True)
            assert L.msm_bases_combine(h._h, ctypes.byref(cb), None, out.ctypes.data_as(vp)) == -1
            assert np.all(out == 0xFFFFFFFF)
            dkw = {k: _dev(v) for k, v in {**kw, **sc}.items()}
            with pytest.raises(M.MsmError) as e:
                h.combine_device(d_out, m=m, **dkw)
            assert e.value.code == -1
            with pytest.raises(M.MsmError) as e:
                h.combined_device(m=m, **dkw)
            assert e.value.code == -1
    h.combine_device(d_out, a=_dev(as_[:m]), b=_dev(bs[:m]), a_indices=_dev(good), b_first=OFF)
    assert np.array_equal(_host(d_out), _expected()[:m])
    # first + m > n, an index list with first != 0, a.m != b.m
    for kw in (dict(a_first=N - m + 1), dict(b_first=N - m + 1), dict(b_first=1 << 40), dict(a_first=1, a_indices=good),
               dict(b_first=1, b_indices=good)):
        with pytest.raises(M.MsmError) as e:
            h.combine(m=m, **kw)
        assert e.value.code == -1
        with pytest.raises(M.MsmError) as e:
            h.combined(m=m, **kw)
        assert e.value.code == -1
    cb, keep, _ = h._combine_args(None, None, None, 0, 0, None, None, m, False, None, True)
    cb.b.m = m - 1
    out = np.zeros((m, 32), np.uint32)
    assert L.msm_bases_combine(h._h, ctypes.byref(cb), None, out.ctypes.data_as(vp)) == -1


# ---- broadcast ----------------------------------------------------------------------------------------
def test_broadcast_equals_the_repeated_scalar():
    h = _main()
    m = 257
    rnd = random.Random(77)
    x, y = rnd.getrandbits(256), rnd.getrandbits(256)
    as_, bs = _joint_scalars()
    rx, ry = _words([x] * m), _words([y] * m)
    for sub in (False, True):
        kw = dict(b_first=OFF, m=m, sub=sub)
        assert np.array_equal(h.combine(a=x, b=bs[:m], **kw), h.combine(a=rx, b=bs[:m], **kw))
        assert np.array_equal(h.combine(a=as_[:m], b=y, **kw), h.combine(a=as_[:m], b=ry, **kw))
        assert np.array_equal(h.combine(a=x, b=y, **kw), h.combine(a=rx, b=ry, **kw))
        assert np.array_equal(h.combine(a=x, **kw), h.combine(a=rx, **kw))
        assert np.array_equal(h.combine(b=y, **kw), h.combine(b=ry, **kw))
    pa, pb = _affine(_bases()[256]), _affine(_bases()[OFF + 256])
    got = h.combine(a=x, b=y, b_first=OFF, m=m)
    assert _affine(got[256]) == O.aff_add(O.c_scalar_mul(pa, x), O.c_scalar_mul(pb, y))


def test_narrow_broadcast_is_a_progression():
    # x P_i + y P_(OFF + i) = (x K0 + y (K0 + OFF STEP) + i STEP (x + y)) G, k0 and step below 2^64
    x, y, m = 0xBEEF, 0x1234, 513
    k0, step = x * K0 + y * (K0 + OFF * STEP), STEP * (x + y)
    assert k0 < 1 << 64 and step < 1 << 64
    exp = M.gen_points(m, k0=k0, step=step)
    assert np.array_equal(_main().combine(a=x, b=y, b_first=OFF, m=m, scalar_bits=16), exp)
    assert np.array_equal(_main().combine(a=x, b=y, b_first=OFF, m=m), exp)
    k0, step = K0 + y * (K0 + OFF * STEP), STEP * (1 + y)
    assert np.array_equal(_main().combine(b=y, b_first=OFF, m=m, scalar_bits=16), M.gen_points(m, k0=k0, step=step))


# ---- consistency with the scale entries ---------------------------------------------------------------
def test_combine_is_the_sum_of_two_scale_calls():
    h = _main()
    as_, bs = _joint_scalars()
    sa = h.scale(as_[:64], first=0)
    sb = h.scale(bs[:64], first=OFF)
    exp = O.affine_to_wire([O.aff_add(_affine(p), _affine(q)) for p, q in zip(sa, sb)])
    assert np.array_equal(h.combine(a=as_[:64], b=bs[:64], b_first=OFF), exp)
    assert np.array_equal(exp, _expected()[:64])


@pytest.mark.parametrize("levels", [1, 2])
def test_fold_is_combined_on_the_two_halves(levels):
    n = 300
    rnd = random.Random(300)
    x = rnd.randrange(1, R)
    xi = pow(x, -1, R)
    with M.Bases.from_wire(_bases()[:n], levels=1) as h:
        for kw, a in ((dict(x_inv=xi), xi), (dict(), None)):
            wire = h.combine(a=a, b=x, b_first=n // 2, m=n // 2)
            # (xi k_i + x k_(i + n/2)) G, against the oracle at the ends
            for i in (0, n // 2 - 1):
                pa, pb = _affine(_bases()[i]), _affine(_bases()[i + n // 2])
                assert _affine(wire[i]) == O.aff_add(O.c_scalar_mul(pa, 1 if a is None else a), O.c_scalar_mul(pb, x))
            with h.fold(x, levels=levels, window_size=13, **kw) as f, \
                    h.combined(a=a, b=x, b_first=n // 2, m=n // 2, levels=levels, window_size=13) as c:
                assert f.info == c.info and f.info["n"] == n // 2
                for j in range(levels):
                    assert np.array_equal(M._test_bases_records(f, j), M._test_bases_records(c, j))
                assert np.array_equal(f.points(), wire)
    with M.Bases.from_wire(_bases()[:7], levels=1) as odd:
        with pytest.raises(ValueError):
            odd.fold(x)


# ---- created handles ----------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2])
def test_a_created_handle_is_the_wire_handle_of_the_combined_points(levels):
    src = _main()
    as_, bs = _joint_scalars()
    one = _one_scalars()[0]
    rnd = random.Random(17)
    idx = np.array([rnd.randrange(300) for _ in range(200)], np.uint32)
    cases = [
        ("joint", dict(a=as_[:300], b=bs[:300], b_first=OFF), _expected()[:300]),
        ("one", dict(b=one[5:135], a_first=5, b_first=OFF + 5), _expected()[5:135]),
        ("indexed", dict(a=as_[idx], b=bs[idx], a_indices=idx, b_indices=idx + OFF), _expected()[idx]),
        ("sum", dict(b_first=OFF, m=300), None),
    ]
    for what, kw, exp_pts in cases:
        wire = src.combine(**kw)
        if exp_pts is not None:
            assert np.array_equal(wire, exp_pts)
        m = wire.shape[0]
        with M.Bases.from_wire(wire, levels=levels, window_size=13) as ref:
            want = [M._test_bases_records(ref, j) for j in range(levels)]
            info = ref.info
        msm_sc = M.gen_scalars(m, seed=31)
        exp = O.msm(wire, msm_sc, window=10, threads=8)
        dkw = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        for make in (lambda: src.combined(levels=levels, window_size=13, **kw),
                     lambda: src.combined_device(levels=levels, window_size=13, **dkw)):
            with make() as b:
                assert b.info == info, what
                for j in range(levels):
                    assert np.array_equal(M._test_bases_records(b, j), want[j]), (what, j)
                assert b.compute(msm_sc) == exp
                assert np.array_equal(b.points(), wire), what


# ---- device entries -----------------------------------------------------------------------------------
def test_device_entries():
    import torch

    m = 1000
    h = _main()
    as_, bs = _joint_scalars()
    d_a, d_b = _dev(as_), _dev(bs)
    d_out = torch.zeros((m, 32), dtype=torch.int32, device="cuda")
    h.combine_device(d_out, a=d_a, b=d_b, b_first=OFF)
    assert np.array_equal(_host(d_out), _expected())
    # the output feeds the device MSM as it is
    msm_sc = M.gen_scalars(m, seed=41)
    assert M.compute_msm_device(d_out, _dev(msm_sc), m) == O.msm(_expected(), msm_sc, window=10, threads=8)
    d_out.zero_()
    h.combine_device(d_out, b=_dev(_one_scalars()[0]), b_first=OFF)
    assert np.array_equal(_host(d_out), _expected())
    d_out.zero_()
    h.combine_device(d_out, b_first=OFF, m=m)
    assert np.array_equal(_host(d_out), h.combine(b_first=OFF, m=m))
    # indexed, a broadcast side, and narrow scalars in a slice that is only 4-byte aligned
    rnd = random.Random(1000)
    vals = [rnd.getrandbits(64) for _ in range(m)]
    y = rnd.getrandbits(64)
    idx = np.array([rnd.randrange(N) for _ in range(m)], np.uint32)
    narrow = M.scalars_to_wire(vals, scalar_bits=64)
    exp = h.combine(a=narrow, b=y, b_indices=idx, scalar_bits=64)
    for i in (0, 500, 999):
        pa, pb = _affine(_bases()[i]), _affine(_bases()[idx[i]])
        assert _affine(exp[i]) == O.aff_add(O.c_scalar_mul(pa, vals[i]), O.c_scalar_mul(pb, y))
    d_pad = _dev(np.concatenate([np.zeros(1, np.uint32), narrow.reshape(-1)]))
    d_y = _dev(np.concatenate([np.zeros(1, np.uint32), M.scalars_to_wire([y], scalar_bits=64).reshape(-1)]))
    d_out.zero_()
    h.combine_device(d_out, a=d_pad.data_ptr() + 4, b=d_y.data_ptr() + 4, b_broadcast=True, m=m, b_indices=_dev(idx),
                     scalar_bits=64, stream=torch.cuda.current_stream().cuda_stream or M.MSM_STREAM_NULL)
    assert np.array_equal(_host(d_out), exp)
    # misaligned or overlapping pointers: refused from their values
    d_pad8 = _dev(np.concatenate([np.zeros(1, np.uint32), as_.reshape(-1)]))
    d_big = _dev(np.zeros(m * 32 + 4, np.uint32))
    d_idx = _dev(np.arange(m, dtype=np.uint32))
    o = d_out.data_ptr()
    for kw, out_ptr in ((dict(a=d_pad8.data_ptr() + 4, b=d_b.data_ptr()), o),       # 8-word a scalars off by 4
                        (dict(a=d_a.data_ptr(), b=d_pad8.data_ptr() + 4), o),       # b scalars off by 4
                        (dict(b=d_pad8.data_ptr() + 4), o),
                        (dict(a=d_a.data_ptr(), b=d_b.data_ptr()), d_big.data_ptr() + 4),  # the output off by 4
                        (dict(), d_big.data_ptr() + 4),
                        (dict(a=d_a.data_ptr()), d_a.data_ptr()),                  # the output over a's scalars
                        (dict(a=d_a.data_ptr(), b=d_b.data_ptr()), d_b.data_ptr()),  # over b's
                        (dict(b=d_big.data_ptr() + 16 * m), d_big.data_ptr()),     # scalars inside the output
                        (dict(a_indices=d_big.data_ptr() + 64), d_big.data_ptr()),  # an index list inside the output
                        (dict(b_indices=d_out.data_ptr() + 128 * m - 4), o),
                        (dict(a_indices=d_idx.data_ptr() + 2), o),                # index lists off by 2
                        (dict(b_indices=d_idx.data_ptr() + 2), o)):
        with pytest.raises(M.MsmError) as e:
            h.combine_device(out_ptr, m=m, **kw)
        assert e.value.code == -1, kw
    with pytest.raises(M.MsmError) as e:
        h.combined_device(a=d_pad8.data_ptr() + 4, m=m)
    assert e.value.code == -1
    with pytest.raises(M.MsmError) as e:
        h.combined_device(b_indices=d_idx.data_ptr() + 2, m=m)
    assert e.value.code == -1
    assert np.array_equal(_host(d_out), exp)  # no refused call wrote


# ---- empty --------------------------------------------------------------------------------------------
def test_empty_calls():
    h = _main()
    none8 = np.zeros((0, 8), np.uint32)
    assert h.combine(a=none8, b=none8, a_first=3, b_first=N).shape == (0, 32)
    assert h.combine(m=0).shape == (0, 32)
    assert h.combine(a=5, m=0, b_indices=np.zeros(0, np.uint32)).shape == (0, 32)
    h.combine_device(0, m=0, a_first=N)
    for make in (lambda: h.combined(a=none8, b_first=10, levels=2), lambda: h.combined_device(m=0, b_first=10)):
        with make() as e:
            assert e.info["n"] == 0
            assert e.compute(none8) == (0, 1)
            assert e.points().shape == (0, 32)
    with M.Bases.from_wire(np.zeros((0, 32), np.uint32)) as z:
        assert z.combine().shape == (0, 32)
        assert z.combine(h, m=0).shape == (0, 32)
        with z.combined() as e:
            assert e.info["n"] == 0


# ---- guard mode ---------------------------------------------------------------------------------------
def test_guard_bands_stay_clean():
    L = M.load()
    m = 257
    as_, bs = _joint_scalars()
    one = _one_scalars()[0]
    rnd = random.Random(257)
    j = np.array([rnd.randrange(m) for _ in range(m)], np.uint32)
    pts = np.concatenate([_bases()[:m], _bases()[OFF:OFF + m]])
    exp = _expected()[:m]
    msm_sc = M.gen_scalars(m, seed=5)
    _main.cache_clear()  # the shutdown below frees every live handle's records
    try:
        L.msm_shutdown()
        M._test_guard(True)
        with M.Bases.from_wire(pts, levels=1) as b:
            sum_exp = None
            cases = [(dict(a=as_[:m], b=bs[:m], b_first=m), exp),
                     (dict(a=as_[j], b=bs[j], a_indices=j, b_indices=j + m), exp[j]),
                     (dict(b=one[:m], b_first=m), exp),
                     (dict(a=3, b=one[j], a_indices=j, b_indices=j + m, sub=True), None),
                     (dict(b_first=m, m=m), None)]
            for kw, want in cases:
                dkw = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
                if isinstance(kw.get("a"), int):
                    dkw["a"], dkw["a_broadcast"] = _dev(_words([kw["a"]])), True
                M._test_guard_release()  # every buffer at this call's own size
                got = b.combine(**kw)
                assert M._test_guard_check() == []
                if want is not None:
                    assert np.array_equal(got, want)
                M._test_guard_release()
                d_out = _dev(np.zeros((m, 32), np.uint32))
                b.combine_device(d_out, **dkw)
                assert np.array_equal(_host(d_out), got)
                assert M._test_guard_check() == []
                for make in (lambda: b.combined(levels=2, **kw), lambda: b.combined_device(levels=2, **dkw)):
                    with make() as nb:
                        assert M._test_guard_check() == []
                        assert nb.compute(msm_sc) == O.msm(got, msm_sc, window=10, threads=8)
                    M._test_guard_release()
            bad = j.copy()
            bad[256] = 2 * m  # a failing call: the error word's guards too
            with pytest.raises(M.MsmError):
                b.combine_device(_dev(np.zeros((m, 32), np.uint32)), a=_dev(as_[:m]), b=_dev(bs[:m]), a_indices=_dev(bad))
            assert M._test_guard_check() == []
            with pytest.raises(M.MsmError):
                b.combined_device(b=_dev(bs[:m]), b_indices=_dev(bad))
            assert M._test_guard_check() == []
    finally:
        L.msm_shutdown()
        M._test_guard(False)
