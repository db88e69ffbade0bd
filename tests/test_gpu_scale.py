"""GPU tests of the per-point scalar multiples of a bases handle (include/msm.h msm_bases_scale*,
k_scale_points): Q_i = s_i P_i, bit-exact.

Expected values at any n without a scalar multiplication per point: the bases are P_i = k_i G
(k_i = K0 + i STEP) and the scalars s_i = (A + i B) / k_i mod r, full-width and pseudo-random, so the
result is gen_points(n, k0=A, step=B) word for word; adding j r (j <= 27, below 2^256) to a scalar
leaves the point and exercises unreduced scalars.  Special points and scalars go against the oracle's
own scalar multiplication."""
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
A, B = 11, 5
NBIG = (1 << 14) + 3
IDENT = O.affine_to_wire([(0, 1)])[0]


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def _bases():
    pts = M.gen_points(NBIG, k0=K0, step=STEP)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _expected():
    pts = M.gen_points(NBIG, k0=A, step=B)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _scalar_ints():
    """s_i with s_i P_i = (A + i B) G; every third one has a multiple of r added."""
    out = []
    for i in range(NBIG):
        s = (A + i * B) * pow(K0 + i * STEP, -1, R) % R
        if i % 3 == 2:
            s += (1 + i % 27) * R
        assert s < 1 << 256
        out.append(s)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _scalars():
    sc = O.ints_to_be_words(list(_scalar_ints()))
    sc.setflags(write=False)
    return sc


def _affine(rec):
    return (O.be_words_to_int(rec[:8]), O.be_words_to_int(rec[8:16]))


def _mul_wire(pts_aff, scalars):
    return O.affine_to_wire([O.c_scalar_mul(p, s) for p, s in zip(pts_aff, scalars)])


@functools.lru_cache(maxsize=None)
def _h300():
    """(scalars, indices, expected points) of the n = 300 handle cases."""
    rnd = random.Random(300)
    idx = np.array([rnd.randrange(300) for _ in range(200)], np.uint32)
    ints = _scalar_ints()
    # s'_k with s'_k P_idx[k] = (A + idx[k] B) G: the scalar of the indexed base
    sc_idx = O.ints_to_be_words([ints[i] for i in idx])
    return idx, sc_idx, _expected()[idx]


# ---- sizes at the lane, wave and workgroup edges ------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, NBIG])
def test_multiples_of_the_generators_points(n):
    with M.Bases.from_wire(_bases()[:n], levels=1) as b:
        got = b.scale(_scalars()[:n])
    assert got.shape == (n, 32) and got.dtype == np.uint32
    # word for word: x, y, t = x y, z = 1, every coordinate canonical
    assert np.array_equal(got, _expected()[:n])


# ---- special scalars ----------------------------------------------------------------------------------
def test_special_scalars():
    specials = [0, 1, 2, R - 1, R, R + 1, 1 << 255, (1 << 256) - 1]
    scalars = []
    for k in range(8):  # each special on eight lanes, between different neighbours
        scalars += specials[k:] + specials[:k]
    scalars += [1 << k for k in range(256)]  # one bit at each window boundary, and inside each window
    assert len(scalars) == 320
    aff = [_affine(r) for r in _bases()[:64]]
    assert aff[0] == O.c_scalar_mul(O.G, K0)
    with M.Bases.from_wire(_bases()[:64], levels=1) as b:
        for c in range(0, 320, 64):
            part = scalars[c:c + 64]
            got = b.scale(part)
            assert np.array_equal(got, _mul_wire(aff, part)), c
            for s, rec in zip(part, got):
                if s in (0, R):
                    assert np.array_equal(rec, IDENT)


# ---- special bases ------------------------------------------------------------------------------------
def test_special_bases():
    g = _affine(_bases()[5])
    bases = [(0, 1), (0, P - 1), (I4, 0), (P - I4, 0), g]
    ks = [0, 1, 2, 3, 4, 5, (1 << 255) + 3]
    idx = np.array([i for i in range(len(bases)) for _ in ks], np.uint32)
    scalars = ks * len(bases)
    with M.Bases.from_wire(O.affine_to_wire(bases), levels=1) as b:
        got = b.scale(scalars, indices=idx)
    assert np.array_equal(got, _mul_wire([bases[i] for i in idx], scalars))
    assert np.array_equal(got[0], IDENT) and np.array_equal(got[len(ks) + 2], IDENT)  # 0 O, 2 (0, -1)


def test_a_base_given_with_z_not_one():
    n = 70
    pts = _bases()[:n].copy()
    rnd = random.Random(70)
    for i in (0, 1, 63, 64, 69):
        x, y = _affine(pts[i])
        z = rnd.randrange(2, P)
        pts[i] = np.concatenate([O.int_to_be_words(x * z % P), O.int_to_be_words(y * z % P),
                                 O.int_to_be_words(x * y % P * z % P), O.int_to_be_words(z)])
    with M.Bases.from_wire(pts, levels=1) as b:
        assert np.array_equal(b.scale(_scalars()[:n]), _expected()[:n])
        assert np.array_equal(b.points(), _bases()[:n])  # normalised: z = 1


# ---- narrow scalars -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _b257():
    return M.Bases.from_wire(_bases()[:257], levels=1)


@pytest.mark.parametrize("bits", [1, 8, 33, 64, 128, 253, 254])
def test_narrow_scalars_equal_the_wide_call(bits):
    n = 257
    rnd = random.Random(bits)
    vals = [rnd.getrandbits(bits) for _ in range(n)]
    vals[0], vals[1], vals[64], vals[256] = (1 << bits) - 1, 0, 1 << (bits - 1), (1 << bits) - 1
    b = _b257()
    narrow = M.scalars_to_wire(vals, scalar_bits=bits)
    assert narrow.shape == (n, (bits + 31) // 32)
    got = b.scale(narrow, scalar_bits=bits)
    assert np.array_equal(got, b.scale(O.ints_to_be_words(vals)))
    for i in (0, 64, 256):
        assert _affine(got[i]) == O.c_scalar_mul(_affine(_bases()[i]), vals[i])
    assert np.array_equal(got[1], IDENT)


def test_a_bit_above_the_width_is_refused():
    n, bits = 257, 33
    L = M.load()
    vp = ctypes.c_void_p
    rnd = random.Random(33)
    vals = [rnd.getrandbits(bits) for _ in range(n)]
    sc = M.scalars_to_wire(vals, scalar_bits=bits).copy()
    exp = _b257().scale(sc, scalar_bits=bits)
    bad = sc.copy()
    bad[200, 0] |= 2  # bit 33
    # the host entry: before any work
    out = np.full((n, 32), 0xFFFFFFFF, np.uint32)
    rc = L.msm_bases_scale(_b257()._h, None, bad.ctypes.data_as(vp), M._opts(None, scalar_bits=bits),
                           out.ctypes.data_as(vp))
    assert rc == -1 and np.all(out == 0xFFFFFFFF)
    assert M._test_guard_check() == []
    with pytest.raises(M.MsmError) as e:
        _b257().scaled(bad, scalar_bits=bits)
    assert e.value.code == -1
    # the device entries: after the launch
    d_out = _dev(np.zeros((n, 32), np.uint32))
    with pytest.raises(M.MsmError) as e:
        _b257().scale_device(_dev(bad), d_out, scalar_bits=bits)
    assert e.value.code == -1
    with pytest.raises(M.MsmError) as e:
        _b257().scaled_device(_dev(bad), scalar_bits=bits)
    assert e.value.code == -1
    # and the handle still computes
    _b257().scale_device(_dev(sc), d_out, scalar_bits=bits)
    assert np.array_equal(_host(d_out), exp)
    msm_sc = M.gen_scalars(n, seed=5)
    assert _b257().compute(msm_sc) == O.msm(_bases()[:n], msm_sc, window=10, threads=8)


# ---- subsets ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _b300():
    return M.Bases.from_wire(_bases()[:300], levels=1)


def test_range_and_indexed_subsets():
    b = _b300()
    assert np.array_equal(b.scale(_scalars()[5:135], first=5), _expected()[5:135])
    assert np.array_equal(b.scale(_scalars()[299:300], first=299), _expected()[299:300])
    rnd = random.Random(400)
    idx = np.array([rnd.randrange(300) for _ in range(400)], np.uint32)  # repeats, m > n
    idx[:4] = [299, 0, 299, 0]
    ints = _scalar_ints()
    got = b.scale([ints[i] for i in idx], indices=idx)
    assert np.array_equal(got, _expected()[idx])


def test_all_zero_indices_are_the_fixed_base_batch():
    rnd = random.Random(64)
    scalars = [rnd.getrandbits(256) for _ in range(64)]
    p0 = _affine(_bases()[0])
    got = _b300().scale(scalars, indices=np.zeros(64, np.uint32))
    assert np.array_equal(got, _mul_wire([p0] * 64, scalars))


def test_subset_errors():
    b = _b300()
    L = M.load()
    vp = ctypes.c_void_p
    sc = np.ascontiguousarray(_scalars()[:130])
    idx = np.arange(130, dtype=np.uint32)
    idx[77] = 300
    out = np.full((130, 32), 0xFFFFFFFF, np.uint32)
    arr = (vp * 1)(idx.ctypes.data)
    sub = M.Subset(0, 130, ctypes.cast(arr, vp))
    # index = n: the host entry before any work, the device entry after the launch
    assert L.msm_bases_scale(b._h, ctypes.byref(sub), sc.ctypes.data_as(vp), None, out.ctypes.data_as(vp)) == -1
    assert np.all(out == 0xFFFFFFFF)
    d_out = _dev(np.zeros((130, 32), np.uint32))
    with pytest.raises(M.MsmError) as e:
        b.scale_device(_dev(sc), d_out, indices=_dev(idx))
    assert e.value.code == -1
    with pytest.raises(M.MsmError) as e:
        b.scaled_device(_dev(sc), indices=_dev(idx))
    assert e.value.code == -1
    idx[77] = 77
    b.scale_device(_dev(sc), d_out, indices=_dev(idx))
    assert np.array_equal(_host(d_out), _expected()[:130])
    # first + m > n, and an index list with first != 0
    for first, indices in ((171, None), (1 << 40, None), (1, idx)):
        with pytest.raises(M.MsmError) as e:
            b.scale(sc, first=first, indices=indices)
        assert e.value.code == -1
        with pytest.raises(M.MsmError) as e:
            b.scaled(sc, first=first, indices=indices)
        assert e.value.code == -1


def test_a_folded_source_is_read_at_level_0():
    idx, sc_idx, exp_idx = _h300()
    with M.Bases.from_wire(_bases()[:300], levels=2, window_size=13) as b2:
        assert np.array_equal(b2.scale(_scalars()[:300]), _expected()[:300])
        assert np.array_equal(b2.scale(_scalars()[5:135], first=5), _expected()[5:135])
        assert np.array_equal(b2.scale(sc_idx, indices=idx), exp_idx)


# ---- created handles ----------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2])
def test_a_created_handle_is_the_wire_handle_of_the_scaled_points(levels):
    idx, sc_idx, exp_idx = _h300()
    src = _b300()
    rnd = random.Random(17)
    cases = [
        ("all", _scalars()[:300], {}, _expected()[:300]),
        ("range", _scalars()[5:135], {"first": 5}, _expected()[5:135]),
        ("indexed", sc_idx, {"indices": idx}, exp_idx),
    ]
    for what, sc, kw, exp_pts in cases:
        m = sc.shape[0]
        wire = src.scale(sc, **kw)
        assert np.array_equal(wire, exp_pts)
        with M.Bases.from_wire(wire, levels=levels, window_size=13) as ref:
            want = [M._test_bases_records(ref, j) for j in range(levels)]
            info = ref.info
        msm_sc = M.gen_scalars(m, seed=31)
        exp = O.msm(exp_pts, msm_sc, window=10, threads=8)
        narrow = [rnd.getrandbits(64) for _ in range(m)]
        exp_narrow = O.msm(exp_pts, O.ints_to_be_words(narrow), window=10, threads=8)
        sub_idx = np.array([rnd.randrange(m) for _ in range(120)], np.uint32)
        exp_sub = O.msm(exp_pts[sub_idx], msm_sc[:120], window=10, threads=8)
        dkw = dict(kw)
        if "indices" in dkw:
            dkw["indices"] = _dev(dkw["indices"])
        for make in (lambda: src.scaled(sc, levels=levels, window_size=13, **kw),
                     lambda: src.scaled_device(_dev(sc), levels=levels, window_size=13, **dkw)):
            with make() as b:
                assert b.info == info, what
                for j in range(levels):
                    assert np.array_equal(M._test_bases_records(b, j), want[j]), (what, j)
                assert b.compute(msm_sc) == exp
                assert b.compute(M.scalars_to_wire(narrow, scalar_bits=64), scalar_bits=64) == exp_narrow
                assert b.compute_subset(msm_sc[:120], indices=sub_idx) == exp_sub
                assert np.array_equal(b.points(), wire), what


def test_points_reads_a_handle_back():
    pts = _bases()[:300]
    assert np.array_equal(_b300().points(), pts)
    assert np.array_equal(_b300().points(first=7, m=100), pts[7:107])
    assert np.array_equal(_b300().points(first=290), pts[290:])
    idx = np.array([299, 0, 0, 64, 63], np.uint32)
    assert np.array_equal(_b300().points(indices=idx), pts[idx])
    with M.Bases.from_x(np.ascontiguousarray(pts[:, :8]), levels=2) as bx:  # no host copy of its y
        assert np.array_equal(bx.points(), pts)


# ---- device entries -----------------------------------------------------------------------------------
def test_device_entries():
    import torch

    n = 1000
    with M.Bases.from_wire(_bases()[:n], levels=1) as b:
        d_sc = _dev(_scalars()[:n])
        d_out = torch.zeros((n, 32), dtype=torch.int32, device="cuda")
        b.scale_device(d_sc, d_out)
        assert np.array_equal(_host(d_out), _expected()[:n])
        # the output feeds the device MSM as it is
        msm_sc = M.gen_scalars(n, seed=41)
        assert M.compute_msm_device(d_out, _dev(msm_sc), n) == O.msm(_expected()[:n], msm_sc, window=10, threads=8)
        # indexed, and narrow scalars in a slice that is only 4-byte aligned
        rnd = random.Random(1000)
        vals = [rnd.getrandbits(64) for _ in range(n)]
        idx = np.array([rnd.randrange(n) for _ in range(n)], np.uint32)
        narrow = M.scalars_to_wire(vals, scalar_bits=64)
        exp = b.scale(narrow, indices=idx, scalar_bits=64)
        for i in (0, 500, 999):
            assert _affine(exp[i]) == O.c_scalar_mul(_affine(_bases()[idx[i]]), vals[i])
        d_pad = _dev(np.concatenate([np.zeros(1, np.uint32), narrow.reshape(-1)]))
        d_out.zero_()
        b.scale_device(d_pad.data_ptr() + 4, d_out, m=n, indices=_dev(idx), scalar_bits=64,
                       stream=torch.cuda.current_stream().cuda_stream or M.MSM_STREAM_NULL)
        assert np.array_equal(_host(d_out), exp)
        # misaligned or overlapping pointers: refused from their values
        d_pad8 = _dev(np.concatenate([np.zeros(1, np.uint32), _scalars()[:n].reshape(-1)]))
        d_big = _dev(np.zeros(n * 32 + 4, np.uint32))
        for sc_ptr, out_ptr in ((d_pad8.data_ptr() + 4, d_out.data_ptr()),       # 8-word scalars off by 4
                                (d_sc.data_ptr(), d_big.data_ptr() + 4),          # the output off by 4
                                (d_sc.data_ptr(), d_sc.data_ptr()),               # the output over the scalars
                                (d_big.data_ptr() + 16 * n, d_big.data_ptr())):  # the scalars inside the output
            with pytest.raises(M.MsmError) as e:
                b.scale_device(sc_ptr, out_ptr, m=n)
            assert e.value.code == -1
        with pytest.raises(M.MsmError) as e:
            b.scaled_device(d_pad8.data_ptr() + 4, m=n)
        assert e.value.code == -1
        with pytest.raises(M.MsmError) as e:
            b.scale_device(d_sc, d_out, indices=d_pad.data_ptr() + 2, m=n)
        assert e.value.code == -1


# ---- empty --------------------------------------------------------------------------------------------
def test_empty_calls():
    b = _b300()
    none8 = np.zeros((0, 8), np.uint32)
    assert b.scale(none8, first=3).shape == (0, 32)
    assert b.scale(none8, indices=np.zeros(0, np.uint32)).shape == (0, 32)
    b.scale_device(0, 0, m=0, first=300)
    for make in (lambda: b.scaled(none8, first=10, levels=2), lambda: b.scaled_device(0, m=0, first=10)):
        with make() as e:
            assert e.info["n"] == 0
            assert e.compute(none8) == (0, 1)
            assert e.points().shape == (0, 32)
    with M.Bases.from_wire(np.zeros((0, 32), np.uint32)) as z:
        assert z.scale(none8).shape == (0, 32)
        with z.scaled(none8) as e:
            assert e.info["n"] == 0


# ---- guard mode ---------------------------------------------------------------------------------------
def test_guard_bands_stay_clean():
    L = M.load()
    n = 257
    pts, sc, exp = _bases()[:n], _scalars()[:n], _expected()[:n]
    rnd = random.Random(257)
    idx = np.array([rnd.randrange(n) for _ in range(n)], np.uint32)
    ints = _scalar_ints()
    sc_idx = O.ints_to_be_words([ints[i] for i in idx])
    msm_sc = M.gen_scalars(n, seed=5)
    _b257.cache_clear()  # the shutdown below frees every live handle's records
    _b300.cache_clear()
    try:
        L.msm_shutdown()
        M._test_guard(True)
        with M.Bases.from_wire(pts, levels=1) as b:
            for s, kw, want in ((sc, {}, exp), (sc_idx, {"indices": idx}, exp[idx])):
                dkw = {k: _dev(v) for k, v in kw.items()}
                M._test_guard_release()  # every buffer at this call's own size
                assert np.array_equal(b.scale(s, **kw), want)
                assert M._test_guard_check() == []
                M._test_guard_release()
                d_out = _dev(np.zeros((n, 32), np.uint32))
                b.scale_device(_dev(s), d_out, **dkw)
                assert np.array_equal(_host(d_out), want)
                assert M._test_guard_check() == []
                for make in (lambda: b.scaled(s, levels=2, **kw), lambda: b.scaled_device(_dev(s), levels=2, **dkw)):
                    with make() as nb:
                        assert M._test_guard_check() == []
                        assert nb.compute(msm_sc) == O.msm(want, msm_sc, window=10, threads=8)
                    M._test_guard_release()
            bad = idx.copy()
            bad[256] = n  # a failing call: the error word's guards too
            with pytest.raises(M.MsmError):
                b.scale_device(_dev(sc_idx), _dev(np.zeros((n, 32), np.uint32)), indices=_dev(bad))
            assert M._test_guard_check() == []
            with pytest.raises(M.MsmError):
                b.scaled_device(_dev(sc_idx), indices=_dev(bad))
            assert M._test_guard_check() == []
    finally:
        L.msm_shutdown()
        M._test_guard(False)
