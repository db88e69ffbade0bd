"""GPU tests of the fixed-base tables (include/msm.h msm_fixed_*; k_fixed_build, k_fixed_eval,
k_fixed_normalise): Q_i = sum_j s_ij B_j, bit-exact.

Expected values at any m without a scalar multiplication per point, as tests/test_gpu_scale.py has
them: the base is B = K0 G and the scalars s_i = (A + i STEP_B) / K0 mod r, so the result is
gen_points(m, k0=A, step=STEP_B) word for word; every third scalar has a multiple of r added (below
2^256).  With k bases k_j G the first k - 1 scalars of a row are random 256-bit integers and the last
one is solved for the same sum.  Special points and scalars go against the oracle's own scalar
multiplication."""
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
K0, STEP = 3, 7         # the bases k_j G, k_j = K0 + j STEP
A, STEP_B = 11, 5       # the results (A + i STEP_B) G
NBIG = (1 << 14) + 3
NORM_E = 8              # k_fixed_normalise takes 64 NORM_E points per workgroup
IDENT = O.affine_to_wire([(0, 1)])[0]


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _affine(rec):
    return (O.be_words_to_int(rec[:8]), O.be_words_to_int(rec[8:16]))


@functools.lru_cache(maxsize=None)
def _gens():
    pts = M.gen_points(8, k0=K0, step=STEP)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _expected():
    pts = M.gen_points(NBIG, k0=A, step=STEP_B)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _rows(k, m=NBIG, seed=0):
    """[m, k, 8] wire scalars with sum_j s_ij (K0 + j STEP) = A + i STEP_B mod r."""
    rnd = random.Random(1000 * k + seed)
    ks = [K0 + j * STEP for j in range(k)]
    inv_last = pow(ks[-1], -1, R)
    out = []
    for i in range(m):
        row = [rnd.getrandbits(256) for _ in range(k - 1)]
        last = (A + i * STEP_B - sum(s * kj for s, kj in zip(row, ks))) * inv_last % R
        if i % 3 == 2:
            last += (1 + i % 27) * R
        assert last < 1 << 256
        out += row + [last]
    sc = O.ints_to_be_words(out).reshape(m, k, 8)
    sc.setflags(write=False)
    return sc


@functools.lru_cache(maxsize=None)
def _src():
    return M.Bases.from_wire(_gens(), levels=1)


@functools.lru_cache(maxsize=None)
def _table(k=1, w=0, b=0):
    return _src().fixed_table(first=0, count=k, window_bits=w, scalar_bits=b)


def _drop_caches():
    _src.cache_clear()
    _table.cache_clear()


def _mul_wire(base, scalars):
    return O.affine_to_wire([O.c_scalar_mul(base, s) for s in scalars])


# ---- sizes at the lane, wave, workgroup and normalise-block edges ------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 64 * NORM_E - 1, 64 * NORM_E, 64 * NORM_E + 1, 577, 1000,
                               NBIG])
def test_multiples_of_one_base(m):
    t = _table()
    assert t.info == {"bases": 1, "window_bits": 12, "scalar_bits": 256, "windows": 22, "records": 22 * 2048,
                      "bytes": 22 * 2048 * 128, "device": _src().info["device"]}
    got = t.mul(_rows(1)[:m])
    assert got.shape == (m, 32) and got.dtype == np.uint32
    # word for word: x, y, t = x y, z = 1, every coordinate canonical
    assert np.array_equal(got, _expected()[:m])


# ---- several bases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m", [(2, 1000), (3, 1000), (8, 257)])
def test_several_bases(k, m):
    assert np.array_equal(_table(k).mul(_rows(k, 1000)[:m]), _expected()[:m])


def test_python_ints_and_nested_rows():
    t = _table(2)
    rnd = random.Random(2)
    rows = [[rnd.getrandbits(256), rnd.getrandbits(256)] for _ in range(5)]
    flat = [s for r in rows for s in r]
    want = t.mul(O.ints_to_be_words(flat).reshape(5, 2, 8))
    assert np.array_equal(t.mul(rows), want) and np.array_equal(t.mul(flat), want)
    g0, g1 = _affine(_gens()[0]), _affine(_gens()[1])
    for r, rec in zip(rows, want):
        assert _affine(rec) == M.point_add_affine(O.c_scalar_mul(g0, r[0]), O.c_scalar_mul(g1, r[1]))
    with pytest.raises(ValueError):
        t.mul(flat[:3])


def test_a_repeated_index_is_the_same_base_twice():
    m = 300
    rnd = random.Random(11)
    # s_i0 B_1 + s_i1 B_0 + s_i2 B_1 with k_1 (s_i0 + s_i2) + k_0 s_i1 = A + i STEP_B
    k0, k1 = K0, K0 + STEP
    out = []
    for i in range(m):
        a, b = rnd.getrandbits(256), rnd.getrandbits(256)
        out += [a, b, ((A + i * STEP_B - a * k1 - b * k0) * pow(k1, -1, R)) % R]
    with _src().fixed_table(indices=[1, 0, 1]) as t:
        assert t.info["bases"] == 3
        assert np.array_equal(t.mul(out), _expected()[:m])


# ---- the table itself ---------------------------------------------------------------------------------
def test_table_read_back():
    with _src().fixed_table(first=0, count=2, window_bits=4, scalar_bits=16) as t:
        inf = t.info
        assert (inf["windows"], inf["records"], inf["bytes"]) == (5, 2 * 5 * 8, 2 * 5 * 8 * 128)
        pts = t.points()
        want = [O.c_scalar_mul(_affine(_gens()[j]), d << (4 * win))
                for j in range(2) for win in range(5) for d in range(1, 9)]
        assert np.array_equal(pts, O.affine_to_wire(want))
        # ordinary prepared records: what a creation makes of those points
        with t._records_handle() as rh, M.Bases.from_wire(pts, levels=1) as ref:
            assert np.array_equal(M._test_bases_records(rh, 0), M._test_bases_records(ref, 0))
    # a handle made from x-coordinates gives the same table
    xs = np.ascontiguousarray(_gens()[:2, :8])
    with M.Bases.from_x(xs, levels=1) as bx, bx.fixed_table(window_bits=4, scalar_bits=16) as tx:
        assert np.array_equal(tx.points(), pts)


# ---- special scalars ----------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [4, 8, 9])
def test_special_scalars(w):
    half = 1 << (w - 1)
    specials = [0, 1, 2, half, half + 1, (1 << w) - 1, R - 1, R, R + 1, 1 << 255, (1 << 256) - 1]
    scalars = []
    for k in range(8):  # each special on eight lanes, between different neighbours
        scalars += specials[k:] + specials[:k]
    scalars += [1 << k for k in range(256)]  # one bit at each window boundary, and inside each window
    g = _affine(_gens()[0])
    assert g == O.c_scalar_mul(O.G, K0)
    got = _table(1, w).mul(scalars)
    assert np.array_equal(got, _mul_wire(g, scalars))
    for s, rec in zip(scalars, got):
        if s in (0, R):
            assert np.array_equal(rec, IDENT)


# ---- special bases ------------------------------------------------------------------------------------
def test_special_bases():
    g = _affine(_gens()[5])
    bases = [(0, 1), (0, P - 1), (I4, 0), (P - I4, 0), g]
    ks = [0, 1, 2, 3, 4, 5, (1 << 255) + 3]
    wire = O.affine_to_wire(bases)
    rnd = random.Random(70)
    z = rnd.randrange(2, P)  # the last base given with z != 1
    wire[4] = np.concatenate([O.int_to_be_words(g[0] * z % P), O.int_to_be_words(g[1] * z % P),
                              O.int_to_be_words(g[0] * g[1] % P * z % P), O.int_to_be_words(z)])
    with M.Bases.from_wire(wire, levels=1) as b:
        for j, base in enumerate(bases):
            with b.fixed_table(indices=[j]) as t:
                got = t.mul(ks)
                assert np.array_equal(got, _mul_wire(base, ks)), j
                assert np.array_equal(got[0], IDENT)
        with b.fixed_table() as t:  # all five at once: the sum of the multiples
            rows = [[rnd.getrandbits(256) for _ in bases] for _ in range(3)]
            for row, rec in zip(rows, t.mul(rows)):
                acc = (0, 1)
                for base, s in zip(bases, row):
                    acc = M.point_add_affine(acc, O.c_scalar_mul(base, s))
                assert _affine(rec) == acc


# ---- widths -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 8, 33, 64, 128, 253, 254])
def test_narrow_scalars_equal_the_wide_call(bits):
    m = 257
    rnd = random.Random(bits)
    vals = [rnd.getrandbits(bits) for _ in range(m)]
    vals[0], vals[1], vals[64], vals[256] = (1 << bits) - 1, 0, 1 << (bits - 1), (1 << bits) - 1
    t = _table()
    narrow = M.scalars_to_wire(vals, scalar_bits=bits)
    assert narrow.shape == (m, (bits + 31) // 32)
    got = t.mul(narrow, scalar_bits=bits)
    assert np.array_equal(got, t.mul(O.ints_to_be_words(vals)))
    g = _affine(_gens()[0])
    for i in (0, 64, 256):
        assert _affine(got[i]) == O.c_scalar_mul(g, vals[i])
    assert np.array_equal(got[1], IDENT)


def test_a_bit_above_the_width_is_refused():
    m, bits = 257, 33
    L = M.load()
    vp = ctypes.c_void_p
    rnd = random.Random(33)
    vals = [rnd.getrandbits(bits) for _ in range(m)]
    sc = M.scalars_to_wire(vals, scalar_bits=bits).copy()
    t = _table()
    exp = t.mul(sc, scalar_bits=bits)
    bad = sc.copy()
    bad[200, 0] |= 2  # bit 33
    # the host entry: before any work
    out = np.full((m, 32), 0xFFFFFFFF, np.uint32)
    rc = L.msm_fixed_mul(t._h, bad.ctypes.data_as(vp), m, M._opts(None, scalar_bits=bits), out.ctypes.data_as(vp))
    assert rc == -1 and np.all(out == 0xFFFFFFFF)
    with pytest.raises(M.MsmError) as e:
        t.mul_bases(bad, scalar_bits=bits)
    assert e.value.code == -1
    # the device entries: after the launch
    d_out = _dev(np.zeros((m, 32), np.uint32))
    with pytest.raises(M.MsmError) as e:
        t.mul_device(_dev(bad), d_out, scalar_bits=bits)
    assert e.value.code == -1
    with pytest.raises(M.MsmError) as e:
        t.mul_bases_device(_dev(bad), m, scalar_bits=bits)
    assert e.value.code == -1
    # and the table still computes
    t.mul_device(_dev(sc), d_out, scalar_bits=bits)
    assert np.array_equal(_host(d_out), exp)


def test_a_table_of_64_bits():
    m = 300
    rnd = random.Random(64)
    vals = [rnd.getrandbits(64) for _ in range(m)]
    vals[:3] = [(1 << 64) - 1, 0, 1 << 63]
    t = _table(1, 8, 64)
    assert t.info["windows"] == 9 and t.info["records"] == 9 * 128
    want = _table().mul(O.ints_to_be_words(vals))
    assert np.array_equal(t.mul(M.scalars_to_wire(vals, scalar_bits=64), scalar_bits=64), want)
    small = [v >> 31 for v in vals]
    assert np.array_equal(t.mul(M.scalars_to_wire(small, scalar_bits=33), scalar_bits=33),
                          _table().mul(O.ints_to_be_words(small)))
    # an 8-word call is read at the table's width
    assert np.array_equal(t.mul(O.ints_to_be_words(vals)), want)
    wide = O.ints_to_be_words(vals).copy()
    wide[7, 5] = 1  # bit 64
    with pytest.raises(M.MsmError) as e:
        t.mul(wide)
    assert e.value.code == -1
    d_out = _dev(np.zeros((m, 32), np.uint32))
    with pytest.raises(M.MsmError) as e:
        t.mul_device(_dev(wide), d_out)
    assert e.value.code == -1
    # a call wider than the table
    for bits in (65, 128, 256):
        with pytest.raises(M.MsmError) as e:
            t.mul(M.scalars_to_wire([1] * 4, scalar_bits=bits), scalar_bits=bits)
        assert e.value.code == -1


# ---- against the ladder -------------------------------------------------------------------------------
def test_equals_scale_with_zero_indices():
    rnd = random.Random(1000)
    sc = O.ints_to_be_words([rnd.getrandbits(256) for _ in range(1000)])
    assert np.array_equal(_table().mul(sc), _src().scale(sc, indices=np.zeros(1000, np.uint32)))


# ---- created handles ----------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2])
def test_a_created_handle_is_the_wire_handle_of_the_points(levels):
    m = 300
    t = _table(2)
    sc = _rows(2, 1000)[:m]
    wire = t.mul(sc)
    assert np.array_equal(wire, _expected()[:m])
    with M.Bases.from_wire(wire, levels=levels, window_size=13) as ref:
        want = [M._test_bases_records(ref, j) for j in range(levels)]
        info = ref.info
    msm_sc = M.gen_scalars(m, seed=31)
    exp = O.msm(wire, msm_sc, window=10, threads=8)
    for make in (lambda: t.mul_bases(sc, levels=levels, window_size=13),
                 lambda: t.mul_bases_device(_dev(sc), m, levels=levels, window_size=13)):
        with make() as b:
            assert b.info == info
            for j in range(levels):
                assert np.array_equal(M._test_bases_records(b, j), want[j]), j
            assert b.compute(msm_sc) == exp
            assert np.array_equal(b.points(), wire)


# ---- device entries -----------------------------------------------------------------------------------
def test_device_entries():
    import torch

    m = 1000
    t = _table()
    sc = np.ascontiguousarray(_rows(1)[:m]).reshape(m, 8)
    d_sc = _dev(sc)
    d_out = torch.zeros((m, 32), dtype=torch.int32, device="cuda")
    t.mul_device(d_sc, d_out)
    assert np.array_equal(_host(d_out), _expected()[:m])
    # the output feeds the device MSM as it is
    msm_sc = M.gen_scalars(m, seed=41)
    assert M.compute_msm_device(d_out, _dev(msm_sc), m) == O.msm(_expected()[:m], msm_sc, window=10, threads=8)
    # a non-default stream, and narrow scalars in a slice that is only 4-byte aligned
    rnd = random.Random(1000)
    vals = [rnd.getrandbits(64) for _ in range(m)]
    narrow = M.scalars_to_wire(vals, scalar_bits=64)
    exp = t.mul(narrow, scalar_bits=64)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_pad = _dev(np.concatenate([np.zeros(1, np.uint32), narrow.reshape(-1)]))
        d_out.zero_()
        t.mul_device(d_pad.data_ptr() + 4, d_out, m=m, scalar_bits=64, stream=side.cuda_stream)
    assert np.array_equal(_host(d_out), exp)
    with torch.cuda.stream(side):
        d_k2 = _dev(_rows(2, 1000))
        d_out.zero_()
        _table(2).mul_device(d_k2, d_out)
    assert np.array_equal(_host(d_out), _expected()[:m])
    # misaligned or overlapping pointers: refused from their values
    d_pad8 = _dev(np.concatenate([np.zeros(1, np.uint32), sc.reshape(-1)]))
    d_big = _dev(np.zeros(m * 32 + 4, np.uint32))
    for sc_ptr, out_ptr in ((d_pad8.data_ptr() + 4, d_out.data_ptr()),       # 8-word scalars off by 4
                            (d_sc.data_ptr(), d_big.data_ptr() + 4),          # the output off by 4
                            (d_sc.data_ptr(), d_sc.data_ptr()),               # the output over the scalars
                            (d_big.data_ptr() + 16 * m, d_big.data_ptr())):  # the scalars inside the output
        with pytest.raises(M.MsmError) as e:
            t.mul_device(sc_ptr, out_ptr, m=m)
        assert e.value.code == -1
    with pytest.raises(M.MsmError) as e:
        t.mul_bases_device(d_pad8.data_ptr() + 4, m)
    assert e.value.code == -1
    with pytest.raises(M.MsmError) as e:
        t.mul_device(d_pad.data_ptr() + 2, d_out, m=m, scalar_bits=64)
    assert e.value.code == -1


# ---- creation errors ----------------------------------------------------------------------------------
def test_creation_errors():
    b = _src()
    for kw in ({"first": 0, "count": 0}, {"first": 0, "count": 9}, {"first": 7, "count": 2}, {"indices": [8]},
               {"indices": [0] * 9}, {"first": 0, "count": 1, "window_bits": 1},
               {"first": 0, "count": 1, "window_bits": 17}, {"first": 0, "count": 1, "scalar_bits": 257},
               {"first": 0, "count": 4, "window_bits": 16}):
        with pytest.raises(M.MsmError) as e:
            b.fixed_table(**kw)
        assert e.value.code == -1, kw
    with b.fixed_table() as t:  # all eight bases
        assert t.info["bases"] == 8
    with M.Bases.from_wire(M.gen_points(9), levels=1) as b9:
        with pytest.raises(M.MsmError):
            b9.fixed_table()


# ---- lifetime -----------------------------------------------------------------------------------------
def test_lifetime():
    L = M.load()
    sc = _rows(1)[:100]
    none8 = np.zeros((0, 8), np.uint32)
    with M.Bases.from_wire(_gens()[:1], levels=1) as b:
        t = b.fixed_table()
    # the source is gone, the table is not
    assert np.array_equal(t.mul(sc), _expected()[:100])
    # m = 0
    assert t.mul(none8).shape == (0, 32)
    t.mul_device(0, 0, m=0)
    for make in (lambda: t.mul_bases(none8, levels=2), lambda: t.mul_bases_device(0, 0)):
        with make() as e:
            assert e.info["n"] == 0 and e.compute(none8) == (0, 1)
    h = t._h
    t.close()
    t.close()
    stale = M.FixedBase(h)
    for call in (lambda: stale.info, lambda: stale.mul(sc), lambda: stale.mul_bases(sc), lambda: stale.points()):
        with pytest.raises(M.MsmError) as e:
            call()
        assert e.value.code == -1
    assert L.msm_fixed_destroy(h) == -1
    stale._h = 0
    # a table is no handle and a handle no table
    t2 = _table()
    assert L.msm_bases_destroy(t2._h) == -1 and L.msm_fixed_destroy(_src()._h) == -1
    assert np.array_equal(t2.mul(sc), _expected()[:100])
    # after msm_shutdown every token is stale, and the library works again
    src_h, tab_h = _src()._h, t2._h
    _drop_caches()  # (the wrappers' close() finds the tokens gone)
    t3 = M.FixedBase(tab_h)
    L.msm_shutdown()
    with pytest.raises(M.MsmError) as e:
        t3.mul(sc)
    assert e.value.code == -1
    t3._h = 0
    assert L.msm_fixed_destroy(tab_h) == -1 and L.msm_bases_destroy(src_h) == -1
    assert np.array_equal(_table().mul(sc), _expected()[:100])


# ---- guard mode ---------------------------------------------------------------------------------------
def test_guard_bands_stay_clean():
    L = M.load()
    m, k = 257, 2
    sc = np.ascontiguousarray(_rows(2, 1000)[:m])
    exp = _expected()[:m]
    msm_sc = M.gen_scalars(m, seed=5)
    _drop_caches()  # the shutdown below frees every live handle's records
    try:
        L.msm_shutdown()
        M._test_guard(True)
        with M.Bases.from_wire(_gens(), levels=1) as b:
            M._test_guard_release()  # every buffer at this call's own size
            with b.fixed_table(first=0, count=k) as t:
                assert M._test_guard_check() == []
                assert "fx_proj" in M._test_guard_names()
                M._test_guard_release()
                assert np.array_equal(t.mul(sc), exp)
                assert M._test_guard_check() == []
                M._test_guard_release()
                d_out = _dev(np.zeros((m, 32), np.uint32))
                t.mul_device(_dev(sc), d_out)
                assert np.array_equal(_host(d_out), exp)
                assert M._test_guard_check() == []
                for make in (lambda: t.mul_bases(sc, levels=2), lambda: t.mul_bases_device(_dev(sc), m, levels=2)):
                    M._test_guard_release()
                    with make() as nb:
                        assert M._test_guard_check() == []
                        assert nb.compute(msm_sc) == O.msm(exp, msm_sc, window=10, threads=8)
                narrow = M.scalars_to_wire([1] * (m * k), scalar_bits=33).copy()
                narrow[300, 0] |= 2  # a failing call: the error word's guards too
                with pytest.raises(M.MsmError):
                    t.mul_device(_dev(narrow), d_out, scalar_bits=33)
                assert M._test_guard_check() == []
                with pytest.raises(M.MsmError):
                    t.mul_bases_device(_dev(narrow), m, scalar_bits=33)
                assert M._test_guard_check() == []
            # a small table of odd shape, built into buffers of exactly its size
            M._test_guard_release()
            with b.fixed_table(indices=[1, 0, 1], window_bits=5, scalar_bits=31) as t5:
                assert M._test_guard_check() == []
                assert np.array_equal(t5.mul([[1, 2, 3]], scalar_bits=31)[0],
                                      O.affine_to_wire([O.c_scalar_mul(O.G, 4 * (K0 + STEP) + 2 * K0)])[0])
                assert M._test_guard_check() == []
    finally:
        L.msm_shutdown()
        M._test_guard(False)
