"""GPU tests of compressed points (include/msm.h MSM_POINTS_X_*, k_decompress_x): decompression of both
forms against points whose y is known from their construction (multiples of G from the generator, and
curve points crafted for every Tonelli-Shanks depth), the error rules, bit-exact parity of a compressed
handle with the wire handle of the same points, the device entries, and the guard-band mode."""
import ctypes
import functools
import random

import numpy as np
import pytest

import _sqrt_model as S
import msm_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

P = O.P
I4 = O.sqrt_mod(P - 1)  # sqrt(-1): (I4, 0) has order 4
K0, STEP = 3, 7
NBIG = (1 << 14) + 3


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def _gen():
    """The generator's own wire points (k G, k = K0 + i STEP): x, y, x y, 1."""
    pts = M.gen_points(NBIG, k0=K0, step=STEP)
    pts.setflags(write=False)
    return pts


def _affine(pts):
    return [(O.be_words_to_int(r[:8]), O.be_words_to_int(r[8:16])) for r in pts]


def _ysign_words(pts):
    """Compressed ysign words of wire points, flags from the known y."""
    aff = _affine(pts)
    return M.xs_to_wire([x for x, _ in aff], "ysign", signs=[y > P - y for _, y in aff])


@functools.lru_cache(maxsize=None)
def _crafted():
    return S.crafted_points()


# ---- decompression, subgroup form -------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, NBIG])
def test_subgroup_form_gives_back_the_generators_points(n):
    pts = _gen()[:n]
    got = M.decompress_points(np.ascontiguousarray(pts[:, :8]), "subgroup")
    assert got.shape == (n, 32) and np.array_equal(got, pts)
    if n == 64:  # both roots' branches run: about half of the points need the negated one
        flips = sum(S.sqrt_ts(S.y_squared(x)) != y for x, y in _affine(pts))
        assert 16 <= flips <= 48
    if n == 65:  # Python ints in, and the ysign form of the same points
        assert np.array_equal(M.decompress_points([x for x, _ in _affine(pts)]), pts)
        assert np.array_equal(M.decompress_points(_ysign_words(pts), "ysign"), pts)


# ---- decompression, sign form -----------------------------------------------------------------------
def test_sign_form_at_every_depth_and_the_special_points():
    aff = []
    for _, x, y in _crafted():
        aff += [(x, y), (x, (P - y) % P)]
    aff += [(0, 1), (0, P - 1), (I4, 0), (P - I4, 0)]
    words = M.xs_to_wire([x for x, _ in aff], "ysign", signs=[y > P - y for _, y in aff])
    assert O.be_words_to_ints(words[-4:]) == [0, 1 << 255, I4, P - I4]
    got = M.decompress_points(words, "ysign")
    assert np.array_equal(got, O.affine_to_wire(aff))
    # compress is its inverse
    assert np.array_equal(M.compress_points(got, "ysign"), words)


def test_subgroup_form_at_every_depth():
    inside, outside = [], []
    for _, x, y in _crafted():
        mine = [(x, yy) for yy in (y, (P - y) % P) if O.c_scalar_mul((x, yy), O.R_ORDER) == O.IDENTITY]
        assert len(mine) <= 1
        if mine:
            inside.append(mine[0])
        else:
            outside.append(x)
    assert len(inside) >= 12 and len(outside) >= 12  # each coset pair is hit by half of the points
    got = M.decompress_points([x for x, _ in inside], "subgroup")
    assert np.array_equal(got, O.affine_to_wire(inside))
    for x in outside[:3]:  # on the curve, neither root in the subgroup
        with pytest.raises(M.MsmError) as e:
            M.decompress_points([x], "subgroup")
        assert e.value.code == -4


# ---- errors -----------------------------------------------------------------------------------------
def _create_raw(words, form):
    """msm_bases_create_compressed with *out preset to a sentinel: (code, *out)."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    h = ctypes.c_void_p(0xDEAD)
    rc = M.load().msm_bases_create_compressed(w.ctypes.data_as(ctypes.c_void_p), w.shape[0], form, None, 1,
                                              ctypes.byref(h))
    return rc, h.value


@functools.lru_cache(maxsize=None)
def _good257():
    pts = _gen()[:257]
    sub = np.ascontiguousarray(pts[:, :8])
    sgn = _ysign_words(pts)
    sub.setflags(write=False)
    sgn.setflags(write=False)
    return sub, sgn


@functools.lru_cache(maxsize=None)
def _bad_inputs():
    nonres = next(x for x in range(1, 200) if S.sqrt_or_none(S.y_squared(x)) is None)
    coset = I4 * O.scalar_mul(O.G, 5)[1] % P  # the x of 5 G + T4
    assert O.on_curve((coset, S.sqrt_or_none(S.y_squared(coset))))
    # (word, code in the subgroup form or None for "fine", code in the sign form or None)
    return [
        ("non-residue", nonres, -4, -4),
        ("coset", coset, -4, None),
        ("x = p", P, -3, -3),
        ("x = 2^253", 1 << 253, -3, -3),
        ("bit 254", 5 | 1 << 254, -3, -3),
        ("bits 253 and 255", 5 | 1 << 253 | 1 << 255, -3, -3),
        ("(sqrt(-1), flag 1)", I4 | 1 << 255, -3, -4),
    ]


@pytest.mark.parametrize("at", [0, 63, 64, 255, 256])
def test_one_bad_point_fails_the_creation(at):
    sub, sgn = _good257()
    sc = M.gen_scalars(257, seed=5)
    exp = O.msm(_gen()[:257], sc, window=10, threads=8)
    for what, word, code_sub, code_sgn in _bad_inputs():
        for form, good, code in ((S.FORM_SUBGROUP, sub, code_sub), (S.FORM_YSIGN, sgn, code_sgn)):
            assert S.decompress(word, form)[0] == (code or 0), what  # the model agrees with the table
            v = good.copy()
            v[at] = O.int_to_be_words(word)
            rc, h = _create_raw(v, form)
            if code is None:
                assert rc == 0 and h, (what, form)
                assert M.load().msm_bases_destroy(h) == 0
                continue
            assert (rc, h) == (code, None), (what, form, at)
            with pytest.raises(M.MsmError) as e:
                M.decompress_points(v, form)
            assert e.value.code == code, (what, form, at)
        # and a good creation on the same device succeeds
        with M.Bases.from_x(sub) as b:
            assert b.compute(sc) == exp, what


def test_a_range_error_takes_precedence():
    sub, sgn = _good257()
    nonres = _bad_inputs()[0][1]
    for form, good in ((S.FORM_SUBGROUP, sub), (S.FORM_YSIGN, sgn)):
        for a, b in ((3, 200), (200, 3), (64, 65)):
            v = good.copy()
            v[a] = O.int_to_be_words(nonres)
            v[b] = O.int_to_be_words(P)
            assert _create_raw(v, form) == (-3, None)


def test_bad_points_are_written_as_the_identity():
    sub, _ = _good257()
    v = sub[:70].copy()
    v[64] = O.int_to_be_words(_bad_inputs()[0][1])
    d_out = _dev(np.full((70, 32), 0xFFFFFFFF, np.uint32))
    with pytest.raises(M.MsmError) as e:
        M.decompress_points_device(_dev(v), 70, d_out)
    assert e.value.code == -4
    exp = _gen()[:70].copy()
    exp[64] = O.affine_to_wire([(0, 1)])[0]
    assert np.array_equal(_host(d_out), exp)


def test_argument_rules():
    sub, _ = _good257()
    L = M.load()
    vp = ctypes.c_void_p
    for form in (0, 3, 7):
        assert _create_raw(sub, form) == (-1, None)
        with pytest.raises(M.MsmError) as e:
            M.decompress_points(sub, form)
        assert e.value.code == -1
    out = np.zeros((257, 32), np.uint32)
    h = vp(0xDEAD)
    for opts in (M._opts(None, scalar_bits=64), M._opts(13, windows=(0, 2)), M._opts(None, devices=[0]),
                 M._opts(None, scalar_type="u32")):
        assert L.msm_bases_create_compressed(sub.ctypes.data_as(vp), 257, 1, opts, 1, ctypes.byref(h)) == -1
        assert h.value is None
        h = vp(0xDEAD)
        assert L.msm_decompress_points(sub.ctypes.data_as(vp), 257, 1, opts, out.ctypes.data_as(vp)) == -1
    # a device pointer off by 4 bytes: refused from its value
    d = _dev(np.concatenate([np.zeros(1, np.uint32), sub.reshape(-1)]))
    d_out = _dev(np.zeros(257 * 32 + 4, np.uint32))
    with pytest.raises(M.MsmError) as e:
        M.Bases.from_x_device(d.data_ptr() + 4, 257)
    assert e.value.code == -1
    with pytest.raises(M.MsmError) as e:
        M.decompress_points_device(d.data_ptr() + 4, 257, d_out)
    assert e.value.code == -1
    with pytest.raises(M.MsmError) as e:
        M.decompress_points_device(_dev(sub), 257, d_out.data_ptr() + 4)
    assert e.value.code == -1


def test_empty_vectors():
    for form in ("subgroup", "ysign"):
        assert M.decompress_points(np.zeros((0, 8), np.uint32), form).shape == (0, 32)
        assert M.decompress_points([], form).shape == (0, 32)
        with M.Bases.from_x(np.zeros((0, 8), np.uint32), form, levels=2) as b:
            assert b.info["n"] == 0
            assert b.compute(np.zeros((0, 8), np.uint32)) == (0, 1)
    with M.Bases.from_x_device(0, 0) as b:
        assert b.info["n"] == 0
    M.decompress_points_device(0, 0, 0)


# ---- handle parity ----------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2])
def test_a_compressed_handle_is_the_wire_handle(levels):
    n = 300
    pts = _gen()[:n]
    sc = M.gen_scalars(n, seed=31)
    exp = O.msm(pts, sc, window=10, threads=8)
    rnd = random.Random(7)
    narrow = [rnd.getrandbits(64) for _ in range(n)]
    exp_narrow = O.msm(pts, O.ints_to_be_words(narrow), window=10, threads=8)
    idx = np.array([rnd.randrange(n) for _ in range(120)], np.uint32)
    exp_sub = O.msm(pts[idx], sc[:120], window=10, threads=8)
    with M.Bases.from_wire(pts, levels=levels, window_size=13) as ref:
        want = [M._test_bases_records(ref, j) for j in range(levels)]
        info = ref.info
    for words, form in ((np.ascontiguousarray(pts[:, :8]), "subgroup"), (_ysign_words(pts), "ysign")):
        for make in (lambda: M.Bases.from_x(words, form, levels=levels, window_size=13),
                     lambda: M.Bases.from_x_device(_dev(words), n, form, levels=levels, window_size=13)):
            with make() as b:
                assert b.info == info
                for j in range(levels):
                    assert np.array_equal(M._test_bases_records(b, j), want[j]), (form, j)
                assert b.compute(sc) == exp
                assert b.compute(M.scalars_to_wire(narrow, scalar_bits=64), scalar_bits=64) == exp_narrow
                assert b.compute_subset(sc[:120], indices=idx) == exp_sub


# ---- device entries ---------------------------------------------------------------------------------
def test_decompressed_points_feed_the_device_msm():
    import torch

    n = 1000
    pts = _gen()[:n]
    sc = M.gen_scalars(n, seed=41)
    exp = O.msm(pts, sc, window=10, threads=8)
    d_xs = _dev(pts[:, :8])
    d_pts = torch.zeros((n, 32), dtype=torch.int32, device="cuda")
    M.decompress_points_device(d_xs, n, d_pts, "subgroup")
    assert np.array_equal(_host(d_pts), pts)
    assert M.compute_msm_device(d_pts, _dev(sc), n) == exp
    d_pts.zero_()
    M.decompress_points_device(_dev(_ysign_words(pts)), n, d_pts, "ysign")
    assert np.array_equal(_host(d_pts), pts)


# ---- guard mode -------------------------------------------------------------------------------------
def test_guard_bands_stay_clean():
    L = M.load()
    n = 257
    pts = _gen()[:n]
    sc = M.gen_scalars(n, seed=5)
    exp = O.msm(pts, sc, window=10, threads=8)
    xs = np.ascontiguousarray(pts[:, :8])
    try:
        L.msm_shutdown()
        M._test_guard(True)
        assert "dx_pts" in M._test_guard_names()
        with M.Bases.from_x(xs, levels=2) as b:
            assert M._test_guard_check() == []
            assert b.compute(sc) == exp
        M._test_guard_release()
        assert np.array_equal(M.decompress_points(_ysign_words(pts), "ysign"), pts)
        assert M._test_guard_check() == []
        bad = xs.copy()
        bad[256] = O.int_to_be_words(P)  # the error word's guards too
        with pytest.raises(M.MsmError):
            M.Bases.from_x(bad)
        assert M._test_guard_check() == []
    finally:
        L.msm_shutdown()
        M._test_guard(False)
