"""GPU tests of the scalar-field vector entries (include/msm.h msm_fr_*; k_fr_combine, k_fr_powers,
k_fr_dot_partial, k_fr_dot_final): exact arithmetic mod r against Python integers.

A vector is made from *raw* 256-bit integers, the memory an element holds: for "wire" the integer itself
(any value below 2^256, meaning its residue), for "fr_mont" a canonical a = v 2^256 mod r.  _value() gives
what a raw integer means and _raw() what a result must hold, so one reference serves the four form pairs."""
import functools
import random

import numpy as np
import pytest

import msm_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

R = M.FR_MODULUS
RR = 1 << 256
R_INV = pow(RR, -1, R)
FORMS = ("wire", "fr_mont")
K0, STEP = 3, 7  # the end-to-end bases k_i G, k_i = K0 + i STEP, in the prime-order subgroup


def _enc(raws, form):
    order = "big" if form == "wire" else "little"
    buf = b"".join(int(v).to_bytes(32, order) for v in raws)
    return np.frombuffer(buf, dtype=">u4" if form == "wire" else "<u4").astype(np.uint32).reshape(-1, 8)


def _dec(arr, form):
    raw = np.ascontiguousarray(arr, dtype=np.uint32).astype(">u4" if form == "wire" else "<u4").tobytes()
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "big" if form == "wire" else "little") for i in range(len(raw) // 32)]


def _value(raw, form):
    return raw % R if form == "wire" else raw * R_INV % R


def _raw(value, form):
    return value % R if form == "wire" else value * RR % R


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32).reshape(-1, 8)


def _edges(form):
    # raw memory: wire takes anything below 2^256, fr_mont anything below r
    return [0, 1, R - 1] + ([R, R + 1, RR - 1, 1 << 255] if form == "wire" else [RR % R, R - 2])


@functools.lru_cache(maxsize=None)
def _vector(m, form, seed):
    """m raw integers: random, with the edge values at index 0, at the last lane of the first wave and at m - 1."""
    rnd = random.Random(seed * 100003 + m)
    vals = [rnd.getrandbits(256) for _ in range(m)]
    if form == "fr_mont":
        vals = [v % R for v in vals]
    edges = _edges(form)
    for j, i in enumerate(sorted({0, min(63, m - 1), m - 1})):
        vals[i] = edges[(seed + j) % len(edges)]
    return tuple(vals)


# ---- combine ------------------------------------------------------------------------------------------
SHAPES = [(x, None, False, False) for x in ("none", "bcast", "each")] + \
         [(x, y, True, sub) for x in ("none", "bcast", "each") for y in ("none", "bcast", "each") for sub in (False, True)]


def _combine_case(m, fin, fout, x_mode, y_mode, has_b, sub, seed):
    """Raw operands of one shape and the raw result."""
    a, b = _vector(m, fin, seed), _vector(m, fin, seed + 1) if has_b else None
    mult = {"none": None, "bcast": _vector(1, fin, seed + 2), "each": _vector(m, fin, seed + 3)}
    x, y = mult[x_mode], None if y_mode is None else {"none": None, "bcast": _vector(1, fin, seed + 4),
                                                     "each": _vector(m, fin, seed + 5)}[y_mode]
    pick = lambda v, i: 1 if v is None else _value(v[i % len(v)], fin)
    exp = []
    for i in range(m):
        t = pick(x, i) * _value(a[i], fin)
        if has_b:
            t += (-1 if sub else 1) * pick(y, i) * _value(b[i], fin)
        exp.append(_raw(t, fout))
    return a, b, x, y, exp


@pytest.mark.parametrize("fout", FORMS)
@pytest.mark.parametrize("fin", FORMS)
@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_combine_every_shape(m, fin, fout):
    for k, (x_mode, y_mode, has_b, sub) in enumerate(SHAPES):
        a, b, x, y, exp = _combine_case(m, fin, fout, x_mode, y_mode, has_b, sub, seed=k % 3)
        dev = lambda v: None if v is None else _dev(_enc(v, fin))
        got = M.fr_combine(dev(a), dev(b), x=dev(x), y=dev(y), sub=sub, form=fin, out_form=fout,
                           x_broadcast=x_mode == "bcast", y_broadcast=y_mode == "bcast")
        assert _dec(_host(got), fout) == exp, (x_mode, y_mode, has_b, sub)
        if k % 7 == 0:  # the host entry on the same operands
            enc = lambda v: None if v is None else _enc(v, fin)
            res = M.fr_combine(enc(a), enc(b), x=enc(x), y=enc(y), sub=sub, form=fin, out_form=fout,
                               x_broadcast=x_mode == "bcast", y_broadcast=y_mode == "bcast")
            assert _dec(res, fout) == exp


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m", [65, 4097])
def test_combine_in_place(m, form):
    a, b, x, y, exp = _combine_case(m, form, form, "bcast", "bcast", True, False, seed=1)
    for target in ("a", "b"):
        da, db = _dev(_enc(a, form)), _dev(_enc(b, form))
        out = da if target == "a" else db
        got = M.fr_combine(da, db, x=_dev(_enc(x, form)), y=_dev(_enc(y, form)), form=form, out=out)
        assert got is out and _dec(_host(out), form) == exp
        other = db if target == "a" else da
        assert _dec(_host(other), form) == list(b if target == "a" else a)  # the other operand is untouched


def test_fold_mul_convert_and_int_multipliers():
    n = 130
    a = _vector(n, "wire", 7)
    x, xi = 0x1234567890abcdef << 100, pow(0x1234567890abcdef << 100, -1, R)
    exp = [(x * a[i] + xi * a[i + n // 2]) % R for i in range(n // 2)]
    d = _dev(_enc(a, "wire"))
    assert _dec(_host(M.fr_fold(d, x, xi)), "wire") == exp
    assert _dec(M.fr_fold(_enc(a, "wire"), x, xi), "wire") == exp
    assert _dec(_host(M.fr_fold(d, x)), "wire") == [(x * a[i] + a[i + n // 2]) % R for i in range(n // 2)]
    low = d[:n // 2]
    assert M.fr_fold(d, x, xi, out=low) is low and _dec(_host(d[:n // 2]), "wire") == exp  # in place, into the low half
    assert _dec(_host(d[n // 2:]), "wire") == list(a[n // 2:])
    b = _vector(n, "wire", 8)
    assert _dec(_host(M.fr_mul(_dev(_enc(a, "wire")), _dev(_enc(b, "wire")))), "wire") == [u * v % R for u, v in zip(a, b)]
    mont = M.scalars_to_wide([v % R for v in a], "fr_mont")
    import torch

    dm = torch.from_numpy(mont.view(np.int64)).cuda()  # [n, 4] int64: arkworks memory as torch holds it
    assert _dec(_host(M.fr_convert(dm, "fr_mont", "wire")), "wire") == [v % R for v in a]
    back = M.fr_convert(M.fr_convert(dm, "fr_mont", "wire"), "wire", "fr_mont")
    assert np.array_equal(_host(back), mont.view(np.uint32).reshape(-1, 8))
    assert M.fr_to_ints(M.fr_mul(dm, 5, form="fr_mont"), "fr_mont") == [5 * v % R for v in a]


def test_combine_device_errors_leave_the_library_usable():
    import torch

    m = 257
    a = _vector(m, "fr_mont", 2)
    good = lambda: _dec(_host(M.fr_convert(_dev(_enc(a, "fr_mont")), "fr_mont", "wire")), "wire") == \
        [_value(v, "fr_mont") for v in a]
    assert good()
    buf = torch.zeros((m + 1, 8), dtype=torch.int32, device="cuda")
    calls = [
        lambda: M.fr_combine(buf[:m], out=buf[1:]),                               # a partial overlap
        lambda: M.fr_combine(buf[:m], buf[:m], x=buf[:m], out=buf[:m]),           # a multiplier as the output
        lambda: M.fr_combine(buf.view(-1)[1:1 + 8 * m]),                          # a misaligned operand
        lambda: M.fr_combine(buf[:m], out=buf.view(-1)[1:1 + 8 * m]),             # a misaligned output
        lambda: M.fr_dot(buf.view(-1)[1:1 + 8 * m]),
        lambda: M.fr_powers(3, m, out=buf.view(-1)[1:1 + 8 * m]),
    ]
    for bad_at in (0, 63, m - 1):  # a device fr_mont input >= r: the error word, after the launch
        raws = list(a)
        raws[bad_at] = R + bad_at
        d = _dev(_enc(raws, "fr_mont"))
        calls += [lambda d=d: M.fr_convert(d, "fr_mont", "wire"), lambda d=d: M.fr_dot(d, form="fr_mont"),
                  lambda d=d: M.fr_mul(_dev(_enc(a, "fr_mont")), d, form="fr_mont"),
                  lambda d=d: M.fr_dot(_dev(_enc(a, "fr_mont")), d, form="fr_mont")]
    one_bad = _dev(_enc([R], "fr_mont"))
    calls.append(lambda: M.fr_mul(_dev(_enc(a, "fr_mont")), one_bad, form="fr_mont"))  # a broadcast multiplier >= r
    for call in calls:
        with pytest.raises(M.MsmError) as e:
            call()
        assert e.value.code == -1
        assert good()


# ---- powers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g_kind", ["zero", "one", "minus_one", "two", "random"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4097, (1 << 16) + 3])
def test_powers(n, g_kind):
    rnd = random.Random(n)
    g = {"zero": 0, "one": 1, "minus_one": R - 1, "two": 2, "random": rnd.getrandbits(256)}[g_kind]
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * g % R
    for first in (None, 0, rnd.getrandbits(256)):
        exp = pw if first is None else [first * v % R for v in pw]
        for form in FORMS:
            got = M.fr_powers(g, n, first=first, out_form=form, device=0)
            assert np.array_equal(_host(got), _enc([_raw(v, form) for v in exp], form)), (first, form)
    assert np.array_equal(M.fr_powers(g, n), _enc(pw, "wire"))  # the host entry


# ---- dot ----------------------------------------------------------------------------------------------
def _dot_sizes():
    c = M._test_fr_constants()
    T, cap = c["threads"], c["dot_cap"]
    assert cap * T <= 1 << 19
    return [1, 63, 64, 65, T - 1, T, T + 1, cap * T + 65]


@functools.lru_cache(maxsize=None)
def _dot_operands():
    """Raw operands for the longest case, canonical so that both forms read them, and two arrays of each."""
    n = _dot_sizes()[-1]
    rnd = np.random.default_rng(5)
    out = []
    for _ in range(2):
        words = rnd.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
        raws = [v % R for v in _dec(words, "fr_mont")]
        raws[0], raws[63], raws[-1] = R - 1, 0, 1
        out.append(tuple(raws))
    return out


@pytest.mark.parametrize("k", range(8))
def test_dot(k):
    n = _dot_sizes()[k]
    a, b = (v[-n:] for v in _dot_operands())
    s_ab, s_a = sum(u * v for u, v in zip(a, b)) % R, sum(a) % R
    for fin in FORMS:
        da, db = _dev(_enc(a, fin)), _dev(_enc(b, fin))
        # raw integers read in form fin: a value is raw R^-e, so a product carries R^-2e
        v_ab = s_ab if fin == "wire" else s_ab * R_INV * R_INV % R
        v_a = s_a if fin == "wire" else s_a * R_INV % R
        for fout in FORMS:
            assert _dec(M.fr_dot(da, db, form=fin, out_form=fout), fout) == [_raw(v_ab, fout)]
            assert _dec(M.fr_dot(da, form=fin, out_form=fout), fout) == [_raw(v_a, fout)]
        if n <= 4096:
            assert _dec(M.fr_dot(_enc(a, fin), _enc(b, fin), form=fin), fin) == [_raw(v_ab, fin)]
            assert _dec(M.fr_dot(_enc(a, fin), form=fin), fin) == [_raw(v_a, fin)]
    if 1 < n <= 4096:  # wire inputs at and above r
        big = [v + (R if i % 2 else 0) for i, v in enumerate(a)]
        assert M.fr_to_ints([M.fr_dot(_dev(_enc(big, "wire")), _dev(_enc(b, "wire")))])[0] == s_ab
        assert M.fr_to_ints([M.fr_dot(_dev(_enc(big, "wire")))])[0] == s_a


@pytest.mark.parametrize("n", [64, 257, 5000])
def test_dot_of_cancelling_inputs_is_zero(n):
    a = _dot_operands()[0][:n]
    both = list(a) + [(R - v) % R for v in a]
    ones = [1] * (2 * n)
    for form in FORMS:
        enc = lambda v: _dev(_enc([_raw(u, form) for u in v], form))
        assert not M.fr_dot(enc(both), enc(ones), form=form).any()
        assert not M.fr_dot(enc(both), form=form).any()


# ---- guard mode ---------------------------------------------------------------------------------------
def test_guard_bands_stay_clean():
    L = M.load()
    m = 257
    a, b = _vector(m, "wire", 0), _vector(m, "wire", 1)
    x = 12345
    exp = [(x * u + 3 * v) % R for u, v in zip(a, b)]
    n_dot = M._test_fr_constants()["threads"] * 3 + 5
    da = _dot_operands()[0][:n_dot]
    try:
        L.msm_shutdown()
        M._test_guard(True)
        assert "fr_part" in M._test_guard_names()
        calls = [
            lambda: _dec(M.fr_combine(_enc(a, "wire"), _enc(b, "wire"), x=x, y=3), "wire") == exp,
            lambda: _dec(_host(M.fr_combine(_dev(_enc(a, "wire")), _dev(_enc(b, "wire")), x=x, y=3)), "wire") == exp,
            lambda: M.fr_to_ints(M.fr_powers(3, m)) == [pow(3, i, R) for i in range(m)],
            lambda: M.fr_to_ints(M.fr_powers(3, m, device=0)) == [pow(3, i, R) for i in range(m)],
            lambda: M.fr_to_ints([M.fr_dot(_enc(da, "wire"))]) == [sum(da) % R],
            lambda: M.fr_to_ints([M.fr_dot(_dev(_enc(da, "wire")), _dev(_enc(da, "wire")))]) == [sum(v * v for v in da) % R],
        ]
        for call in calls:
            M._test_guard_release()  # every buffer at this call's own size
            assert call()
            assert M._test_guard_check() == []
        bad = _dev(_enc([R - 1] * 64 + [R], "fr_mont"))  # failing calls: the error word's guards too
        for call in (lambda: M.fr_convert(bad, "fr_mont", "wire"), lambda: M.fr_dot(bad, form="fr_mont")):
            M._test_guard_release()
            with pytest.raises(M.MsmError):
                call()
            assert M._test_guard_check() == []
    finally:
        L.msm_shutdown()
        M._test_guard(False)


# ---- end to end -----------------------------------------------------------------------------------------
def test_one_inner_product_round_from_device_arrays():
    """<a', G'> = C + x^2 L + x^-2 R for G' = x^-1 G_lo + x G_hi and a' = x a_lo + x^-1 a_hi, every scalar and
    point on the device: L and R from subset MSMs, G' from Bases.fold, a' from fr_fold."""
    n, h = 64, 32
    rnd = random.Random(64)
    a = [rnd.getrandbits(256) for _ in range(n)]  # wire integers, most of them above r
    x = rnd.randrange(2, R)
    xi = pow(x, -1, R)
    d_a = _dev(M.scalars_to_wire(a))
    with M.Bases.from_wire(M.gen_points(n, k0=K0, step=STEP), levels=1) as g:
        C = g.compute_device(d_a)
        L = g.compute_subset_device(d_a[:h], first=h, m=h)  # <a_lo, G_hi>
        Rt = g.compute_subset_device(d_a[h:], first=0, m=h)  # <a_hi, G_lo>
        d_a2 = M.fr_fold(d_a, x, xi)
        with g.fold(x, xi) as g2:
            lhs = g2.compute_device(d_a2)
    rhs = O.aff_add(C, O.aff_add(O.scalar_mul(L, x * x % R), O.scalar_mul(Rt, xi * xi % R)))
    assert lhs == rhs
    ks = [K0 + i * STEP for i in range(n)]
    assert C == O.closed_form_msm(ks, [v % R for v in a])


def test_srs_from_device_powers_matches_scale_word_for_word():
    n, tau = 70, random.Random(70).getrandbits(256)
    powers = [pow(tau, i, R) for i in range(n)]
    import torch

    with M.Bases.from_wire(M.gen_points(4, k0=K0, step=STEP), levels=1) as g:
        exp = g.scale(M.scalars_to_wire(powers), indices=np.zeros(n, np.uint32))
        with g.fixed_table(first=0, count=1) as t:
            d_out = torch.zeros((n, 32), dtype=torch.int32, device="cuda")
            t.mul_device(M.fr_powers(tau, n, device=0), d_out)
            assert np.array_equal(d_out.cpu().numpy().view(np.uint32), exp)
            with t.mul_bases_device(M.fr_powers(tau, n, device=0), n, levels=1) as srs:
                assert np.array_equal(srs.points(), exp)


def test_arkworks_memory_through_convert_into_scale():
    n = 64
    rnd = random.Random(9)
    vals = [rnd.randrange(R) for _ in range(n)]
    vals[0], vals[1], vals[-1] = 0, 1, R - 1
    import torch

    d_mont = torch.from_numpy(M.scalars_to_wide(vals, "fr_mont").view(np.int64)).cuda()
    with M.Bases.from_wire(M.gen_points(n, k0=K0, step=STEP), levels=1) as g:
        d_out = torch.zeros((n, 32), dtype=torch.int32, device="cuda")
        g.scale_device(M.fr_convert(d_mont, "fr_mont", "wire"), d_out)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), g.scale(M.scalars_to_wire(vals)))
