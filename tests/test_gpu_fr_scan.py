"""GPU tests of msm_fr_inverse*, msm_fr_scan* and msm_fr_tensor* (k_fr_inverse, k_fr_scan_spans / _totals /
_apply, k_fr_tensor): exact arithmetic mod r against Python integers, on raw integers in both element forms
as tests/test_gpu_fr.py makes them (_vector: what the memory holds; _value what it means, _raw what a result
must hold).  Sizes follow the kernels' shape, read from the constants hook: E elements per lane, a tile of
256 E, and through the grid-cap hooks spans of several tiles and workgroups striding over tiles."""
import functools
import random

import numpy as np
import pytest

import msm_amd as M
import test_gpu_fr as F
from _closed_form import as_xy
from oracle import oracle as O

pytestmark = pytest.mark.gpu

R, RR, FORMS = F.R, F.RR, F.FORMS
_enc, _dec, _value, _raw, _dev, _host, _vector = F._enc, F._dec, F._value, F._raw, F._dev, F._host, F._vector
K0, STEP = F.K0, F.STEP


def _shape():
    c = M._test_fr_scan_constants()
    return c["e"], c["tile"]


def _sizes():
    _, tile = _shape()
    return [1, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 2 * tile + 65]


def _inv(v):
    return pow(v, -1, R) if v % R else 0


def _inverse_exp(raws, fin, fout, scale=1):
    return [_raw(scale * _inv(_value(a, fin)), fout) for a in raws]


def _got(t, form):
    return _dec(_host(t) if hasattr(t, "cpu") else t, form)


# ---- inverse ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fout", FORMS)
@pytest.mark.parametrize("fin", FORMS)
@pytest.mark.parametrize("k", range(11))
def test_inverse_sizes_and_forms(k, fin, fout):
    m = _sizes()[k]
    a = _vector(m, fin, k % 3)
    exp = _inverse_exp(a, fin, fout)
    assert _got(M.fr_inverse(_dev(_enc(a, fin)), form=fin, out_form=fout), fout) == exp
    if k in (0, 5, 9):  # the host entry
        assert _got(M.fr_inverse(_enc(a, fin), form=fin, out_form=fout), fout) == exp


@pytest.mark.parametrize("form", FORMS)
def test_inverse_edge_values_and_zeros(form):
    E, tile = _shape()
    m = 3 * tile
    a = list(_vector(m, form, 4))  # edge values at 0, 63 and m - 1
    zero = [0] + ([R, 2 * R] if form == "wire" else [])  # raw memory that means zero
    at = [lane * E + j for lane in (0, 63, 64, 255) for j in (0, E - 1)]  # lanes 0, 63, 64, 255: first and last of their E
    for n, i in enumerate(at):
        a[2 * tile + i] = zero[n % len(zero)]
    a[0] = 0
    for i in range(tile, 2 * tile):  # one tile all zero between two ordinary ones
        a[i] = zero[i % len(zero)]
    assert _got(M.fr_inverse(_dev(_enc(a, form)), form=form), form) == _inverse_exp(a, form, form)
    allz = [zero[i % len(zero)] for i in range(tile + 3)]
    assert not _host(M.fr_inverse(_dev(_enc(allz, form)), form=form)).any()
    one = list(allz)
    one[tile // 2 + 1] = a[5]
    assert _got(M.fr_inverse(_dev(_enc(one, form)), form=form), form) == _inverse_exp(one, form, form)
    if form == "wire":  # r and 2 r count as zero, r + 1 and 2 r + 2 do not
        got = M.fr_to_ints(M.fr_inverse(_dev(_enc([R, 2 * R, R + 1, 2 * R + 2], "wire"))))
        assert got == [0, 0, 1, _inv(2)]


def test_inverse_scale_in_place_overlap_and_stride():
    import torch

    E, tile = _shape()
    m = tile + 65
    for form in FORMS:
        a = _vector(m, form, 5)
        d = _dev(_enc(a, form))
        for scale in (None, 1, 0, R + 12345, RR - 1):
            exp = _inverse_exp(a, form, form, 1 if scale is None else scale)
            assert _got(M.fr_inverse(d, scale=scale, form=form), form) == exp, scale
        assert _got(M.fr_inverse(_enc(a[:65], form), scale=R + 7, form=form), form) == _inverse_exp(a[:65], form, form, 7)
        assert M.fr_inverse(d, form=form, out=d) is d  # in place
        assert _got(d, form) == _inverse_exp(a, form, form)
    buf = torch.zeros((m + 1, 8), dtype=torch.int32, device="cuda")
    for call in (lambda: M.fr_inverse(buf[:m], out=buf[1:]), lambda: M.fr_inverse(buf[1:], out=buf[:m]),
                 lambda: M.fr_inverse(buf.view(-1)[1:1 + 8 * m]), lambda: M.fr_inverse(buf[:m], out=buf.view(-1)[1:1 + 8 * m])):
        with pytest.raises(M.MsmError) as e:
            call()
        assert e.value.code == -1
    # one workgroup striding over four tiles, the last of one element
    m = 3 * tile + 1
    for fin, fout in (("wire", "fr_mont"), ("fr_mont", "wire")):
        a = _vector(m, fin, 6)
        got = M._test_fr_inverse_device(_dev(_enc(a, fin)), 1, scale=3, form=fin, out_form=fout)
        assert _got(got, fout) == _inverse_exp(a, fin, fout, 3)
    a = _vector(m, "wire", 6)
    assert _got(M._test_fr_inverse_device(_dev(_enc(a, "wire")), 2), "wire") == _inverse_exp(a, "wire", "wire")


def test_inverse_mont_input_at_or_above_r_raises_from_both_entries():
    _, tile = _shape()
    m = tile + 5
    a = _vector(m, "fr_mont", 2)
    for bad_at in (0, 63, m - 1):
        raws = list(a)
        raws[bad_at] = R + bad_at
        for arg in (_dev(_enc(raws, "fr_mont")), _enc(raws, "fr_mont")):
            with pytest.raises(M.MsmError) as e:
                M.fr_inverse(arg, form="fr_mont")
            assert e.value.code == -1
    assert _got(M.fr_inverse(_dev(_enc(a, "fr_mont")), form="fr_mont"), "fr_mont") == _inverse_exp(a, "fr_mont", "fr_mont")


# ---- scan ---------------------------------------------------------------------------------------------
def _scan_exp(raws, fin, fout, sum_, exclusive, first=None):
    """The raw results of a scan over raw inputs: integers all the way."""
    acc = 0 if sum_ else (1 if first is None else first % R)
    out = []
    for a in raws:
        v = _value(a, fin)
        nxt = (acc + v) % R if sum_ else acc * v % R
        out.append(_raw(acc if exclusive else nxt, fout))
        acc = nxt
    return out


def _scan(d, sum_, exclusive, fin, fout, first=None, out=None, cap=None):
    if cap is not None:
        return M._test_fr_scan_device(d, cap, first=first, sum=sum_, exclusive=exclusive, form=fin, out_form=fout, out=out)
    if sum_:
        return M.fr_cumsum(d, exclusive=exclusive, form=fin, out_form=fout, out=out)
    return M.fr_cumprod(d, first=first, exclusive=exclusive, form=fin, out_form=fout, out=out)


MODES = [(s, x) for s in (False, True) for x in (False, True)]


@pytest.mark.parametrize("fout", FORMS)
@pytest.mark.parametrize("fin", FORMS)
@pytest.mark.parametrize("k", range(11))
def test_scan_sizes_and_forms(k, fin, fout):
    m = _sizes()[k]
    a = _vector(m, fin, (k + 1) % 3)  # wire: random 256-bit integers, nearly all of them above r
    if m > 65:
        a = tuple(v if i not in (0, 63, m - 1) or _value(v, fin) else 1 for i, v in enumerate(a))  # keep the products alive
    d = _dev(_enc(a, fin))
    for sum_, exclusive in MODES:
        assert _got(_scan(d, sum_, exclusive, fin, fout), fout) == _scan_exp(a, fin, fout, sum_, exclusive), (sum_, exclusive)
    if k in (0, 5, 9):  # the host entry
        h = _enc(a, fin)
        for sum_, exclusive in MODES:
            assert _got(_scan(h, sum_, exclusive, fin, fout), fout) == _scan_exp(a, fin, fout, sum_, exclusive)


def test_scan_first_in_place_and_a_zero_in_the_middle():
    _, tile = _shape()
    m = tile + 65
    rnd = random.Random(11)
    for form in FORMS:
        a = [v if _value(v, form) else 1 for v in _vector(m, form, 7)]
        a[0], a[63], a[m - 1] = _raw(3, form) if form == "fr_mont" else R + 3, 2, a[1]  # no zero from the edge values
        for first in (0, 1, rnd.getrandbits(256)):
            for exclusive in (False, True):
                got = M.fr_cumprod(_dev(_enc(a, form)), first=first, exclusive=exclusive, form=form)
                assert _got(got, form) == _scan_exp(a, form, form, False, exclusive, first), (first, exclusive)
        assert _got(M.fr_cumprod(_enc(a[:300], form), first=R + 5, form=form), form) == _scan_exp(a[:300], form, form, False,
                                                                                                  False, 5)
        for sum_, exclusive in MODES:  # in place
            d = _dev(_enc(a, form))
            assert _scan(d, sum_, exclusive, form, form, out=d) is d
            assert _got(d, form) == _scan_exp(a, form, form, sum_, exclusive)
        z = list(a)
        z[tile // 2 + 7] = R if form == "wire" else 0  # a zero: every later product is 0, every earlier one as before
        got = _got(M.fr_cumprod(_dev(_enc(z, form)), form=form), form)
        assert got == _scan_exp(z, form, form, False, False)
        assert got[:tile // 2 + 7] == _scan_exp(a, form, form, False, False)[:tile // 2 + 7] and not any(got[tile // 2 + 7:])


@pytest.mark.parametrize("cap,tiles,extra,spans", [(1, 3, 1, [4]), (3, 7, 65, [3, 3, 2]), (1024, 5, 1, [1] * 6)])
def test_scan_spans_and_carries(cap, tiles, extra, spans):
    """cap 1: one span of four tiles, the carry crossing tiles inside it.  cap 3 at 7 tiles + 65: spans of 3, 3
    and 2 tiles, the last tile ragged.  cap 1024: the production path (fr_cumprod / fr_cumsum), one tile per span."""
    _, tile = _shape()
    m = tiles * tile + extra
    pl = M._test_fr_scan_plan(m, cap)
    ntiles = -(-m // tile)
    assert [min(pl["tiles_per_span"], ntiles - b * pl["tiles_per_span"]) for b in range(pl["grid"])] == spans
    for fin, fout in (("wire", "fr_mont"), ("fr_mont", "wire")):
        a = tuple(v if _value(v, fin) else 1 for v in _vector(m, fin, 8))
        d = _dev(_enc(a, fin))
        for sum_, exclusive in MODES:
            got = _scan(d, sum_, exclusive, fin, fout, cap=None if cap == 1024 else cap)
            assert _got(got, fout) == _scan_exp(a, fin, fout, sum_, exclusive), (sum_, exclusive)
    a = tuple(v if v % R else 1 for v in _vector(m, "wire", 9))
    d = _dev(_enc(a, "wire"))
    first = 0xfeedface
    got = _scan(d, False, True, "wire", "wire", first=first, cap=None if cap == 1024 else cap)
    assert _got(got, "wire") == _scan_exp(a, "wire", "wire", False, True, first)
    # the last element of an inclusive scan: fr_dot's sum, and the product of the integers
    last_sum = _got(_scan(d, True, False, "wire", "wire", cap=None if cap == 1024 else cap), "wire")[-1]
    assert last_sum == M.fr_to_ints([M.fr_dot(d)])[0] == sum(a) % R
    prod = 1
    for v in a:
        prod = prod * v % R
    assert _got(_scan(d, False, False, "wire", "wire", cap=None if cap == 1024 else cap), "wire")[-1] == prod


def test_scan_mont_input_at_or_above_r_raises_from_both_entries():
    _, tile = _shape()
    m = tile + 5
    a = _vector(m, "fr_mont", 2)
    for bad_at in (0, m - 1):
        raws = list(a)
        raws[bad_at] = R + bad_at
        for arg in (_dev(_enc(raws, "fr_mont")), _enc(raws, "fr_mont")):
            for fn in (M.fr_cumprod, M.fr_cumsum):
                with pytest.raises(M.MsmError) as e:
                    fn(arg, form="fr_mont")
                assert e.value.code == -1
    assert _got(M.fr_cumsum(_dev(_enc(a, "fr_mont")), form="fr_mont"), "fr_mont") == _scan_exp(a, "fr_mont", "fr_mont", True, False)


# ---- tensor -------------------------------------------------------------------------------------------
def _tensor_exp(pairs, first=None):
    out = [1 if first is None else first % R]
    for lo, hi in pairs:  # pair j on bit j: the new bit is the top one so far
        out = [v * lo % R for v in out] + [v * hi % R for v in out]
    return out


@functools.lru_cache(maxsize=None)
def _pairs(k, seed=0):
    rnd = random.Random(1000 * seed + k)
    return tuple((rnd.getrandbits(256), rnd.getrandbits(256)) for _ in range(k))


@pytest.mark.parametrize("k", list(range(15)) + [17])
def test_tensor(k):
    pairs = _pairs(k)
    exp = _tensor_exp(pairs)
    for form in FORMS:
        got = M.fr_tensor(pairs, out_form=form, device=0)
        assert np.array_equal(_host(got), _enc([_raw(v, form) for v in exp], form)), form
    if k <= 9:  # the host entry, and a first factor through both
        for form in FORMS:
            assert np.array_equal(M.fr_tensor(pairs, out_form=form), _enc([_raw(v, form) for v in exp], form))
        first = R + 99 + k
        exp1 = _enc(_tensor_exp(pairs, first), "wire")
        assert np.array_equal(M.fr_tensor(pairs, first=first), exp1)
        assert np.array_equal(_host(M.fr_tensor(pairs, first=first, device=0)), exp1)


def test_tensor_steps_and_edge_pairs():
    assert M._test_fr_constants()["pow_steps"] == 16  # k = 17 above: 2^13 lanes of 16 elements each
    edge = [0, 1, R - 1, R, R + 1, RR - 1, 2]
    pairs = [(edge[j % 7], edge[(j + 3) % 7]) for j in range(7)] + [(1, R - 1), (R - 1, 1), (5, RR - 1)]
    for first in (None, 0, R - 1):
        exp = _enc(_tensor_exp(pairs, first), "wire")
        assert np.array_equal(_host(M.fr_tensor(pairs, first=first, device=0)), exp)
    ones = [(1, 1)] * 6
    assert M.fr_to_ints(M.fr_tensor(ones, first=7, device=0)) == [7] * 64
    import torch

    out = torch.zeros((64, 8), dtype=torch.int32, device="cuda")
    assert M.fr_tensor(ones, out=out) is out and M.fr_to_ints(out) == [1] * 64
    with pytest.raises(ValueError):
        M.fr_tensor(ones, out=out[:32])
    wide = torch.zeros(8 * 64 + 8, dtype=torch.int32, device="cuda")
    with pytest.raises(M.MsmError):
        M.fr_tensor(ones, out=wide[1:1 + 8 * 64])  # misaligned


@pytest.mark.parametrize("k", [0, 5, 13])
def test_tensor_of_squarings_is_powers_word_for_word(k):
    g = random.Random(k).getrandbits(256)
    pairs = [(1, pow(g, 1 << j, R)) for j in range(k)]
    for form in FORMS:
        assert np.array_equal(_host(M.fr_tensor(pairs, first=3, out_form=form, device=0)),
                              _host(M.fr_powers(g, 1 << k, first=3, out_form=form, device=0)))


# ---- guard bands and poison -----------------------------------------------------------------------------
def test_guard_bands_stay_clean_and_poison_changes_nothing():
    import torch

    L = M.load()
    _, tile = _shape()
    m = 2 * tile + 65
    a = tuple(v if v % R else 1 for v in _vector(m, "wire", 3))
    ea = _enc(a, "wire")
    pairs = _pairs(9, 1)
    inv, tens = _inverse_exp(a, "wire", "wire", 5), _tensor_exp(pairs, 7)
    scans = {mode: _scan_exp(a, "wire", "wire", *mode) for mode in MODES}

    def calls(da, bad):
        good = [lambda: _got(M.fr_inverse(ea, scale=5), "wire") == inv,
                lambda: _got(M.fr_inverse(da, scale=5), "wire") == inv,
                lambda: _got(M._test_fr_inverse_device(da, 1, scale=5), "wire") == inv,
                lambda: _got(M.fr_tensor(pairs, first=7), "wire") == tens,
                lambda: _got(M.fr_tensor(pairs, first=7, device=0), "wire") == tens]
        for mode in MODES:
            good += [lambda mode=mode: _got(_scan(ea, *mode, "wire", "wire"), "wire") == scans[mode],
                     lambda mode=mode: _got(_scan(da, *mode, "wire", "wire"), "wire") == scans[mode],
                     lambda mode=mode: _got(_scan(da, *mode, "wire", "wire", cap=2), "wire") == scans[mode]]
        failing = [lambda: M.fr_inverse(bad, form="fr_mont"), lambda: M.fr_inverse(_host(bad), form="fr_mont"),
                   lambda: M.fr_cumprod(bad, form="fr_mont"), lambda: M.fr_cumsum(_host(bad), form="fr_mont"),
                   lambda: M.fr_cumsum(bad, form="fr_mont"), lambda: M.fr_tensor([(1, 2)] * 32),
                   lambda: M.fr_tensor(pairs, out=torch.zeros(8 * 512 + 1, dtype=torch.int32, device="cuda")[1:])]
        return good, failing

    try:
        L.msm_shutdown()
        M._test_guard(True)
        assert "fr_part" in M._test_guard_names()
        for fill in (0, 1, 3):  # the identity of a product scan is 1 and of a sum 0: both fills
            M._test_guard_fill(fill)
            good, failing = calls(_dev(ea), _dev(_enc([R - 1] * (tile + 64) + [R], "fr_mont")))
            for call in good:
                M._test_guard_release()  # every buffer at this call's own size
                assert call()
                assert M._test_guard_check() == []
                if fill:
                    M._test_guard_poison()  # the same call on buffers that hold nothing of the launch before it
                    assert call()
                    assert M._test_guard_check() == []
            for call in failing:
                M._test_guard_release()
                with pytest.raises(M.MsmError):
                    call()
                assert M._test_guard_check() == []
                if fill:
                    M._test_guard_poison()
                    assert good[1]() and good[-2]()
                    assert M._test_guard_check() == []
    finally:
        M._test_guard_fill(0)
        L.msm_shutdown()
        M._test_guard(False)


# ---- end to end -----------------------------------------------------------------------------------------
def test_inner_product_verifier_folds_to_the_tensor_msm():
    """Four folds of 16 generators leave one point, sum_i s_i P_i with s the tensor product of the rounds'
    (x^-1, x): Bases.fold pairs P_i with P_(i + n/2), so the FIRST round decides the TOP bit of i."""
    n, rounds = 16, 4
    rnd = random.Random(16)
    xs = [rnd.randrange(2, R) for _ in range(rounds)]
    xinv = M.fr_to_ints(M.fr_inverse(xs))
    assert [x * xi % R for x, xi in zip(xs, xinv)] == [1] * rounds
    pairs = [(xinv[rounds - 1 - b], xs[rounds - 1 - b]) for b in range(rounds)]  # pair b on bit b: round rounds - 1 - b
    s = M.fr_tensor(pairs, device=0)
    s_int = [1] * n
    for i in range(n):
        for j in range(rounds):
            s_int[i] = s_int[i] * (xs[j] if (i >> (rounds - 1 - j)) & 1 else xinv[j]) % R
    assert M.fr_to_ints(s) == s_int
    with M.Bases.from_wire(M.gen_points(n, k0=K0, step=STEP), levels=1) as g:
        direct = g.compute_device(s)
        h = g
        try:
            for j in range(rounds):
                nxt = h.fold(xs[j], xinv[j], levels=1)
                if h is not g:
                    h.close()
                h = nxt
            assert h.info["n"] == 1
            folded = as_xy(h.points()[0])
        finally:
            if h is not g:
                h.close()
    assert folded == direct
    assert direct == O.closed_form_msm([K0 + i * STEP for i in range(n)], s_int)


def test_grand_product_of_a_permutation_closes_at_one():
    """z_0 = 1, z_(i+1) = z_i f_i / g_i with g a permutation of f: the exclusive running product starts at 1 and
    the inclusive one ends at 1.  Every vector stays on the device."""
    _, tile = _shape()
    m = 2 * tile + 65
    rnd = random.Random(2065)
    f = [rnd.randrange(1, R) for _ in range(m)]
    g = list(f)
    rnd.shuffle(g)
    df, dg = _dev(_enc(f, "wire")), _dev(_enc(g, "wire"))
    ratio = M.fr_mul(df, M.fr_inverse(dg))
    z = M.fr_to_ints(M.fr_cumprod(ratio, exclusive=True))
    exp, acc = [], 1
    for u, v in zip(f, g):
        exp.append(acc)
        acc = acc * u * pow(v, -1, R) % R
    assert z == exp and z[0] == 1 and acc == 1
    assert M.fr_to_ints(M.fr_cumprod(ratio)[-1:]) == [1]
