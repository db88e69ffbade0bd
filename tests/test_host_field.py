"""hostfield.h at operand level against Python integers (msm_test_host_field; needs no device).

fq_mul, fq_mul_n and fq_inv finish every MSM.  The hook takes and returns raw representatives -- the
integer an Fq's four limbs hold, below p -- so each function is priced on plain integers with
nothing of the library's in the reference: fq_mul(a, b) = a b / 2^256 mod p, fq_inv(a) =
2^512 / a mod p, and so on.  The operands are the field's and the limbs' edges, the values that
drive fq_inv's strip_twos through its zero-low-limb branch (odd 2^t and p - odd 2^t around the limb
boundaries), every pair of those, and 2,000 random pairs.
"""
import functools
import random

import msm_amd as M
from oracle import oracle as O

P = O.P
R = 1 << 256
RINV = pow(R, -1, P)
SHIFTS = (62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193)


@functools.lru_cache(maxsize=None)
def specials():
    vals = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2]
    for k in (64, 128, 192):
        vals += [1 << k, (1 << k) - 1, P >> k << k]  # p with its low one, two, three limbs cleared
    for t in SHIFTS:
        for odd in (1, 3, 0x1F5):
            vals += [odd << t, P - (odd << t)]
    assert all(0 <= v < P for v in vals)
    return sorted(set(vals))


@functools.lru_cache(maxsize=None)
def pairs():
    sp = specials()
    rnd = random.Random(0xF1E1D)
    out = [(a, b) for a in sp for b in sp]
    for i in range(2000):
        hi = (253, 253, 64, 130)[i % 4]  # full-width and short operands
        out.append((rnd.randrange(P) >> (253 - hi), rnd.randrange(P)))
    return out


def check(name, got, want, operands):
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not bad, \
        f"{name}: {len(bad)} of {len(want)} differ; first at {operands[bad[0]]}: library {got[bad[0]]:#x}, integers {want[bad[0]]:#x}"


def test_products():
    ab = pairs()
    a, b = [x for x, _ in ab], [y for _, y in ab]
    want = [x * y * RINV % P for x, y in ab]
    check("fq_mul", M._test_host_field("mul", a, b), want, ab)
    # the interleaved batches: the list, and the list moved on by one and two places, so that every
    # operand pair meets every lane of fq_mul_n<3> and fq_mul_n<4>
    for name, lanes in (("mul_n3", 3), ("mul_n4", 4)):
        for shift in range(lanes):
            sab = ab[shift:] + ab[:shift]
            got = M._test_host_field(name, [x for x, _ in sab], [y for _, y in sab])
            check(f"fq_{name} (list moved by {shift})", got, want[shift:] + want[:shift], sab)


def test_sums_and_differences():
    ab = pairs()
    a, b = [x for x, _ in ab], [y for _, y in ab]
    check("fq_add", M._test_host_field("add", a, b), [(x + y) % P for x, y in ab], ab)
    check("fq_sub", M._test_host_field("sub", a, b), [(x - y) % P for x, y in ab], ab)


def test_inverse():
    vals = specials() + sorted({x for x, _ in pairs()[-2000:]} | {y for _, y in pairs()[-2000:]})
    # a is x R, the inverse x^-1 R = R^2 / a; 0 -> 0
    want = [pow(v, -1, P) * R * R % P if v else 0 for v in vals]
    check("fq_inv", M._test_host_field("inv", vals), want, vals)
    zero_low = [v for v in vals if v and not v & ((1 << 64) - 1)]
    assert len(zero_low) >= 8  # strip_twos' u[0] == 0 branch, on entry


def test_inverse_meets_a_zero_low_limb_inside_the_loop():
    # u - v (or v - u) with 64 or more trailing zeros after the first subtraction: a = p - odd 2^t
    # gives v - u = odd 2^t at once
    vals = [P - (odd << t) for t in SHIFTS if t >= 64 for odd in (1, 3, 0x1F5)]
    check("fq_inv", M._test_host_field("inv", vals), [pow(v, -1, P) * R * R % P for v in vals], vals)


def test_forms():
    vals = specials() + [x for x, _ in pairs()[-500:]]
    check("fq_from_std", M._test_host_field("from_std", vals), [v * R % P for v in vals], vals)
    check("fq_to_std", M._test_host_field("to_std", vals), [v * RINV % P for v in vals], vals)
    for k in (1, 32, 63):
        check(f"div2k_mod k = {k}", M._test_host_field(f"div2k_{k}", vals), [v * pow(2, -k, P) % P for v in vals], vals)


# ---- points: raw extended coordinates against the oracle's affine group law ------------------------
I4 = O.sqrt_mod(P - 1)
TORSION = [(0, 1), (0, P - 1), (I4, 0), (P - I4, 0)]


def ext(aff, z):
    x, y = aff
    return tuple(v * R % P for v in (x * z, y * z, x * y * z, z))


def affine(pt, want_t=True):
    X, Y, T, Z = (v * RINV % P for v in pt)
    assert all(v < P for v in pt)
    if want_t:
        assert X * Y % P == T * Z % P
    zi = pow(Z, -1, P)
    return (X * zi % P, Y * zi % P)


@functools.lru_cache(maxsize=None)
def point_pairs():
    rnd = random.Random(0xED25)
    pts = [O.scalar_mul(O.G, rnd.randrange(1, O.R_ORDER)) for _ in range(6)]
    pts += [O.aff_add(pts[0], TORSION[2])] + TORSION
    zs = [1, 2, P - 1, (P + 1) // 2, 1 << 192] + [rnd.randrange(1, P) for _ in range(3)]
    out = []
    for i, p in enumerate(pts):
        for j, q in enumerate(pts + [p, O.aff_neg(p)]):
            out.append((p, q, zs[(i + j) % len(zs)], zs[(3 * i + j + 1) % len(zs)]))
    return out


def test_point_addition():
    pp = point_pairs()
    a, b = [ext(p, z1) for p, _, z1, _ in pp], [ext(q, z2) for _, q, _, z2 in pp]
    want = [O.aff_add(p, q) for p, q, _, _ in pp]
    got = M._test_host_field("pt_add", a, b)
    assert [affine(g) for g in got] == want
    got = M._test_host_field("pt_add_no_t", a, b)
    assert [affine(g, False) for g in got] == want and all(g[2] == 0 for g in got)


def test_point_doubling():
    pp = point_pairs()
    a = [ext(p, z1) for p, _, z1, _ in pp]
    for name, k in (("pt_dbl", 1), ("pt_dbl_n1", 1), ("pt_dbl_n2", 2), ("pt_dbl_n5", 5)):
        got = M._test_host_field(name, a)
        assert [affine(g) for g in got] == [O.scalar_mul(p, 1 << k) for p, _, _, _ in pp], name


def test_hook_refuses_operands_outside_the_field():
    import pytest

    with pytest.raises(M.MsmError):
        M._test_host_field("mul", [P], [1])
    with pytest.raises(M.MsmError):
        M._test_host_field("add", [1], [P + 5])
