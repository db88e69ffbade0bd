"""CPU tests of point decompression's parts that need no device: the model of the device's square root
(tests/_sqrt_model.py) against the oracle's, on non-residues, 0 and inputs of every depth; the kernel's
constants, recomputed from p and compared with what the library holds; the limb bounds of the kernel's
own compositions; and msm_compress_points against plain Python."""
import random

import numpy as np
import pytest

import _sqrt_model as S
import msm_amd as M
import test_limb_bounds as LB
from oracle import oracle as O

P = O.P


def test_field_shape():
    assert S.TWO_ADICITY == 47 and S.Q % 2 == 1 and (S.Q << 47) + 1 == P
    assert S.NONRESIDUE == 11
    assert pow(S.OMEGA, 1 << 46, P) == P - 1  # order exactly 2^47
    assert pow(O.EDWARDS_D, (P - 1) // 2, P) == P - 1  # d x^2 - 1 is never 0


def test_library_constants_recomputed_from_p():
    c = M._test_decompress_constants()
    assert c["two_adicity"] == S.TWO_ADICITY
    assert c["exp"] == (S.Q - 1) // 2 and c["exp"] < 1 << (32 * c["exp_words"])
    assert c["order"] == O.R_ORDER and c["order"].bit_length() == c["order_bits"]
    # omega in the device's Montgomery form (R = 2^261), 29-bit limbs, canonical
    limbs = c["omega_mont_limbs"]
    assert all(0 <= v < 1 << 29 for v in limbs)
    assert sum(v << (29 * i) for i, v in enumerate(limbs)) == S.OMEGA * (1 << 261) % P


def test_zero_one_and_nonresidues():
    assert S.sqrt_or_none(0) == 0
    assert S.sqrt_or_none(1) == 1
    rnd = random.Random(3)
    seen = 0
    for u in list(range(2, 60)) + [rnd.randrange(P) for _ in range(60)]:
        ref = O.sqrt_mod(u)
        got = S.sqrt_or_none(u)
        if ref is None:
            seen += 1
            assert got is None
        else:
            assert got is not None and got * got % P == u and got in (ref, P - ref)
    assert seen >= 30


def test_every_depth():
    rnd = random.Random(5)
    for k in range(S.TWO_ADICITY):
        y = S.depth_input(k, rnd.randrange(2, P))
        u = y * y % P
        assert S.first_round_depth(u) == k
        trace = []
        r = S.sqrt_ts(u, trace)
        assert r * r % P == u and r in (y, P - y)
        assert (trace[0] if trace else 0) == k and trace == sorted(trace, reverse=True)
        ref = O.sqrt_mod(u)
        assert r in (ref, P - ref)
    # a non-residue: the loop gives up at i = m = 47, and r^2 != u
    u = S.NONRESIDUE
    assert S.first_round_depth(u) == 47 and S.sqrt_or_none(u) is None


def test_crafted_points_cover_every_depth_on_the_curve():
    pts = S.crafted_points()
    assert [k for k, _, _ in pts] == list(range(47))
    for k, x, y in pts:
        assert O.on_curve((x, y)) and S.first_round_depth(S.y_squared(x)) == k
        for yy in (y, (P - y) % P):
            w = S.compress((x, yy), S.FORM_YSIGN)
            assert S.decompress(w, S.FORM_YSIGN) == (0, (x, yy))


def test_decompress_model_rules():
    i4 = O.sqrt_mod(P - 1)
    assert S.decompress(0, S.FORM_SUBGROUP) == (0, (0, 1))
    assert S.decompress(0, S.FORM_YSIGN) == (0, (0, 1))
    assert S.decompress(1 << 255, S.FORM_YSIGN) == (0, (0, P - 1))
    assert S.decompress(i4, S.FORM_YSIGN) == (0, (i4, 0))
    assert S.decompress(i4 | 1 << 255, S.FORM_YSIGN)[0] == S.ERR_BAD_POINT
    assert S.decompress(i4, S.FORM_SUBGROUP)[0] == S.ERR_BAD_POINT  # an order-4 point
    for form in (S.FORM_SUBGROUP, S.FORM_YSIGN):
        assert S.decompress(P, form)[0] == S.ERR_COORD_RANGE
        assert S.decompress(1 << 253, form)[0] == S.ERR_COORD_RANGE
    assert S.decompress(1 << 254, S.FORM_YSIGN)[0] == S.ERR_COORD_RANGE
    for k in (1, 2, 3, 50):
        pt = O.scalar_mul(O.G, k)
        assert S.decompress(pt[0], S.FORM_SUBGROUP) == (0, pt)
        assert O.point_from_x(pt[0]) == pt
        # the coset k G + T4: on the curve, neither root in the subgroup
        x = i4 * pt[1] % P
        assert S.decompress(x, S.FORM_SUBGROUP)[0] == S.ERR_BAD_POINT
        assert S.decompress(x, S.FORM_YSIGN)[0] == 0


def test_kernel_compositions_stay_inside_the_proved_limb_bounds():
    """k_decompress_x's own operand forms, through test_limb_bounds' interval model (every fe_mul there
    asserts its columns below 2^64 and its operands' values below 2^257)."""
    B, N_MUL = LB.B, LB.N_MUL
    one = B.normalised(P)                        # ONE29 = R mod p
    x_std = B.normalised(P)                      # the range-checked input, as limbs
    xm = LB.fe_mul(x_std, B.normalised(P))       # fe_to_mont: x R2_29
    x2 = LB.fe_mul(xm, xm)
    num = LB.fe_norm(LB.fe_add(x2, one))
    den = LB.fe_sub(one, N_MUL)                  # fe_mul_d's output is below 2p (test_mul_d_exact_and_below_2p)
    acc = LB.fe_mul(N_MUL, den)                  # fe_inv: r = r a, r = r r
    u = LB.fe_mul(num, acc)
    assert num.v < 4 * P and den.v < 10 * P
    for v in (xm, x2, acc, u):                   # fe_mul outputs
        assert v is N_MUL
    LB.fe_mul(u, N_MUL)                          # fe_sqrt_ts: every product is of fe_mul outputs and u, omega
    LB.fe_mul(N_MUL, one)
    # the ladder's point: (xm, r, xm r, ONE29), each within N_MUL, as test_pdbl_bounds / test_padd_bounds take them
    for v in (xm, one):
        assert v.v <= N_MUL.v and all(a <= b for a, b in zip(v.l, N_MUL.l))


def test_compress_points_against_python():
    rnd = random.Random(9)
    i4 = O.sqrt_mod(P - 1)
    pts = [O.scalar_mul(O.G, rnd.randrange(1, O.R_ORDER)) for _ in range(12)]
    pts += [(0, 1), (0, P - 1), (i4, 0), (P - i4, 0), (5, (P - 1) // 2), (5, (P + 1) // 2)]
    for name, form in (("subgroup", S.FORM_SUBGROUP), ("ysign", S.FORM_YSIGN)):
        exp = [S.compress(p, form) for p in pts]
        got = M.compress_points(pts, name)
        assert got.shape == (len(pts), 8) and O.be_words_to_ints(got) == exp
        assert O.be_words_to_ints(M.compress_points(O.affine_to_wire(pts), name)) == exp
    assert (S.compress((5, (P + 1) // 2), S.FORM_YSIGN) >> 255) == 1 and (S.compress((5, (P - 1) // 2), 2) >> 255) == 0
    assert M.compress_points(np.zeros((0, 16), np.uint32)).shape == (0, 8)
    with pytest.raises(M.MsmError) as e:
        M.compress_points([(P, 1)])
    assert e.value.code == -3
    with pytest.raises(M.MsmError) as e:
        M.compress_points([(1, 1)], 7)
    assert e.value.code == -1
    # the packer sets the flag; the caller does not OR it in
    w = M.xs_to_wire([5, 6], "ysign", signs=[True, False])
    assert O.be_words_to_ints(w) == [5 | 1 << 255, 6]
    with pytest.raises(ValueError):
        M.xs_to_wire([1 << 255], "ysign", signs=[False])
    with pytest.raises(ValueError):
        M.xs_to_wire([1], "subgroup", signs=[False])
