"""The limb-exact models of the per-lane point kernels' functions (tests/_fp29_model.py: fe_sqr,
fe_std_neg, fe_mul_out_is_one, pt_from_record, fe_sqrt_ts, pt_mul_order, k_shift_bases' lane,
k_fixed_eval's addition chain) against plain integers, on the whole catalogue
(tests/_lane_catalogue.py), with every row checked to lie inside its function's contract: the
reference alone is right at every entry before tests/test_gpu_lanes.py asks the device.
"""
import random

import pytest

import _fp29_model as F
import _lane_catalogue as L
import _sqrt_model as S
from _bases_model import check_record_bounds, decode_record, expected_record_values
from _fp29_model import NL, P, RINV, value_of
from oracle import oracle as O
from test_fp29_model import affine_of, check_point, normalised

MASK_SETS = [F.DEFAULT_MASKS, F.NARROW_MASKS]


def std(limbs):
    return value_of(limbs) * RINV % P


def test_rows_are_inside_their_contracts():
    cat = L.catalogue()
    for op in ("sqr", "std_neg", "is_one", "from_record", "shift_lane", "sqrt_ts", "mul_order"):
        assert cat[op], op
        for row in cat[op]:
            assert L.in_contract(op, row), (op, row)


def test_catalogue_reaches_the_extremes():
    cat = L.catalogue()
    ymx = [value_of(r[0:NL]) for r in cat["from_record"]]
    ypx = [value_of(r[F.PRE_HALF:F.PRE_HALF + NL]) for r in cat["from_record"]]
    assert 10 * P - 1 in ymx and 8 * P - 1 in ymx and 4 * P - 1 in ypx and 0 in ymx and 0 in ypx
    assert any(r[NL - 1] > F.K8P29[NL - 1] for r in cat["from_record"])  # the top limb fe_sub could not take
    depths = {(k, value_of(u) >= P) for u, _, k in cat["sqrt_ts"] if k is not None}
    assert depths == {(k, hi) for k in range(S.TWO_ADICITY) for hi in (False, True)}
    for u, v, k in cat["sqrt_ts"]:
        assert std(u) == v and (k is None or S.first_round_depth(v) == k)
    assert sum(1 for p, _, _ in cat["mul_order"] if any(value_of(c) >= P for c in p)) >= 6
    # fe_std_neg: a borrow out of every one of the eight low limbs in one row
    assert any(all(a[i] > F.P29[i] for i in range(1, NL - 1)) and a[0] > 1 for a in cat["std_neg"])


@pytest.mark.parametrize("masks", MASK_SETS, ids=("wide", "narrow"))
def test_small_functions(masks):
    cat, exp = L.catalogue(), L.expected(masks)
    for a, r in zip(cat["sqr"], exp["sqr"]):
        assert value_of(r) % P == value_of(a) ** 2 * RINV % P and value_of(r) < 2 * P and normalised(r), a
    for a, r in zip(cat["std_neg"], exp["std_neg"]):
        assert value_of(r) == (P - value_of(a)) % P and all(x <= F.MASK for x in r), a
    hits = 0
    for a, (r,) in zip(cat["is_one"], exp["is_one"]):
        # the comment's claim: among fe_mul outputs (normalised, below 2p) the two patterns are all of 1
        if L.is_mul_output(a):
            assert r == int(std(a) == 1), a
        else:
            assert r == 0, a
        hits += r
    assert hits == 2
    assert sum(1 for a in cat["is_one"] if std(a) == 1 and not L.is_mul_output(a)) >= 2 * (NL - 1)


@pytest.mark.parametrize("masks", MASK_SETS, ids=("wide", "narrow"))
def test_pt_from_record(masks):
    for rec, pt in zip(L.catalogue()["from_record"], L.expected(masks)["from_record"]):
        ymx, ypx = value_of(rec[0:NL]), value_of(rec[F.PRE_HALF:F.PRE_HALF + NL])
        x, y = (ypx - ymx) * RINV % P, (ypx + ymx) * RINV % P
        assert [std(c) for c in pt] == [x, y, x * y % P, 1], rec
        assert all(value_of(c) < 2 * P and normalised(c) for c in pt), rec
    # a record's own point comes back: (x / 2, y / 2) doubled by the addition of the halves
    for aff, _ in L.special_points():
        rec = F.prepare_record(F.be_words(aff[0]) + F.be_words(aff[1]), F.PT_FMT_XY, masks)[0]
        assert affine_of(F.pt_from_record(rec, masks)) == aff


@pytest.mark.parametrize("masks", MASK_SETS, ids=("wide", "narrow"))
def test_shift_lane(masks):
    for (rec, s, aff), out in zip(L.catalogue()["shift_lane"], L.expected(masks)["shift_lane"]):
        vals, limbs = decode_record(out)
        assert vals == expected_record_values(O.scalar_mul(aff, 1 << s)), (aff, s)
        check_record_bounds(limbs)


@pytest.mark.parametrize("masks", MASK_SETS, ids=("wide", "narrow"))
def test_fe_sqrt_ts(masks):
    exp = L.expected(masks)
    for (u, v, k), r, tr in zip(L.catalogue()["sqrt_ts"], exp["sqrt_ts"], exp["sqrt_trace"]):
        ref_tr = []
        assert std(r) == S.sqrt_ts(v, ref_tr), (v, k)        # the integer restatement, round for round
        assert tr == ref_tr and (not k or tr[0] == k), (v, k)
        assert value_of(r) < 2 * P and normalised(r)
        if k is not None or v in (0, 1, 4, S.OMEGA * S.OMEGA % P):
            assert std(r) ** 2 % P == v, (v, k)
        if v in (11, S.OMEGA, 3021):
            assert std(r) ** 2 % P != v


@pytest.mark.parametrize("masks", MASK_SETS, ids=("wide", "narrow"))
def test_pt_mul_order(masks):
    for (p, aff, note), q in zip(L.catalogue()["mul_order"], L.expected(masks)["mul_order"]):
        assert affine_of(p) == aff, note
        check_point(q, O.scalar_mul(aff, O.R_ORDER), note)
    # the two answers k_decompress_x tells apart, and a point it refuses
    res = {note: affine_of(q) for (_, _, note), q in zip(L.catalogue()["mul_order"], L.expected(masks)["mul_order"])}
    assert res["generator multiple"] == O.IDENTITY and res["(0, -1)"] == (0, P - 1)
    assert res["order 4r"] not in (O.IDENTITY, (0, P - 1))


@pytest.mark.parametrize("masks", MASK_SETS, ids=("wide", "narrow"))
def test_fixed_eval_chain(masks):
    rnd = random.Random(77)
    bases = [O.scalar_mul(O.G, 5), O.aff_add(O.scalar_mul(O.G, 9), L.ORDER4[0])]
    w, b = 4, 16
    records, Wn, _ = L.fixed_table(bases, w, b, masks)
    rows = [(0, 0), (1, 0), (1 << (w - 1), (1 << w) - 1), ((1 << b) - 1, (1 << b) - 1)]
    rows += [(rnd.randrange(1 << b), rnd.randrange(1 << b)) for _ in range(8)]
    for row in rows:
        digits = [L.fixed_digits(s, b, w) for s in row]
        assert all(sum(d << (w * i) for i, d in enumerate(ds)) == s for ds, s in zip(digits, row))
        want = O.aff_add(O.scalar_mul(bases[0], row[0]), O.scalar_mul(bases[1], row[1]))
        acc = F.fixed_eval_chain(records, digits, w, Wn, masks)
        check_point(acc, want, row)
    assert F.fixed_eval_chain(records, [[0] * Wn] * 2, w, Wn, masks) == F.pt_identity()
