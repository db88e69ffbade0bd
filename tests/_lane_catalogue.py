"""Operand catalogue of the per-lane point kernels' functions (msm_kernels.hip pt_from_record,
fe_sqrt_ts, pt_mul_order, fe_std_neg, fe_mul_out_is_one, k_shift_bases' lane), shared by the model's
self-check (tests/test_lane_model.py) and the device comparison (tests/test_gpu_lanes.py).

The rows are raw limbs at the extremes of each function's operand forms, not conversions of wire
points: record halves just under their value bounds, both representatives v and v + p of a lazy
value, borrows through every limb.  `in_contract` states each function's contract; the model's
outputs are computed once per mask set and shared (`expected`).
"""
import functools
import random

import _fp29_model as F
import _sqrt_model as S
from _bases_model import RECORD_VALUE_BOUNDS
from _fp29_catalogue import N_EDGES, N_MAX, ORDER2, ORDER4, ext_point, halved_record, mont, plus_p
from _fp29_model import LB, M32, MASK, NL, ONE29, ONE_P29, P, P29, limbs_of, value_of
from oracle import oracle as O

SHIFT_COUNTS = (1, 2, 5, 13)


def normalised(a):
    return all(0 <= x <= MASK for x in a[:NL - 1]) and 0 <= a[NL - 1] <= M32


def is_mul_output(a):
    return normalised(a) and value_of(a) < 2 * P


def _lifted_records(aff, lifts):
    return [F.pack_record(*halved_record(aff, lift)) for lift in lifts]


def special_points():
    """(affine point, note): a subgroup point, the identity, the torsion points, a point of order 4r."""
    g = O.scalar_mul(O.G, 0x1234567)
    return [(g, "generator multiple"), (O.IDENTITY, "identity"), (ORDER2, "(0, -1)"), (ORDER4[0], "(i, 0)"),
            (ORDER4[1], "(-i, 0)"), (O.aff_add(g, ORDER4[0]), "order 4r")]


@functools.lru_cache(maxsize=None)
def catalogue():
    rnd = random.Random(0x1A9E)
    cat = {}

    # ---- fe_sqr: fe_mul outputs at their edges, the doubled form pt_dbl squares, random ----------------
    s_max = F.fe_add(N_MAX, N_MAX)
    cat["sqr"] = [list(a) for a in N_EDGES] + [s_max, list(ONE_P29)] + [limbs_of(rnd.randrange(2 * P)) for _ in range(40)]

    # ---- fe_std_neg: canonical standard-form limbs -----------------------------------------------------
    over = [MASK] * (NL - 1) + [P29[NL - 1] - 1]                    # every low limb above p's: eight borrows
    over1 = [x + 1 for x in P29[:NL - 1]] + [0]                     # each low limb one above p's
    over1[0] = 2
    neg = [limbs_of(v) for v in (0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2)] + [over, over1]
    neg += [limbs_of(1 << (LB * i)) for i in range(NL)] + [limbs_of(MASK << (LB * i)) for i in range(NL - 1)]
    neg += [limbs_of(P29[NL - 1] << (LB * (NL - 1)))]               # the top limb alone: p's own
    neg += [limbs_of(rnd.randrange(P)) for _ in range(30)]
    cat["std_neg"] = neg

    # ---- fe_mul_out_is_one: the two patterns of 1, one limb off, the same value unnormalised -----------
    ones = []
    for base in (ONE29, ONE_P29):
        ones.append(list(base))
        for i in range(NL):
            for d in (1, -1):
                a = list(base)
                a[i] += d
                ones.append(a)
        for i in range(NL - 1):  # value unchanged, limb i one radix richer: must compare false
            a = list(base)
            a[i] += 1 << LB
            a[i + 1] -= 1
            ones.append(a)
    ones += [[0] * NL, list(P29), mont(P - 1), mont(2)] + [limbs_of(rnd.randrange(2 * P)) for _ in range(10)]
    cat["is_one"] = ones

    # ---- pt_from_record: record halves at their bounds ---------------------------------------------------
    ymx_max, ypx_max, kt_max = RECORD_VALUE_BOUNDS
    ymx_rows = [limbs_of(v) for v in (ymx_max - 1, ymx_max - 2 - rnd.randrange(1 << 200), 8 * P - 1, 8 * P, P, 0)]
    ypx_rows = [limbs_of(v) for v in (ypx_max - 1, ypx_max - 2 - rnd.randrange(1 << 200), P, 0)]
    recs = [F.pack_record(a, b, limbs_of(rnd.randrange(kt_max))) for a in ymx_rows for b in ypx_rows]
    lifts = ((0, 0, 0), (9, 3, 1), (8, 0, 1), (0, 3, 0))
    for aff, _ in special_points():
        recs += _lifted_records(aff, lifts)
    recs += [F.pack_record(limbs_of(rnd.randrange(ymx_max)), limbs_of(rnd.randrange(ypx_max)),
                           limbs_of(rnd.randrange(kt_max))) for _ in range(30)]
    cat["from_record"] = recs

    # ---- k_shift_bases' lane: records of curve points, lifted to the bounds, a few doublings ------------
    lanes = []
    pts = [a for a, _ in special_points()] + [O.scalar_mul(O.G, rnd.randrange(1, O.R_ORDER)) for _ in range(2)]
    for n, aff in enumerate(pts):
        lift = lifts[n % len(lifts)]
        lanes.append((_lifted_records(aff, (lift,))[0], SHIFT_COUNTS[n % len(SHIFT_COUNTS)], aff))
    lanes.append((_lifted_records(pts[0], ((9, 3, 1),))[0], 0, pts[0]))
    cat["shift_lane"] = lanes

    # ---- fe_sqrt_ts: every first-round depth, both representatives; the values with no root -------------
    roots = []
    for k in range(S.TWO_ADICITY):
        y = S.depth_input(k, rnd.randrange(2, P))
        u = y * y % P
        roots += [(mont(u), u, k), (plus_p(mont(u)), u, k)]
    for u in (0, 1, P - 1, 11, S.OMEGA, S.OMEGA * S.OMEGA % P, 4, 3021):
        roots.append((mont(u), u, None))
    roots += [(list(P29), 0, None), (list(ONE_P29), 1, None), (plus_p(mont(P - 1)), P - 1, None),
              (plus_p(mont(S.OMEGA)), S.OMEGA, None)]
    cat["sqrt_ts"] = roots

    # ---- pt_mul_order: the special points, each also with p added to one coordinate ----------------------
    order = []
    for n, (aff, note) in enumerate(special_points()):
        p = ext_point(aff)
        order.append((p, aff, note))
        q = list(p)
        q[n % 4] = plus_p(q[n % 4])
        order.append((tuple(q), aff, note + f", coordinate {n % 4} + p"))
    order.append((ext_point(special_points()[0][0], high=True), special_points()[0][0], "generator multiple, all + p"))
    assert len(order) <= 16
    cat["mul_order"] = order
    return cat


def in_contract(op, row):
    """Whether a catalogue row lies inside the contract msm_kernels.hip states for `op`."""
    if op == "sqr":  # fe_mul's: limbs below 2^30, value below 2^257
        return all(0 <= x < 1 << 30 for x in row) and value_of(row) < 1 << 257
    if op == "std_neg":  # canonical standard form
        return normalised(row) and value_of(row) < P
    if op == "is_one":  # any nine limbs: the answer is a limb comparison
        return all(0 <= x <= M32 for x in row)
    if op in ("from_record", "shift_lane"):
        rec = row if op == "from_record" else row[0]
        ymx, ypx = rec[0:NL], rec[F.PRE_HALF:F.PRE_HALF + NL]
        ok = normalised(ymx) and normalised(ypx) and value_of(ymx) < RECORD_VALUE_BOUNDS[0] and \
            value_of(ypx) < RECORD_VALUE_BOUNDS[1]
        return ok and (op == "from_record" or 0 <= row[1] <= 255)
    if op == "sqrt_ts":  # an fe_mul output
        return is_mul_output(row[0])
    if op == "mul_order":  # every coordinate an fe_mul output
        return all(is_mul_output(c) for c in row[0])
    raise KeyError(op)


@functools.lru_cache(maxsize=None)
def expected(masks=F.DEFAULT_MASKS):
    """The model's output for every catalogue row, computed once per mask set."""
    cat = catalogue()
    exp = {
        "sqr": [F.fe_sqr(a, masks) for a in cat["sqr"]],
        "std_neg": [F.fe_std_neg(a) for a in cat["std_neg"]],
        "is_one": [[int(F.fe_mul_out_is_one(a))] for a in cat["is_one"]],
        "from_record": [F.pt_from_record(r, masks) for r in cat["from_record"]],
        "shift_lane": [F.shift_lane(r, s, masks) for r, s, _ in cat["shift_lane"]],
        "mul_order": [F.pt_mul_order(p, masks) for p, _, _ in cat["mul_order"]],
    }
    exp["sqrt_ts"], exp["sqrt_trace"] = [], []
    for u, _, _ in cat["sqrt_ts"]:
        tr = []
        exp["sqrt_ts"].append(F.fe_sqrt_ts(u, masks, tr))
        exp["sqrt_trace"].append(tr)
    return exp


# ---- a small fixed-base table for the addition chain's self-check ---------------------------------------
def fixed_table(bases, w, b, masks=F.DEFAULT_MASKS):
    """(records, Wn, points) of the table msm_fixed_create builds for these affine bases: entry
    (j, win, d) at (j Wn + win) 2^(w-1) + d - 1 holds d 2^(w win) B_j, as k_prepare_points(PT_FMT_XY)
    writes its record."""
    Wn = (b + w) // w
    records, points = [], []
    for base in bases:
        for win in range(Wn):
            q = O.scalar_mul(base, 1 << (w * win))
            acc = O.IDENTITY
            for _ in range(1 << (w - 1)):
                acc = O.aff_add(acc, q)
                points.append(acc)
                records.append(F.prepare_record(F.be_words(acc[0]) + F.be_words(acc[1]), F.PT_FMT_XY, masks)[0])
    return records, Wn, points


def fixed_digits(value, b, w):
    """msm_kernels.hip fixed_digit over fixed_windows(b, w) windows, least significant first."""
    digits, carry = [], 0
    for win in range((b + w) // w):
        v = ((value >> (w * win)) & ((1 << w) - 1) if w * win < b else 0) + carry
        carry = 1 if v > 1 << (w - 1) else 0
        digits.append(v - (carry << w))
    assert carry == 0
    return digits
