"""Static limb-bound proof for the device field/curve code (webgpu-msm_amd/csrc/fp29.cuh, ec.cuh).

The 29-bit-limb lazy Montgomery multiply accumulates up to 18 partial products per 64-bit column
with no carry handling, and the curve formulas feed unnormalised sums/differences into it.  A
column overflow would be a silent, data-dependent wrong answer that random tests hit almost
never, so this test walks every formula in the kernels with per-limb worst-case bounds (interval
arithmetic on the limb maxima) and asserts:

  * every fe_mul column stays < 2^64 (products + reduction terms + incoming carry);
  * every fe_mul operand pair keeps a*b < p * 2^261, so the lazy result is < 2p (no final
    subtraction needed);
  * fe_sub / fe_neg never produce a negative limb (K8P dominates the subtrahend limb-wise);
  * pt_madd's signed differences (fe_sub_s) keep every fe_mul_sd column register inside int64
    (per-limb intervals, with the centring offsets SD_OFF58) and its biased result in [0, 2p).

It mirrors the kernels by hand; test_mirrored_sources_unchanged pins a digest of every mirrored
function body, so an edit to fp29.cuh / ec.cuh fails until the model here is re-reviewed.
"""
# the constants and the bit-exact models (fe_mul_exact, fe_mul_sd_exact, fe_mul_2d_exact, fe_mul_d_exact)
# live in tests/_fp29_model.py, shared with the limb-for-limb device comparison (tests/test_gpu_limbs.py)
from _fp29_model import (DELTA_SD_LOG, K2D_INT, K5P29, K8P29, KD_INT, LB, MASK, NL, P, P29, R,  # noqa: F401
                         SD_OFF58, WIDE_ALL, WIDE_EF, WIDE_EH, WIDE_GH, fe_mul_2d_exact, fe_mul_d_exact,
                         fe_mul_exact, fe_mul_sd_exact, sd_seed, seed, value_of)


class B:
    """Worst-case limb maxima + value maximum of a field element."""

    def __init__(self, limbs, value):
        self.l = list(limbs)
        self.v = value

    @staticmethod
    def normalised(value):
        top = value >> (LB * (NL - 1))
        return B([MASK] * (NL - 1) + [top], value)


N_MUL = B.normalised(2 * P)  # fe_mul output: normalised, value < 2p


def digit_max(wide: int, i: int) -> int:
    return (1 << 32) - 1 if i < NL - 1 and (wide >> i) & 1 else (1 << LB) - 1


def fe_mul(a: B, b: B, wide: int = WIDE_ALL) -> B:
    # the digits add sum_i m_i 2^(29 i) p to the product before the division by R
    extra = sum(digit_max(wide, i) << (LB * i) for i in range(NL)) * P
    assert a.v * b.v + extra < 2 * P * R, "lazy Montgomery output would exceed 2p"
    cols = [0] * (2 * NL)
    for i in range(NL):
        for j in range(NL):
            cols[i + j] += a.l[i] * b.l[j]
    carry = 0
    for k in range(2 * NL):
        red = sum(digit_max(wide, i) * P29[k - i] for i in range(NL) if 1 <= k - i < NL)
        # the register: true column (products + reduction terms + incoming carry) + its seed
        col = cols[k] + red + carry
        assert col + max(0, seed(wide, k)) < 1 << 64, f"column {k} may reach {col / 2**64:.3f} * 2^64"
        # carry out: (column + digit) / 2^29 on the reduction columns, column >> 29 above
        carry = (col + digit_max(wide, k)) >> LB if k < NL else col >> LB
    return N_MUL


def fe_mul_2d(a: B) -> B:
    assert all(x <= MASK for x in a.l[:NL - 1]) and a.v < 1 << 254
    return B.normalised(3 * P)


def fe_add(a: B, b: B) -> B:
    return B([x + y for x, y in zip(a.l, b.l)], a.v + b.v)


def fe_sub_u(a: B, b: B) -> B:
    for i in range(NL):
        assert K8P29[i] >= b.l[i], "fe_sub: negative limb possible"
    assert b.v < 8 * P
    return B([x + k for x, k in zip(a.l, K8P29)], a.v + 8 * P)


def fe_sub_v(a: B, b: B) -> B:
    """a + 5p - b (fp29.cuh fe_sub_v): b must be an fe_mul output (normalised, < 2p)."""
    for i in range(NL):
        assert K5P29[i] >= b.l[i], "fe_sub_v: negative limb possible"
    assert b.v <= 2 * P  # B.v is an exclusive bound
    return B([x + k for x, k in zip(a.l, K5P29)], a.v + 5 * P)


def fe_norm(a: B) -> B:
    return B.normalised(a.v)


def fe_sub(a: B, b: B) -> B:
    for i in range(NL - 1):
        assert a.l[i] < 1 << 30
    return fe_norm(fe_sub_u(a, b))


def fe_neg_v(b: B) -> B:  # kt_neg_if's unnormalised 5p - kt
    for i in range(NL):
        assert K5P29[i] >= b.l[i]
    assert b.v <= 2 * P  # B.v is an exclusive bound
    return B(list(K5P29), 5 * P)


# point coordinates are always fe_mul outputs (or the identity's normalised constants)
PT = dict(X=N_MUL, Y=N_MUL, T=N_MUL, Z=N_MUL)
ONE29 = 536870474 + (276299775 << 29)  # value of Montgomery one is < p; covered by N_MUL


# ---- signed differences (fp29.cuh fe_sub_s / fe_mul_sd, pt_madd) ----------------------------------
class SB:
    """Interval bounds of a field element with signed limbs: per-limb [lo, hi] and value [vlo, vhi]
    (all inclusive)."""

    def __init__(self, lo, hi, vlo, vhi):
        self.lo, self.hi, self.vlo, self.vhi = list(lo), list(hi), vlo, vhi

    @staticmethod
    def of(b: B) -> "SB":  # an unsigned form (exclusive value bound b.v)
        return SB([0] * NL, list(b.l), 0, b.v - 1)


def sb_add(a: SB, b: SB) -> SB:
    return SB([x + y for x, y in zip(a.lo, b.lo)], [x + y for x, y in zip(a.hi, b.hi)], a.vlo + b.vlo, a.vhi + b.vhi)


def fe_sub_s(a: SB, b: SB) -> SB:
    return SB([x - y for x, y in zip(a.lo, b.hi)], [x - y for x, y in zip(a.hi, b.lo)], a.vlo - b.vhi, a.vhi - b.vlo)


def _ival_mul(a0, a1, b0, b1):
    c = (a0 * b0, a0 * b1, a1 * b0, a1 * b1)
    return min(c), max(c)


def fe_mul_sd(a: SB, b: SB, wide: int = WIDE_ALL) -> B:
    """fp29.cuh fe_mul_sd: signed 32x32 products, signed carries, result biased by DELTA_SD p / 2^29.
    Asserts every operand limb fits an int32, every column register fits an int64, and the result
    lies in [0, 2p) -- i.e. it is an ordinary fe_mul output (N_MUL)."""
    for x in a.lo + b.lo:
        assert x >= -(1 << 31)
    for x in a.hi + b.hi:
        assert x < 1 << 31
    delta = 1 << DELTA_SD_LOG
    bias = [delta * P29[k - (NL - 1)] if NL - 1 <= k < 2 * NL - 1 else 0 for k in range(2 * NL)]
    lo, hi = [0] * (2 * NL), [0] * (2 * NL)
    for i in range(NL):
        for j in range(NL):
            x0, x1 = _ival_mul(a.lo[i], a.hi[i], b.lo[j], b.hi[j])
            lo[i + j] += x0
            hi[i + j] += x1
    clo = chi = 0
    for k in range(2 * NL):
        red = sum(digit_max(wide, i) * P29[k - i] for i in range(NL) if 1 <= k - i < NL)
        col_lo = lo[k] + bias[k] + clo
        col_hi = hi[k] + bias[k] + red + chi
        off = seed(wide, k) if k <= NL else 0  # register offset (2^32 - 1, -7), then the centring offset O_k
        o = SD_OFF58[k] << 58
        assert -(1 << 63) <= col_lo + min(0, off) + o and col_hi + max(0, off) + o < 1 << 63, \
            f"column {k} leaves int64"
        if k < NL:  # (column + digit) / 2^29, floor
            clo, chi = col_lo >> LB, (col_hi + digit_max(wide, k)) >> LB
        else:
            clo, chi = col_lo >> LB, col_hi >> LB
    t0, t1 = _ival_mul(a.vlo, a.vhi, b.vlo, b.vhi)
    extra = sum(digit_max(wide, i) << (LB * i) for i in range(NL)) * P
    X = delta * P << (LB * (NL - 1))
    assert t0 + X >= 0, "fe_mul_sd result may be negative"
    assert t1 + X + extra < 2 * P * R, "fe_mul_sd result may reach 2p"
    return N_MUL


def test_madd_bounds():
    # halved record from record_from_halved (k_prepare_points, k_shift_bases): ymx = fe_sub (normalised),
    # ypx = fe_add_n, kt = fe_mul_d of an fe_mul output
    madd_bounds(fe_sub(N_MUL, N_MUL), fe_norm(fe_add(N_MUL, N_MUL)), N_MUL)


def madd_bounds(ymx: B, ypx: B, kt: B):
    """pt_madd(acc, q) for acc an fe_mul-output point (or the identity) and q a record of these forms,
    gathered with either sign."""
    for neg in (False, True):
        # the gather swaps the halves of a negated point (load_pre_signed); kt_neg_if negates d t
        q_ymx, q_ypx = (ypx, ymx) if neg else (ymx, ypx)
        q_kt = fe_neg_v(kt) if neg else kt
        X = Y = T = Z = SB.of(N_MUL)
        A = fe_mul_sd(fe_sub_s(Y, X), SB.of(q_ymx))
        Bv = fe_mul(fe_add(N_MUL, N_MUL), q_ypx)
        C = fe_mul(N_MUL, q_kt)
        E = fe_sub_s(SB.of(Bv), SB.of(A))
        F = fe_sub_s(Z, SB.of(C))
        G = fe_add(N_MUL, C)
        H = fe_add(Bv, A)
        fe_mul_sd(E, F)
        fe_mul(G, H)
        fe_mul_sd(E, SB.of(H))
        fe_mul_sd(F, SB.of(G))


def test_sd_offsets_match_header():
    src = open(os.path.join(_CSRC, "fp29.cuh")).read()
    m = re.search(r"SD_OFF58\[2 \* NL\] = \{([^}]*)\}", src)
    assert [int(x) for x in m.group(1).split(",")] == SD_OFF58
    assert int(re.search(r"DELTA_SD_LOG = (\d+);", src).group(1)) == DELTA_SD_LOG


def test_fe_mul_sd_exact_model():
    """fe_mul_sd is a b R^-1 mod p with a normalised result < 2p, for signed differences of fe_mul
    outputs against the unsigned forms pt_madd feeds it, random and at the interval corners."""
    import random
    rnd = random.Random(17)
    Rinv = pow(R, -1, P)

    def limbs(v):
        return [(v >> (LB * i)) & MASK for i in range(NL - 1)] + [v >> (LB * (NL - 1))]

    def diff(x, y):  # fe_sub_s on limbs (two's complement words)
        return [(p - q) & 0xFFFFFFFF for p, q in zip(limbs(x), limbs(y))]

    def sval(l):
        return sum((x - (1 << 32) if x >> 31 else x) << (LB * i) for i, x in enumerate(l))

    top = [MASK] * (NL - 1)
    cases = []
    for _ in range(2000):
        x, y, z, w = (rnd.randrange(2 * P) for _ in range(4))
        u = rnd.randrange(10 * P)
        cases.append((diff(x, y), limbs(u)))                      # A = (Y - X) ymx
        cases.append((diff(x, y), diff(z, w)))                    # X3 = E F
        cases.append((diff(x, y), limbs(z + w)))                  # T3 = E H, Z3 = F G (sums of two)
    # limb extremes: 0 - max and max - 0 in every limb, against maximal unsigned operands
    mx = top + [(2 * P - 1) >> (LB * (NL - 1))]
    neg = [(-x) & 0xFFFFFFFF for x in mx]
    s_max = [2 * x for x in mx]
    for a in (mx, neg):
        for b in (mx, neg, s_max):
            cases.append((a, b))
    for a, b in cases:
        r = fe_mul_sd_exact(a, b)
        v = value_of(r)
        assert v % P == sval(a) * sval(b) * Rinv % P
        assert 0 <= v < 2 * P and all(x <= MASK for x in r[:NL - 1])


def test_halved_record_is_the_same_point():
    """pt_madd with the halved record ((y-x)/2, (y+x)/2, d t) and D = Z1 returns the textbook
    add-2008-hwcd-3 sum (2d, D = 2 Z1) scaled by 1/4: the same projective point."""
    import random
    rnd = random.Random(3)
    d = 3021
    inv2 = pow(2, -1, P)
    for _ in range(50):
        X1, Y1, Z1 = (rnd.randrange(1, P) for _ in range(3))
        T1 = X1 * Y1 * pow(Z1, -1, P) % P
        x2, y2 = rnd.randrange(1, P), rnd.randrange(1, P)
        t2 = x2 * y2 % P
        # textbook
        A = (Y1 - X1) * (y2 - x2); Bv = (Y1 + X1) * (y2 + x2); C = T1 * 2 * d * t2; D = 2 * Z1
        E, F, G, H = Bv - A, D - C, D + C, Bv + A
        ref = [v % P for v in (E * F, G * H, E * H, F * G)]
        # halved record, D = Z1
        A = (Y1 - X1) * (y2 - x2) * inv2; Bv = (Y1 + X1) * (y2 + x2) * inv2; C = T1 * d * t2; D = Z1
        E, F, G, H = Bv - A, D - C, D + C, Bv + A
        got = [v % P for v in (E * F, G * H, E * H, F * G)]
        assert all(g * 4 % P == r for g, r in zip(got, ref))


def padd_operands():
    """pt_add_quad's operands (U-form differences, as before pt_add moved to the V form)."""
    p = q = PT
    A = fe_mul(fe_sub_u(p["Y"], p["X"]), fe_sub(q["Y"], q["X"]))
    Bv = fe_mul(fe_add(p["Y"], p["X"]), fe_add(q["Y"], q["X"]))
    C = fe_mul_2d(fe_mul(p["T"], q["T"]))
    D0 = fe_mul(p["Z"], q["Z"])
    D = fe_add(D0, D0)
    E = fe_sub_u(Bv, A)
    F = fe_sub(D, C)
    G = fe_add(D, C)
    H = fe_add(Bv, A)
    return E, F, G, H


def test_padd_bounds():
    padd_bounds(PT, PT)


def padd_bounds(p, q):
    """ec.cuh pt_add on two points of these coordinate forms; the sum's coordinates (fe_mul outputs)."""
    A = fe_mul(fe_sub_v(p["Y"], p["X"]), fe_sub_v(q["Y"], q["X"]), WIDE_EF)
    Bv = fe_mul(fe_add(p["Y"], p["X"]), fe_add(q["Y"], q["X"]))
    C = fe_mul_2d(fe_mul(p["T"], q["T"]))
    D0 = fe_mul(p["Z"], q["Z"])
    D = fe_add(D0, D0)
    E = fe_sub_v(Bv, A)
    F = fe_sub(D, C)
    G = fe_add(D, C)
    H = fe_add(Bv, A)
    return dict(X=fe_mul(E, F), Y=fe_mul(G, H, WIDE_GH), T=fe_mul(E, H), Z=fe_mul(F, G))


def test_mul_2d_exact_and_bounded():
    import random
    rnd = random.Random(11)
    vals = [0, 1, P - 1, P, 2 * P - 1, (1 << 254) - 1, (1 << 253), (1 << 252) - 1]
    vals += [rnd.randrange(0, 2 * P) for _ in range(20000)] + [rnd.randrange(0, 1 << 254) for _ in range(5000)]
    # values straddling every Barrett boundary q p of 6042 v
    for q in range(0, 6042 * 2, 97):
        for dv in (-2, -1, 0, 1):
            x = (q * P) // K2D_INT + dv
            if 0 <= x < 1 << 254:
                vals.append(x)
    for v in vals:
        limbs, r = fe_mul_2d_exact(v)
        assert r % P == (K2D_INT * v) % P
        assert 0 <= r < 3 * P
        assert all(x <= MASK for x in limbs[:NL - 1])


def test_mul_d_exact_and_below_2p():
    # k_prepare_points: d t = fe_mul_d(fe_mul(x + x, y + y)); the result must be normalised and
    # < 2p like an fe_mul output (pt_madd's C and kt_neg_if's 5p - kt rely on it)
    import random
    rnd = random.Random(12)
    vals = [0, 1, P - 1, P, 2 * P - 1, (1 << 254) - 1, (1 << 253), (1 << 252) - 1]
    vals += [rnd.randrange(0, 2 * P) for _ in range(20000)] + [rnd.randrange(0, 1 << 254) for _ in range(5000)]
    for q in range(0, KD_INT * 2 + 2, 7):  # every Barrett boundary q p of 3021 v, both sides
        for dv in (-2, -1, 0, 1):
            x = (q * P) // KD_INT + dv
            if 0 <= x < 1 << 254:
                vals.append(x)
    for v in vals:
        limbs, r = fe_mul_d_exact(v)
        assert r % P == (KD_INT * v) % P
        assert 0 <= r < 2 * P, (v, r)
        assert all(x <= MASK for x in limbs[:NL - 1])
    # the multiply before it: two doubled fe_mul outputs (S form, value < 4p) meet in fe_mul
    x2 = fe_add(B.normalised(2 * P - 1), B.normalised(2 * P - 1))
    fe_mul(x2, x2)


def test_quad_add_bounds():
    # pt_add_quad: round 1 A | B | T1T2 | Z1Z2 on the four lanes, C = fe_mul_2d(T1T2) on lane 2,
    # then EF | GH | EH | FG -- the same operands as pt_add, through one multiply whose wide steps
    # suit all four (WIDE_GH & WIDE_EH)
    E, F, G, H = padd_operands()
    for a, b in ((E, F), (G, H), (E, H), (F, G)):
        fe_mul(a, b, WIDE_GH & WIDE_EH)


def test_wide_masks_are_maximal():
    """The masks in fp29.cuh are the widest the column budget allows for their operand forms."""
    N = N_MUL
    G, H, E, V = fe_add(fe_add(N, N), N), fe_add(N, N), fe_sub_u(N, N), fe_sub_v(N, N)
    for (a, b), mask in (((G, H), WIDE_GH), ((E, H), WIDE_EH), ((V, V), WIDE_EF)):
        fe_mul(a, b, mask)
        for extra in range(8):
            if not (mask >> extra) & 1:
                try:
                    fe_mul(a, b, mask | 1 << extra)
                except AssertionError:
                    continue
                raise AssertionError(f"mask {mask:#x} could also widen step {extra}")


def test_fe_mul_exact_model():
    """Bit-exact model of fe_mul_w: a b R^-1 mod p, normalised limbs, value < 2p -- random
    operands and operands at the limb maxima of each call site's forms."""
    import random
    rnd = random.Random(5)
    Rinv = pow(R, -1, P)

    def limbs_of(v):
        return [(v >> (LB * i)) & MASK for i in range(NL - 1)] + [v >> (LB * (NL - 1))]

    cases = []
    for _ in range(3000):
        cases.append((limbs_of(rnd.randrange(2 * P)), limbs_of(rnd.randrange(2 * P)), rnd.choice(
            (WIDE_ALL, WIDE_GH, WIDE_EH, WIDE_EF, WIDE_GH & WIDE_EH, 0))))
    # unnormalised operands at their forms' maxima (value = sum of limbs 2^(29 i), kept < 2^257)
    top = (1 << 257) >> (LB * (NL - 1))
    s_max = [(1 << 30) - 1] * (NL - 1) + [top // 2]
    g_max = [3 * (1 << 29) // 2] * (NL - 1) + [top // 4]
    u_max = [x + k - 1 for x, k in zip([0] * NL, K8P29)]
    v_max = [MASK + k for k in K5P29[:NL - 1]] + [((2 * P) >> (LB * (NL - 1))) + K5P29[NL - 1]]
    for a, b, w in ((g_max, s_max, WIDE_GH), (u_max, s_max, WIDE_EH), (s_max, s_max, WIDE_ALL),
                    (v_max, v_max, WIDE_EF), (v_max, s_max, WIDE_ALL)):
        cases.append((a, b, w))
    for a, b, w in cases:
        r = fe_mul_exact(a, b, w)
        v = value_of(r)
        assert v % P == value_of(a) * value_of(b) * Rinv % P
        assert v < 2 * P and all(x <= MASK for x in r[:NL - 1])


def test_pdbl_bounds():
    pdbl_bounds(PT)


def pdbl_bounds(p):
    """ec.cuh pt_dbl on a point of these coordinate forms; the double's coordinates (fe_mul outputs)."""
    A = fe_mul(p["X"], p["X"])
    Bv = fe_mul(p["Y"], p["Y"])
    Z2 = fe_mul(p["Z"], p["Z"])
    C = fe_norm(fe_add(Z2, Z2))
    S = fe_mul(fe_add(p["X"], p["Y"]), fe_add(p["X"], p["Y"]))
    E = fe_sub(fe_sub(S, A), Bv)
    G = fe_sub(Bv, A)
    F = fe_sub(G, C)
    AB = fe_norm(fe_add(A, Bv))
    H = fe_norm(fe_sub_u(B([0] * NL, 0), AB))
    return dict(X=fe_mul(E, F), Y=fe_mul(G, H), T=fe_mul(E, H), Z=fe_mul(F, G))


def test_model_matches_header_constants():
    assert value_of(K8P29) == 8 * P
    assert all(k >= MASK for k in K8P29[:8])
    assert value_of(K5P29) == 5 * P
    assert all(k >= MASK for k in K5P29[:8]) and K5P29[8] >= (2 * P - 1) >> (LB * 8)
    assert P29 == [1, 277610496, 66, 351141280, 452990362, 110046747, 358187729, 198395284, 1223525]


# --- the proof above mirrors these device functions by hand.  Their normalised source text is
# pinned here, so editing any of them fails this test until the mirrored formulas (and this
# table) are re-reviewed.  Regenerate a digest with _body_digest(<file>, <name>).
import hashlib  # noqa: E402
import os  # noqa: E402
import re  # noqa: E402

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "webgpu-msm_amd", "csrc")
REVIEWED = {
    ("fp29.cuh", "mad64"): "b50540a0d8a64ede",
    ("fp29.cuh", "seeded"): "d5de263bcd90d0e8",
    ("fp29.cuh", "fe_mul"): "cb1d67f3d0051cb5",
    ("fp29.cuh", "fe_mul_w"): "9fc551211780fac2",
    ("fp29.cuh", "fe_mul_seed"): "d98e5e7e34126a6e",
    ("fp29.cuh", "fe_norm"): "37b756e7bd4474d2",
    ("fp29.cuh", "fe_add"): "d14b6a137a6ff34d",
    ("fp29.cuh", "fe_add_n"): "bdf7dd24032e38f7",
    ("fp29.cuh", "fe_dbl_n"): "07019b3ba4e2775f",
    ("fp29.cuh", "fe_sub"): "ea72835f159885cc",
    ("fp29.cuh", "fe_sub_u"): "3dba987a0530b5b5",
    ("fp29.cuh", "fe_neg"): "a754b1a94a6b8415",
    ("fp29.cuh", "fe_mul_2d"): "b9f5c6afdcbc7ff4",
    ("fp29.cuh", "fe_mul_d"): "be44d19d0395d3fb",
    ("fp29.cuh", "P29"): "b4babf5a3c9d7331",
    ("fp29.cuh", "K8P29"): "13315f5ba6ec470d",
    ("fp29.cuh", "K5P29"): "f3dc542f8a39d740",
    ("fp29.cuh", "fe_sub_v"): "b95cf1f871e652b6",
    ("fp29.cuh", "fe_sub_s"): "2394a6c588a7e363",
    ("fp29.cuh", "smad64"): "f570120e573dc55c",
    ("fp29.cuh", "SD_OFF58"): "c88a1438ac9f5b80",
    ("fp29.cuh", "fe_mul_sd_seed"): "d2395c468f273ed7",
    ("fp29.cuh", "opaque_v"): "9936fb9d6abd51ca",
    ("fp29.cuh", "fe_mul_sd"): "1524d4c9c2554e87",
    ("ec.cuh", "pt_madd"): "940afc2112f7fd6f",
    ("ec.cuh", "pt_add"): "1449f0a88822c610",
    ("ec.cuh", "pt_dbl"): "784353f9934ef437",
    ("ec.cuh", "kt_neg_if"): "19c79f3cf45dee09",
    ("ec.cuh", "pt_add_quad"): "875eba21c1f11e82",
    # mirrored by the limb-exact model only (tests/_fp29_model.py, compared with the device by
    # tests/test_gpu_limbs.py)
    ("fp29.cuh", "opaque_s"): "46cf266b295cbf08",
    ("fp29.cuh", "fe_sqr"): "f8e70a3f2dd0089a",
    ("fp29.cuh", "fe_geq_p"): "4eb5d532c3233462",
    ("fp29.cuh", "fe_sub_p"): "d1a009c0411c837b",
    ("fp29.cuh", "fe_to_std"): "b8ce08d971edfe7f",
    ("fp29.cuh", "fe_to_host_mont"): "307abc9eeb63e40d",
    ("fp29.cuh", "fe_to_mont"): "1504f8a92b704f1a",
    ("fp29.cuh", "fe_from_words_le"): "452047bc0d4e746b",
    ("fp29.cuh", "fe_to_words_le"): "75b7e2c51d7e06c8",
    ("fp29.cuh", "words_lt_p"): "7561894852928329",
    ("fp29.cuh", "fe_inv"): "7178747f7853f144",
    ("fp29.cuh", "ONE29"): "e27181d893aa29eb",
    ("fp29.cuh", "R2_29"): "a66b69c23bcae68b",
    ("fp29.cuh", "R2H_29"): "67d729fb41ed6ee0",
    ("fp29.cuh", "HALF29"): "fb513a1a00dd9fdd",
    ("fp29.cuh", "R256_29"): "d4cab8ce33c9709c",
    ("msm_kernels.hip", "k_prepare_points"): "dbf1e8d8c7910cf4",
    ("msm_kernels.hip", "load_pre_signed"): "05db1a9e570b7dcc",
    # the per-lane point kernels: mirrored by the proofs at the end of this file, by the limb-exact
    # models of tests/_fp29_model.py (compared with the device by tests/test_gpu_lanes.py), or both
    ("msm_kernels.hip", "pt_from_record"): "65c79ec907d4f2d4",
    ("msm_kernels.hip", "fe_sqrt_ts"): "ccf73a991a94e3af",
    ("msm_kernels.hip", "pt_mul_order"): "600edd33b364daaf",
    ("msm_kernels.hip", "fe_std_neg"): "9e7074f7530e4424",
    ("msm_kernels.hip", "fe_mul_out_is_one"): "d0b82e8a0a18d7de",
    ("msm_kernels.hip", "fe_eq_limbs"): "3692a860963bb15f",
    # the lane frame: the helpers that hold field code or a limb layout (rec[32] <-> slots, words <-> slots)
    ("msm_kernels.hip", "record_from_halved"): "9ca1278c4dccbb09",
    ("msm_kernels.hip", "lane_read_record"): "5e0294e9f8020f58",
    ("msm_kernels.hip", "lane_gather_record"): "dac88734a06a41b0",
    ("msm_kernels.hip", "lane_put_record"): "6fb72bb7c188c881",
    ("msm_kernels.hip", "lane_stage_words"): "b7ffb7a516e0e1b0",
    ("msm_kernels.hip", "lane_stage_affine"): "c76c0f00406dd582",
    ("msm_kernels.hip", "fx_norm_prefix"): "6b51be8e8612ca6d",
    ("msm_kernels.hip", "fx_norm_emit"): "9db8989a95464049",
    ("msm_kernels.hip", "k_shift_bases"): "f0d08d8c3998f392",
    ("msm_kernels.hip", "k_decompress_x"): "f9e7902f9984724f",
    ("msm_kernels.hip", "k_scale_points"): "bfde00ebbfd9ffd9",
    ("msm_kernels.hip", "k_fixed_build"): "70a4acb75279aa06",
    ("msm_kernels.hip", "k_fixed_eval"): "5098db9f158c1bc0",
    ("msm_kernels.hip", "k_fixed_normalise"): "d1986b0a91989aff",
    ("msm_kernels.hip", "dx_omega_limb"): "b1639a51b5be8512",
    ("msm_kernels.hip", "dx_exp_word"): "0551f4741ef8d48c",
    ("msm_kernels.hip", "dx_order_word"): "d22ee440cc326040",
}


def _source(fname):
    src = open(os.path.join(_CSRC, fname)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def _closing(src, i):
    """Index of the bracket that closes the one at src[i]."""
    pair = {"(": ")", "{": "}", "[": "]"}[src[i]]
    depth = 0
    for j in range(i, len(src)):
        depth += 1 if src[j] == src[i] else -1 if src[j] == pair else 0
        if depth == 0:
            return j
    raise AssertionError(f"unbalanced {src[i]} at {i}")


def _body(fname, name):
    """The definition of `name` (a function, a kernel or a constant table), from the start of its
    line to its closing brace, whitespace squeezed.  The parameter list may span lines and hold
    parentheses of its own (array references)."""
    src = _source(fname)
    for m in re.finditer(r"[^\n;{}]*\b" + re.escape(name) + r"\b", src):
        i = m.end()
        for opener in "[(=":
            while src[i].isspace():
                i += 1
            if src[i] == opener:
                i = i + 1 if opener == "=" else _closing(src, i) + 1
        while src[i].isspace():
            i += 1
        if src[i] == "{":
            return " ".join(src[m.start():_closing(src, i) + 1].split())
    raise AssertionError(f"{name} not found in {fname}")


def _body_digest(fname, name):
    return hashlib.sha256(_body(fname, name).encode()).hexdigest()[:16]


def test_mirrored_sources_unchanged():
    changed = {f"{f}:{n}": _body_digest(f, n) for (f, n), d in REVIEWED.items() if _body_digest(f, n) != d}
    assert not changed, ("device code mirrored by this proof changed -- re-check the formulas above, then update "
                         f"REVIEWED with: {changed}")


def test_wide_mask_constants_match_header():
    src = open(os.path.join(_CSRC, "fp29.cuh")).read()
    got = {k: int(v, 16) for k, v in re.findall(r"constexpr uint32_t (WIDE_[A-Z]+) = (0x[0-9A-Fa-f]+)u;", src)}
    assert got == {"WIDE_ALL": WIDE_ALL, "WIDE_GH": WIDE_GH, "WIDE_EH": WIDE_EH, "WIDE_EF": WIDE_EF}


# ---- the per-lane point kernels (msm_kernels.hip k_shift_bases, k_decompress_x, k_scale_points, ----
# ---- k_fixed_build, k_fixed_eval, k_fixed_normalise) ------------------------------------------------
# One lane runs a whole chain of field code per point.  The proofs below walk each chain's call sites
# with the interval machinery above, starting from the record forms k_prepare_points' proof derives
# (test_madd_bounds; _bases_model.RECORD_VALUE_BOUNDS: (y-x)/2 < 10p, (y+x)/2 < 4p, d t < 2p).
import _fp29_model as FM  # noqa: E402
from _bases_model import RECORD_VALUE_BOUNDS  # noqa: E402


def const_form(limbs) -> B:
    """A constant operand: its own limbs and value."""
    return B(limbs, value_of(limbs) + 1)


def within(a: B, bound: B) -> bool:
    return all(x <= y for x, y in zip(a.l, bound.l)) and a.v <= bound.v


ONE_B, HALF_B, R2_B = const_form(FM.ONE29), const_form(FM.HALF29), const_form(FM.R2_29)
UNIT_B = const_form([1] + [0] * (NL - 1))  # fe_to_std's multiplier
REC_YMX, REC_YPX, REC_KT = (B.normalised(v) for v in RECORD_VALUE_BOUNDS)
IDENTITY_PT = dict(X=const_form([0] * NL), Y=ONE_B, T=const_form([0] * NL), Z=ONE_B)


def fe_mul_d(a: B) -> B:
    """fp29.cuh fe_mul_d's input contract: normalised, value < 2^254.  Its output is an fe_mul output
    (test_mul_d_exact_and_below_2p)."""
    assert all(x <= MASK for x in a.l[:NL - 1]) and a.v <= 1 << 254, "fe_mul_d: operand outside its contract"
    return N_MUL


def fe_inv(a: B) -> B:
    """fp29.cuh fe_inv: r = 1, then r = fe_sqr(r) and r = fe_mul(r, a) bit by bit, so r is ONE29 or an
    fe_mul output at every multiply."""
    for r in (ONE_B, N_MUL):
        fe_mul(r, r)
        fe_mul(r, a)
    return N_MUL


def fe_to_std(a: B) -> B:
    return fe_mul(a, UNIT_B)


def from_record_bounds(ymx: B, ypx: B):
    """msm_kernels.hip pt_from_record, the only place the rebuild exists (test_record_rebuild_is_one_text):
    k_shift_bases, k_scale_points, k_fixed_build and k_test_limbs_lane call it."""
    a = fe_mul(ymx, ONE_B)                # (y-x)/2, N_MUL
    xs = fe_sub(ypx, a)                   # x + 8p: normalised, < 12p
    assert within(xs, B.normalised(12 * P))
    ys = fe_norm(fe_add(ypx, a))          # y: normalised, < 6p
    assert within(ys, B.normalised(6 * P))
    X = fe_mul(xs, ONE_B)
    Y = fe_mul(ys, ONE_B)
    assert xs.v * ys.v <= 72 * P * P < P * R  # the comment's "72 p^2 < p R"
    T = fe_mul(xs, ys)
    p = dict(X=X, Y=Y, T=T, Z=ONE_B)
    assert all(within(c, N_MUL) for c in p.values())
    return p


def test_from_record_bounds():
    # why (y-x)/2 takes the multiply by R first: its top limb may pass K8P's, which fe_sub would wrap
    assert REC_YMX.l[NL - 1] > K8P29[NL - 1]
    assert within(fe_sub(N_MUL, N_MUL), REC_YMX) and within(fe_norm(fe_add(N_MUL, N_MUL)), REC_YPX)
    from_record_bounds(REC_YMX, REC_YPX)


def shift_epilogue_bounds(p):
    """k_shift_bases from fe_inv(p.Z) on -- its zh, x and y, then record_from_halved: the three limb vectors
    of the record it writes."""
    zh = fe_mul(fe_inv(p["Z"]), HALF_B)
    x = fe_mul(p["X"], zh)
    y = fe_mul(p["Y"], zh)
    kt = fe_mul_d(fe_mul(fe_add(x, x), fe_add(y, y)))
    return fe_sub(y, x), fe_norm(fe_add(y, x)), kt


def test_shift_bases_closure():
    """The records k_shift_bases writes satisfy the bounds of the records it reads, so level j + 1 may
    feed level j + 2 and pt_madd (madd_bounds) alike."""
    p0 = from_record_bounds(REC_YMX, REC_YPX)
    p1 = pdbl_bounds(p0)   # the first doubling meets Z = 1, the later ones fe_mul outputs
    p2 = pdbl_bounds(p1)
    assert all(within(c, N_MUL) for c in p2.values())
    for p in (p0, p1, p2):
        for out, bound in zip(shift_epilogue_bounds(p), (REC_YMX, REC_YPX, REC_KT)):
            assert within(out, bound), "k_shift_bases writes a record outside the bounds it reads"
    madd_bounds(REC_YMX, REC_YPX, REC_KT)


def _omega_limbs():
    m = re.search(r"W\[NL\] = \{([^}]*)\}", _body("msm_kernels.hip", "dx_omega_limb"))
    return [int(x.strip().rstrip("u")) for x in m.group(1).split(",")]


def sqrt_ts_bounds(u: B):
    """msm_kernels.hip fe_sqrt_ts: w, r, t, t2, b and c are 1, omega or fe_mul outputs, and every
    multiply takes two of them or u."""
    omega = _omega_limbs()
    assert all(x <= MASK for x in omega) and value_of(omega) < P, "dx_omega_limb: not normalised below p"
    forms = (ONE_B, const_form(omega), N_MUL, u)
    for a in forms:
        for b in forms:
            fe_mul(a, b)
    return N_MUL


def test_omega_is_the_model_s():
    omega = _omega_limbs()
    assert omega == FM.OMEGA29
    w = value_of(omega) * FM.RINV % P
    assert pow(w, 1 << 47, P) == 1 and pow(w, 1 << 46, P) == P - 1


def decompress_prologue_bounds():
    """k_decompress_x from the x words to u = (x^2 + 1) / (1 - d x^2), and the point its ladder takes."""
    xw = B.normalised(1 << 256)            # fe_from_words_le: eight words, normalised
    xm = fe_mul(xw, R2_B)                  # fe_to_mont
    x2 = fe_mul(xm, xm)
    num = fe_norm(fe_add(x2, ONE_B))       # normalised, < 3p
    assert within(num, B.normalised(3 * P))
    den = fe_sub(ONE_B, fe_mul_d(x2))      # normalised, < 9p: one of the forms fe_inv receives
    assert within(den, B.normalised(10 * P))
    u = fe_mul(num, fe_inv(den))
    r = sqrt_ts_bounds(u)
    fe_to_std(fe_mul(r, r))
    fe_to_std(u)
    return dict(X=xm, Y=r, T=fe_mul(xm, r), Z=ONE_B)


def test_decompress_bounds():
    p = decompress_prologue_bounds()
    assert all(within(c, N_MUL) for c in p.values())


def ladder_step(acc, p):
    """pt_add(pt_dbl(pt_dbl(acc)), p): a window of k_scale_points; k_fixed_build's and pt_mul_order's
    pt_add(pt_dbl(acc), p) is the same pair of call sites."""
    out = padd_bounds(pdbl_bounds(pdbl_bounds(acc)), p)
    assert all(within(c, N_MUL) for c in out.values())
    return out


def test_ladder_closure():
    rebuilt = from_record_bounds(REC_YMX, REC_YPX)
    for p1 in (rebuilt, decompress_prologue_bounds(), PT):
        p2 = pdbl_bounds(p1)             # k_scale_points' table: P, 2P, 3P and the identity
        p3 = padd_bounds(p2, p1)
        for acc in (IDENTITY_PT, PT):
            for q in (IDENTITY_PT, p1, p2, p3):
                acc = ladder_step(acc, q)
            padd_bounds(pdbl_bounds(acc), p1)  # k_fixed_build, pt_mul_order


def stage_affine_bounds(x: B, y: B):
    """lane_stage_affine (k_scale_points, k_fixed_build, k_fixed_normalise): three canonical forms, handed
    to lane_stage_words as words."""
    fe_to_std(x)
    fe_to_std(y)
    fe_to_std(fe_mul(x, y))


def test_remaining_call_sites():
    # fe_inv's first multiply, for every form it is called with
    fe_inv(N_MUL)                                     # k_shift_bases, k_scale_points, k_fixed_*: a Z
    fe_inv(ONE_B)                                     # the identity's
    fe_inv(fe_sub(ONE_B, N_MUL))                      # k_decompress_x: 1 - d x^2, an fe_sub output
    fe_inv(B.normalised(10 * P))
    # k_scale_points / k_fixed_build: one inversion per lane
    zi = fe_inv(N_MUL)
    stage_affine_bounds(fe_mul(N_MUL, zi), fe_mul(N_MUL, zi))
    # k_fixed_normalise: Z is a pt_madd output or the identity's 1 (lanes past m)
    for z in (N_MUL, ONE_B):
        prefix = fe_mul(z, z)                         # fx_norm_prefix
        prefix = fe_mul(prefix, z)
        inv = fe_inv(prefix)
        inv = fe_inv(z)                               # E = 1: prefix[0] itself
        zi = fe_mul(inv, prefix)                      # fx_norm_emit
        inv = fe_mul(inv, z)
        stage_affine_bounds(fe_mul(N_MUL, zi), fe_mul(N_MUL, zi))
        stage_affine_bounds(fe_mul(N_MUL, inv), fe_mul(N_MUL, inv))
    # k_fixed_eval: the table's records are k_prepare_points' (PT_FMT_XY): test_madd_bounds' operands
    madd_bounds(fe_sub(N_MUL, N_MUL), fe_norm(fe_add(N_MUL, N_MUL)), N_MUL)


# ---- the record-rebuilding prologue and the record epilogue exist once ----------------------------
def _squeezed(fname):
    return " ".join(_source(fname).split())


def _statements(text, start, end):
    text = text[text.index(start):]
    text = text[:text.index(end) + len(end)]
    return [" ".join(st.split()) for st in text.split(";")]


def _calls(kernel, helper):
    return re.search(r"\b%s\(" % re.escape(helper), _body("msm_kernels.hip", kernel)) is not None


def test_record_rebuild_is_one_text():
    """No kernel rebuilds a record's point with statements of its own: every right-hand side of
    pt_from_record's field code occurs once in msm_kernels.hip, and the kernels that rebuild call it."""
    src = _squeezed("msm_kernels.hip")
    ref = _statements(_body("msm_kernels.hip", "pt_from_record"), "const fe one", "p.Z = one")
    assert len(ref) == 9
    field = [st.split(" = ", 1)[1] for st in ref if re.search(r"= fe_(mul|sub|add_n)\(", st)]
    assert len(field) == 6 and field[0] == "fe_mul(ymx, one)"
    for rhs in field:
        assert src.count(rhs) == 1, f"{rhs} occurs {src.count(rhs)} times"
    for kernel in ("k_shift_bases", "k_scale_points", "k_fixed_build", "k_test_limbs_lane"):
        assert _calls(kernel, "pt_from_record"), f"{kernel} does not call pt_from_record"


def test_shift_lane_hook_runs_the_kernel_s_statements():
    """The record epilogue (d t, the two halves, the duplicated top limbs) exists once, in
    record_from_halved; k_prepare_points, k_shift_bases and k_test_limbs_lane's LOP_SHIFT_LANE call it,
    and the hook rebuilds with pt_from_record as the kernel does."""
    src = _squeezed("msm_kernels.hip")
    body = _body("msm_kernels.hip", "record_from_halved")
    for text in ("fe_mul_d(fe_mul(fe_add(x, x), fe_add(y, y)))", "rec[NL] = rec[PRE_HALF + NL] =", "rec[NL + 1] =",
                 "rec[PRE_HALF + NL + 1] =", "rec[PRE_KT + k] ="):
        assert body.count(text) == 1 and src.count(text) == 1, f"{text} occurs {src.count(text)} times"
    for kernel in ("k_prepare_points", "k_shift_bases", "k_test_limbs_lane"):
        assert _calls(kernel, "record_from_halved"), f"{kernel} does not call record_from_halved"
    assert _calls("k_test_limbs_lane", "pt_from_record")
