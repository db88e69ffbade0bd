"""Bit-exact Python model of the device field and curve code (webgpu-msm_amd/csrc/fp29.cuh, ec.cuh,
and the point records of msm_kernels.hip / msm_dev.h), limb for limb.

Every function takes and returns the 9 u32 limbs the device function of the same name holds in
registers (lists of Python ints), and follows its formulas step by step with unbounded integers,
asserting wherever the device's fixed-width registers would wrap: a 64-bit column register, a
32-bit limb, a negative limb.  A tripped assertion therefore means an operand outside the
function's documented precondition, not a wrong answer.

tests/test_limb_bounds.py proves with interval arithmetic that the kernels' call sites stay inside
those preconditions and pins a digest of every mirrored device function (REVIEWED);
tests/test_fp29_model.py checks this model against plain integers; tests/test_gpu_limbs.py compares
the compiled device code with it on every output limb.
"""
P = 8444461749428370424248824938781546531375899335154063827935233455917409239041
NL, LB = 9, 29
MASK = (1 << LB) - 1
M32 = 0xFFFFFFFF
R = 1 << 261
RINV = pow(R, -1, P)
D_COEFF = 3021


def value_of(limbs):
    return sum(x << (LB * i) for i, x in enumerate(limbs))


def limbs_of(v):
    """The normalised representation of v >= 0 (limbs 0..7 < 2^29, the rest in limb 8)."""
    return [(v >> (LB * i)) & MASK for i in range(NL - 1)] + [v >> (LB * (NL - 1))]


def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def signed_value_of(limbs):
    """Value of a signed difference (fe_sub_s): every limb a two's-complement word."""
    return sum(s32(x) << (LB * i) for i, x in enumerate(limbs))


P29 = limbs_of(P)
K8P29 = [536870920, 610271231, 536871443, 661646591, 939568340, 880373981, 718018184, 1050291364, 9788201]
K5P29 = [536870917, 851181567, 536871243, 681964575, 654339076, 550233738, 717196821, 991976422, 6117625]
ONE29 = limbs_of(R % P)
R2_29 = limbs_of(R * R % P)
R2H_29 = limbs_of(R * R * pow(2, -1, P) % P)
HALF29 = limbs_of(R * pow(2, -1, P) % P)
R256_29 = limbs_of((1 << 256) % P)

WIDE_ALL, WIDE_GH, WIDE_EH, WIDE_EF = 0xFF, 0xE7, 0xBF, 0xEF  # fp29.cuh: steps with a 32-bit digit
DEFAULT_MASKS = (WIDE_ALL, WIDE_GH, WIDE_EH, WIDE_EF)
NARROW_MASKS = (0, 0, 0, 0)  # a -DMSM_NARROW_DIGITS build


def seed(wide: int, k: int) -> int:
    """fp29.cuh fe_mul_seed: register offset of column k (2^32 - 1 on the reduction columns, -7
    after a narrow step)."""
    return ((1 << 32) - 1 if k <= NL - 1 else 0) - (7 if k >= 1 and not (wide >> (k - 1)) & 1 else 0)


def is_wide(wide: int, i: int) -> bool:
    return i < NL - 1 and bool((wide >> i) & 1)


def fe_mul_exact(a, b, wide: int = WIDE_ALL, trace=None):
    """Bit-exact model of fp29.cuh fe_mul_w<wide> on limb lists: returns the 9 output limbs.  The
    column registers are kept as true integers and asserted < 2^64 where the device reads them, so
    a wrap is an error here, not a silent difference.  With `trace` (a list) every reduction step
    i = 0..8 appends (register low word, digit, carry into column i + 1)."""
    c = [0] * (2 * NL)
    for k in range(NL + 1):
        c[k] = seed(wide, k)
    for i in range(NL):
        for j in range(NL):
            assert 0 <= a[i] <= M32 and 0 <= b[j] <= M32
            c[i + j] += a[i] * b[j]
    for i in range(NL):
        assert 0 <= c[i] < 1 << 64, f"column {i} wraps"
        lo = c[i] & M32
        if is_wide(wide, i):
            m = ~lo & M32
            carry = 8 * (c[i] >> 32)
        else:
            m = ~lo & MASK
            carry = c[i] >> LB
        c[i + 1] += carry
        if trace is not None:
            trace.append((lo, m, carry))
        for j in range(1, NL):
            c[i + j] += m * P29[j]
    r = [0] * NL
    for k in range(NL, 2 * NL - 1):
        assert 0 <= c[k] < 1 << 64, f"column {k} wraps"
        c[k + 1] += c[k] >> LB
        r[k - NL] = c[k] & MASK
    assert 0 <= c[2 * NL - 1] < 1 << 64
    r[NL - 1] = c[2 * NL - 1] & M32
    return r


# ---- signed differences (fp29.cuh fe_sub_s / fe_mul_sd, pt_madd) ----------------------------------
DELTA_SD_LOG = 26  # fp29.cuh: the bias DELTA_SD p 2^232 added through the seeds of columns 8..16
SD_OFF58 = [-1, -3, -3, -5, -9, -9, -12, -14, -14, -12, -11, -9, -6, -5, -2, -1, -1, 0]  # fp29.cuh: O_k / 2^58


def sd_seed(wide: int, k: int) -> int:
    """fp29.cuh fe_mul_sd_seed as a signed integer: register offset + bias + O_k - O_(k-1) / 2^29."""
    bias = (P29[k - (NL - 1)] << DELTA_SD_LOG) if NL - 1 <= k < 2 * NL - 1 else 0
    return (seed(wide, k) if k <= NL else 0) + bias + (SD_OFF58[k] << 58) - ((SD_OFF58[k - 1] << 29) if k >= 1 else 0)


def fe_mul_sd_exact(a, b, wide: int = WIDE_ALL, trace=None):
    """Bit-exact model of fp29.cuh fe_mul_sd on limb lists (signed limbs; 64-bit two's-complement
    registers, wrap checked against the true integers): returns the 9 output limbs.  With `trace`
    every step k = 0..16 appends (register low word, digit or None, carry into column k + 1, signed
    high word of the register): the reduction steps 0..8, then the final carry pass 9..16."""
    c = [sd_seed(wide, k) for k in range(2 * NL)]  # the registers, as signed integers
    for i in range(NL):
        for j in range(NL):
            c[i + j] += s32(a[i]) * s32(b[j])
    for i in range(NL):
        assert -(1 << 63) <= c[i] < 1 << 63
        lo = c[i] & M32
        hi = s32(c[i] >> 32)
        if is_wide(wide, i):
            m = ~lo & M32
            carry = 8 * hi
        else:
            m = ~lo & MASK
            carry = c[i] >> LB
        c[i + 1] += carry
        if trace is not None:
            trace.append((lo, m, carry, hi))
        for j in range(1, NL):
            c[i + j] += m * P29[j]
    r = [0] * NL
    for k in range(NL, 2 * NL - 1):
        assert -(1 << 63) <= c[k] < 1 << 63
        carry = c[k] >> LB
        if trace is not None:
            trace.append((c[k] & M32, None, carry, s32(c[k] >> 32)))
        c[k + 1] += carry
        r[k - NL] = c[k] & MASK
    assert 0 <= c[2 * NL - 1] < 1 << 32
    r[NL - 1] = c[2 * NL - 1]
    return [x & M32 for x in r]


# ---- scaling by the small constants ---------------------------------------------------------------
K2D_INT, MU2D = 6042, (1 << 284) // P
KD_INT, MU272 = 3021, (1 << 272) // P


def fe_mul_2d_limbs(a):
    """Bit-exact model of fp29.cuh fe_mul_2d on limbs (normalised, value < 2^254)."""
    r, c = [0] * NL, 0
    for i in range(NL - 1):
        c = a[i] * K2D_INT + c
        assert c < 1 << 64
        r[i] = c & MASK
        c >>= LB
    c = a[NL - 1] * K2D_INT + c
    assert c >> 20 < 1 << 32
    q = ((c >> 20) * MU2D) >> 32
    d = 0
    for i in range(NL - 1):
        d += r[i] - q * P29[i]
        assert -(1 << 63) <= d < 1 << 63
        r[i] = d & MASK
        d >>= LB  # Python's >> is arithmetic, like the int64 shift
    r[NL - 1] = d + c - q * P29[NL - 1]
    assert 0 <= r[NL - 1] < 1 << 32
    return r


def fe_mul_2d_exact(v: int):
    """fe_mul_2d on the normalised representation of v (< 2^254): returns (limbs, value)."""
    r = fe_mul_2d_limbs(limbs_of(v))
    return r, value_of(r)


def fe_mul_d_limbs(a):
    """Bit-exact model of fp29.cuh fe_mul_d on limbs (normalised, value < 2^254)."""
    r, c = [0] * NL, 0
    for i in range(NL - 1):
        c = a[i] * KD_INT + c
        assert c < 1 << 64
        r[i] = c & MASK
        c >>= LB
    c = a[NL - 1] * KD_INT + c
    assert c < 1 << 34
    q = ((c >> 8) * MU272) >> 32
    assert q < 1 << 32
    d = 0
    for i in range(NL - 1):
        d += r[i] - q * P29[i]
        assert -(1 << 63) <= d < 1 << 63
        r[i] = d & MASK
        d >>= LB
    r[NL - 1] = d + c - q * P29[NL - 1]
    assert 0 <= r[NL - 1] < 1 << 32
    return r


def fe_mul_d_exact(v: int):
    """fe_mul_d on the normalised representation of v (< 2^254): returns (limbs, value)."""
    r = fe_mul_d_limbs(limbs_of(v))
    return r, value_of(r)


# ---- additions, subtractions, carries --------------------------------------------------------------
def _u32(x, what):
    assert 0 <= x <= M32, f"{what}: limb leaves u32"
    return x


def fe_norm(a):
    a = list(a)
    for i in range(NL - 1):
        a[i + 1] = _u32(a[i + 1] + (a[i] >> LB), "fe_norm")
        a[i] &= MASK
    return a


def fe_add(a, b):
    return [_u32(x + y, "fe_add") for x, y in zip(a, b)]


def fe_add_n(a, b):
    return fe_norm(fe_add(a, b))


def fe_dbl_n(a):
    return fe_norm([_u32(x << 1, "fe_dbl_n") for x in a])


def fe_sub_u(a, b):
    return [_u32(x + k - y, "fe_sub_u") for x, k, y in zip(a, K8P29, b)]


def fe_sub(a, b):
    return fe_norm(fe_sub_u(a, b))


def fe_sub_v(a, b):
    return [_u32(x + k - y, "fe_sub_v") for x, k, y in zip(a, K5P29, b)]


def fe_sub_s(a, b):
    for x, y in zip(a, b):
        assert -(1 << 31) <= x - y < 1 << 31, "fe_sub_s: difference leaves int32"
    return [(x - y) & M32 for x, y in zip(a, b)]


def fe_neg(b):
    return fe_norm([_u32(k - y, "fe_neg") for k, y in zip(K8P29, b)])


def kt_neg_if(kt, neg):
    return [_u32(k - y, "kt_neg_if") for k, y in zip(K5P29, kt)] if neg else list(kt)


# ---- canonical forms, words --------------------------------------------------------------------------
def fe_geq_p(a):
    gt, eq = False, True
    for i in range(NL - 1, -1, -1):
        g, l = a[i] > P29[i], a[i] < P29[i]
        gt = gt or (eq and g)
        eq = eq and not g and not l
    return gt or eq


def fe_sub_p(a):
    r, borrow = [0] * NL, 0
    for i in range(NL):
        t = a[i] - P29[i] + borrow
        borrow = -1 if t < 0 else 0
        r[i] = (t + ((1 << 29) if t < 0 else 0)) & M32
    assert borrow == 0, "fe_sub_p: a < p"
    return r


def fe_mul(a, b, masks=DEFAULT_MASKS):
    return fe_mul_exact(a, b, masks[0])


def fe_to_std(a, masks=DEFAULT_MASKS):
    r = fe_norm(fe_mul(a, [1] + [0] * (NL - 1), masks))
    return fe_sub_p(r) if fe_geq_p(r) else r


def fe_to_host_mont(a, masks=DEFAULT_MASKS):
    r = fe_norm(fe_mul(a, R256_29, masks))
    return fe_sub_p(r) if fe_geq_p(r) else r


def fe_to_mont(a, masks=DEFAULT_MASKS):
    return fe_mul(a, R2_29, masks)


def fe_inv(a, masks=DEFAULT_MASKS):
    r = list(ONE29)
    e = P - 2
    for bit in range(255, -1, -1):
        r = fe_mul(r, r, masks)
        if (e >> bit) & 1:
            r = fe_mul(r, a, masks)
    return r


def fe_from_words_le(w):
    r = [0] * NL
    for i in range(NL):
        bit = 29 * i
        wi, sh = bit >> 5, bit & 31
        lo = w[wi] >> sh
        hi = (w[wi + 1] << (32 - sh)) & M32 if sh > 3 and wi + 1 < 8 else 0
        r[i] = (lo | hi) & MASK
    return r


def fe_to_words_le(a):
    w = [0] * 8
    for i in range(NL):
        bit = 29 * i
        wi, sh = bit >> 5, bit & 31
        w[wi] |= (a[i] << sh) & M32
        if sh > 3 and wi + 1 < 8:
            w[wi + 1] |= a[i] >> (32 - sh)
    return w


PW = [(P >> (32 * i)) & M32 for i in range(8)]


def words_lt_p(w):
    b = 0
    for i in range(8):  # subtract with borrow, word by word
        b = 1 if w[i] - PW[i] - b < 0 else 0
    return b != 0


# ---- points (ec.cuh): (X, Y, T, Z) tuples of limb lists; a record q = (ymx, ypx, kt) ---------------
def pt_identity():
    return ([0] * NL, list(ONE29), [0] * NL, list(ONE29))


def pt_madd(p, q, masks=DEFAULT_MASKS):
    w = masks[0]
    X, Y, T, Z = p
    ymx, ypx, kt = q
    A = fe_mul_sd_exact(fe_sub_s(Y, X), ymx, w)
    B = fe_mul_exact(fe_add(Y, X), ypx, w)
    C = fe_mul_exact(T, kt, w)
    E = fe_sub_s(B, A)
    F = fe_sub_s(Z, C)
    G = fe_add(Z, C)
    H = fe_add(B, A)
    return (fe_mul_sd_exact(E, F, w), fe_mul_exact(G, H, w), fe_mul_sd_exact(E, H, w), fe_mul_sd_exact(F, G, w))


def pt_add(p, q, masks=DEFAULT_MASKS):
    w, gh, _, ef = masks
    A = fe_mul_exact(fe_sub_v(p[1], p[0]), fe_sub_v(q[1], q[0]), ef)
    B = fe_mul_exact(fe_add(p[1], p[0]), fe_add(q[1], q[0]), w)
    C = fe_mul_2d_limbs(fe_mul_exact(p[2], q[2], w))
    D = fe_mul_exact(p[3], q[3], w)
    D = fe_add(D, D)
    E = fe_sub_v(B, A)
    F = fe_sub(D, C)
    G = fe_add(D, C)
    H = fe_add(B, A)
    return (fe_mul_exact(E, F, w), fe_mul_exact(G, H, gh), fe_mul_exact(E, H, w), fe_mul_exact(F, G, w))


def pt_dbl(p, masks=DEFAULT_MASKS):
    w = masks[0]
    X, Y, _, Z = p
    A = fe_mul_exact(X, X, w)
    B = fe_mul_exact(Y, Y, w)
    C = fe_dbl_n(fe_mul_exact(Z, Z, w))
    XY = fe_add(X, Y)
    S = fe_mul_exact(XY, XY, w)
    E = fe_sub(fe_sub(S, A), B)
    G = fe_sub(B, A)
    F = fe_sub(G, C)
    H = fe_neg(fe_add_n(A, B))
    return (fe_mul_exact(E, F, w), fe_mul_exact(G, H, w), fe_mul_exact(E, H, w), fe_mul_exact(F, G, w))


def pt_add_quad(p, r, masks=DEFAULT_MASKS):
    """ec.cuh pt_add_quad, the four lanes of a quad at once: lane c holds coordinate c."""
    w, gh, eh, _ = masks
    X1, Y1, T1, Z1 = p
    X2, Y2, T2, Z2 = r
    s1, a1 = fe_sub_u(Y1, X1), fe_add(Y1, X1)
    s2, a2 = fe_sub(Y2, X2), fe_add(Y2, X2)
    m = [fe_mul_exact(x, y, w) for x, y in ((s1, s2), (a1, a2), (T1, T2), (Z1, Z2))]
    A, B, C, D0 = m[0], m[1], fe_mul_2d_limbs(m[2]), m[3]
    D = fe_add(D0, D0)
    E, F, G, H = fe_sub_u(B, A), fe_sub(D, C), fe_add(D, C), fe_add(B, A)
    return tuple(fe_mul_exact(x, y, gh & eh) for x, y in ((E, F), (G, H), (E, H), (F, G)))


# ---- point records (msm_kernels.hip k_prepare_points / load_pre_signed, msm_dev.h PRE_WORDS) -------
PRE_WORDS, PRE_HALF, PRE_KT = 32, 12, 24
PT_FMT_WIRE, PT_FMT_XY, PT_FMT_XYZ = 0, 1, 2
FMT_WORDS = {PT_FMT_WIRE: 32, PT_FMT_XY: 16, PT_FMT_XYZ: 24}
ERR_COORD_RANGE, ERR_BAD_POINT = 1, 2


def be_words(v):
    """A 256-bit value as the 8 big-endian u32 words of the wire formats."""
    return [(v >> (32 * (7 - i))) & M32 for i in range(8)]


def prepare_record(inp, fmt, masks=DEFAULT_MASKS):
    """k_prepare_points on one input point (its BE words in format fmt): (32 record words, error bits)."""
    f = [list(reversed(inp[8 * i: 8 * i + 8])) for i in range(FMT_WORDS[fmt] // 8)]  # LE words per field
    xw, yw = f[0], f[1]
    tw = f[2] if fmt == PT_FMT_WIRE else [0] * 8
    zw = f[3] if fmt == PT_FMT_WIRE else f[2] if fmt == PT_FMT_XYZ else [1] + [0] * 7
    err = 0
    if not (words_lt_p(xw) and words_lt_p(yw) and words_lt_p(tw) and words_lt_p(zw)):
        err |= ERR_COORD_RANGE
    if all(x == 0 for x in zw):
        err |= ERR_BAD_POINT
    if zw == [1] + [0] * 7:
        x = fe_mul(fe_from_words_le(xw), R2H_29, masks)
        y = fe_mul(fe_from_words_le(yw), R2H_29, masks)
    else:
        zi = fe_inv(fe_to_mont(fe_from_words_le(zw), masks), masks)
        zh = fe_mul(zi, HALF29, masks)
        x = fe_mul(fe_to_mont(fe_from_words_le(xw), masks), zh, masks)
        y = fe_mul(fe_to_mont(fe_from_words_le(yw), masks), zh, masks)
    return halved_record(x, y, masks), err


def pack_record(ymx, ypx, kt):
    """The 32 words of a record (msm_dev.h PRE_WORDS) from its three limb vectors."""
    rec = [0] * PRE_WORDS
    rec[0:NL] = ymx
    rec[PRE_HALF:PRE_HALF + NL] = ypx
    rec[PRE_KT:PRE_KT + NL - 1] = kt[:NL - 1]
    rec[NL] = rec[PRE_HALF + NL] = kt[NL - 1]
    rec[NL + 1] = ypx[NL - 1]
    rec[PRE_HALF + NL + 1] = ymx[NL - 1]
    return rec


def halved_record(x, y, masks=DEFAULT_MASKS):
    """The record k_prepare_points and k_shift_bases write for the halved affine (x / 2, y / 2) they
    hold as fe_mul outputs: (y-x)/2 = fe_sub, (y+x)/2 = fe_add_n, d t = fe_mul_d(2x 2y)."""
    kt = fe_mul_d_limbs(fe_mul(fe_add(x, x), fe_add(y, y), masks))
    return pack_record(fe_sub(y, x), fe_add_n(y, x), kt)


def load_pre_signed(records, ent):
    """msm_kernels.hip load_pre_signed: the record of entry `ent` (index << 1 | sign) as the point it
    adds -- the half at PRE_HALF * sign read first (it supplies all three top limbs), d t negated."""
    rec, sgn = records[ent >> 1], ent & 1
    h0, h1 = rec[PRE_HALF * sgn: PRE_HALF * sgn + PRE_HALF], rec[PRE_HALF * (1 - sgn): PRE_HALF * (1 - sgn) + PRE_HALF]
    av = list(h0[:NL])
    bv = list(h1[:NL - 1]) + [h0[NL + 1]]
    kv = list(rec[PRE_KT:PRE_KT + NL - 1]) + [h0[NL]]
    return (av, bv, kt_neg_if(kv, sgn != 0))


# ---- the per-lane point kernels (msm_kernels.hip k_shift_bases, k_decompress_x, k_scale_points, ----
# ---- k_fixed_build, k_fixed_eval) -------------------------------------------------------------------
def fe_sqr(a, masks=DEFAULT_MASKS):
    return fe_mul(a, a, masks)


ONE_P29 = fe_add_n(ONE29, P29)  # fe_sqrt_ts' one_p: the other limb pattern of 1 below 2p


def fe_eq_limbs(a, b):
    return all(x == y for x, y in zip(a, b))


def fe_mul_out_is_one(t):
    return fe_eq_limbs(t, ONE29) or fe_eq_limbs(t, ONE_P29)


def fe_std_neg(a):
    """p - a on canonical standard-form limbs (0 stays 0): int32 differences with a running borrow."""
    r, borrow, any_ = [0] * NL, 0, 0
    for i in range(NL):
        assert 0 <= a[i] < 1 << 31, "fe_std_neg: limb leaves int32"
        t = P29[i] - a[i] + borrow
        borrow = -1 if t < 0 else 0
        r[i] = t & MASK
        any_ |= a[i]
    assert borrow == 0 or not any_, "fe_std_neg: a > p"
    return r if any_ else list(a)


TWO_ADICITY = 47
Q_ODD = (P - 1) >> TWO_ADICITY
SQRT_EXP, SQRT_EXP_BITS = (Q_ODD - 1) // 2, 7 * 32  # dx_exp_word: DX_EXP_WORDS words, every bit walked
OMEGA = pow(11, Q_ODD, P)                            # 11 is the least non-residue
OMEGA29 = limbs_of(OMEGA * R % P)                    # dx_omega_limb
R_ORDER = 2111115437357092606062206234695386632838870926408408195193685246394721360383
ORDER_BITS = 251


def fe_sqrt_ts(u, masks=DEFAULT_MASKS, trace=None):
    """msm_kernels.hip fe_sqrt_ts on limbs; `trace` collects every round's i."""
    w = list(ONE29)
    for bit in range(SQRT_EXP_BITS - 1, -1, -1):
        w = fe_sqr(w, masks)
        if (SQRT_EXP >> bit) & 1:
            w = fe_mul(w, u, masks)
    r = fe_mul(u, w, masks)
    t = fe_mul(r, w, masks)
    c = list(OMEGA29)
    m = TWO_ADICITY
    while not fe_mul_out_is_one(t):
        i, t2 = 0, t
        while True:
            t2 = fe_sqr(t2, masks)
            i += 1
            if not (i < m and not fe_mul_out_is_one(t2)):
                break
        if i >= m:
            break
        b = c
        for _ in range(i + 1, m):
            b = fe_sqr(b, masks)
        c = fe_sqr(b, masks)
        t = fe_mul(t, c, masks)
        r = fe_mul(r, b, masks)
        m = i
        if trace is not None:
            trace.append(i)
    return r


def pt_mul_order(p, masks=DEFAULT_MASKS):
    acc = pt_identity()
    for k in range(ORDER_BITS - 1, -1, -1):
        acc = pt_dbl(acc, masks)
        if (R_ORDER >> k) & 1:
            acc = pt_add(acc, p, masks)
    return acc


def pt_from_record(rec, masks=DEFAULT_MASKS):
    """The extended point (x : y : x y : 1) of a halved record, as k_shift_bases, k_scale_points and
    pt_from_record rebuild it."""
    ymx, ypx = list(rec[0:NL]), list(rec[PRE_HALF:PRE_HALF + NL])
    one = list(ONE29)
    a = fe_mul(ymx, one, masks)
    xs = fe_sub(ypx, a)
    ys = fe_add_n(ypx, a)
    return (fe_mul(xs, one, masks), fe_mul(ys, one, masks), fe_mul(xs, ys, masks), one)


def shift_lane(rec, S, masks=DEFAULT_MASKS):
    """One lane of k_shift_bases: the record of 2^S Q from the record of Q."""
    p = pt_from_record(rec, masks)
    for _ in range(S):
        p = pt_dbl(p, masks)
    zh = fe_mul(fe_inv(p[3], masks), HALF29, masks)
    return halved_record(fe_mul(p[0], zh, masks), fe_mul(p[1], zh, masks), masks)


def fixed_entry(j, win, d, w, Wn):
    """k_fixed_eval's entry (record << 1 | sign) of digit d != 0 of base j, window win."""
    return ((((j * Wn + win) << (w - 1)) + abs(d) - 1) << 1) | (1 if d < 0 else 0)


def fixed_eval_chain(records, digits, w, Wn, masks=DEFAULT_MASKS):
    """k_fixed_eval's accumulator after one row: digits[j][win] the signed digits of base j's scalar,
    added base-major, windows ascending, zero digits skipped."""
    acc = pt_identity()
    for j, ds in enumerate(digits):
        for win, d in enumerate(ds):
            if d:
                acc = pt_madd(acc, load_pre_signed(records, fixed_entry(j, win, d, w, Wn)), masks)
    return acc
