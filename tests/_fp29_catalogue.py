"""Operand catalogue of the limb-for-limb checks (tests/test_fp29_model.py on the CPU,
tests/test_gpu_limbs.py on the device): deterministic, seeded, and legal -- every function gets
only operands inside its documented precondition, in the forms its call sites feed it
(tests/test_limb_bounds.py lists those forms).  A model assertion tripping on an entry is a bug in
this file.

catalogue(masks) builds everything once per set of WIDE_* masks (the masks of the library under
test); the entries are lists of Python ints and are never modified.
"""
import functools
import random

from _fp29_model import (DEFAULT_MASKS, K5P29, K8P29, K2D_INT, KD_INT, LB, M32, MASK, NL, ONE29, P, P29, PT_FMT_WIRE,
                         PT_FMT_XY, PT_FMT_XYZ, R, be_words, fe_add, fe_mul_exact, fe_mul_sd_exact, fe_sub_s, is_wide,
                         limbs_of)
from oracle import oracle as O

TOP2P = (2 * P - 1) >> (LB * (NL - 1))  # top limb of the largest fe_mul output
N_MAX = [MASK] * (NL - 1) + [TOP2P]     # all-ones low limbs with the largest legal top limb
MUL_MASK_NAMES = ("all", "gh", "eh", "ef", "gheh")
WIDE_TARGETS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)  # register low word at a wide step
NARROW_TARGETS = (0, MASK)                                   # its low 29 bits at a narrow step


def mul_masks(masks):
    w, gh, eh, ef = masks
    return dict(zip(MUL_MASK_NAMES, (w, gh, eh, ef, gh & eh)))


def mont(v):
    """Canonical Montgomery limbs of the field element v."""
    return limbs_of(v * R % P)


def plus_p(a):
    """The same residue in [p, 2p): normalised limbs of value + p."""
    return limbs_of(sum(x << (LB * i) for i, x in enumerate(a)) + P)


# ---- forms ------------------------------------------------------------------------------------------
def form_maxima():
    """The unnormalised operands of test_limb_bounds.test_fe_mul_exact_model at their forms' maxima."""
    top = (1 << 257) >> (LB * (NL - 1))
    s_max = [(1 << 30) - 1] * (NL - 1) + [top // 2]
    g_max = [3 * (1 << 29) // 2] * (NL - 1) + [top // 4]
    u_max = [k - 1 for k in K8P29]
    v_max = [MASK + k for k in K5P29[:NL - 1]] + [TOP2P + K5P29[NL - 1]]
    return dict(s=s_max, g=g_max, u=u_max, v=v_max)


N_EDGES = [limbs_of(v) for v in (0, 1, P - 1, P, P + 1, 2 * P - 1)] + [list(ONE29), list(N_MAX)]


def rand_n(rnd):
    return limbs_of(rnd.randrange(2 * P))


def rand_form(rnd, form):
    """A random operand in a call site's form, built as the kernels build it."""
    x, y, z = rand_n(rnd), rand_n(rnd), rand_n(rnd)
    if form == "n":
        return x
    if form == "s":
        return fe_add(x, y)
    if form == "g":  # D + D + C
        return fe_add(fe_add(x, x), limbs_of(rnd.randrange(3 * P)))
    if form == "u":
        return [a + k - b for a, k, b in zip(x, K8P29, y)]
    if form == "v":
        return [a + k - b for a, k, b in zip(x, K5P29, y)]
    raise KeyError(form)


# the operand forms each mask's call sites multiply (ec.cuh; fp29.cuh's table of masks)
MASK_FORMS = {
    "all": (("n", "n"), ("s", "n"), ("s", "s"), ("u", "n"), ("v", "n"), ("v", "s"), ("n", "v"), ("n", "g")),
    "gh": (("g", "s"),),
    "eh": (("u", "s"),),
    "ef": (("v", "v"),),
    "gheh": (("u", "n"), ("g", "s"), ("u", "s"), ("n", "g")),
}


# ---- digit edges: fe_mul_w ----------------------------------------------------------------------------
def _step_lo(a, b, wide, k):
    tr = []
    fe_mul_exact(a, b, wide, tr)
    return tr[k][0]


def steer_mul(rnd, wide, k, target):
    """An (N, S)-form operand pair whose step-k register low word (its low 29 bits at a narrow step)
    is `target`: a[0] = 1 and b[0] = 7 make column k take 7 a[k] + b[k] and no lower column
    anything, so the pair is solved from the model's own low word with a[k] = b[k] = 0."""
    mod = 1 << 32 if is_wide(wide, k) else 1 << LB
    a, b = rand_n(rnd), rand_n(rnd)
    if k == 0:
        # column 0 is seed + a0 b0: solve a0 b0 = target + 1 (mod 2^32 | 2^29), the power of two in
        # it shared between a0 = u 2^ea (u odd) and b0
        t = (target + 1) % mod
        if t == 0:
            a[0] = 0
        else:
            ea = ((t & -t).bit_length() - 1) // 2
            for _ in range(10000):
                u = rnd.randrange(1 << (LB - ea)) | 1
                b0 = (t >> ea) * pow(u, -1, mod >> ea) % (mod >> ea)
                if b0 < 1 << 30:
                    break
            else:
                raise AssertionError(f"no operand pair for step 0, low word {target:#x}")
            a[0], b[0] = u << ea, b0
    elif k < NL - 1:
        a[0], b[0] = 1, 7
        a[k] = b[k] = 0
        need = (target - _step_lo(a, b, wide, k)) % mod
        a[k] = min(need // 7, MASK)
        b[k] = need - 7 * a[k]
        assert b[k] < 1 << 30
    else:
        # step 8: the top limbs must stay small, so a lower pair is steered -- with b[0..3] = 0,
        # a[4] b[4] lands in column 8 and in no lower one (a[0] b[8] takes the remainder)
        a[0] = 1
        b[0:5] = [0, 0, 0, 0, 7]
        a[4] = 0
        b[8] = 0
        need = (target - _step_lo(a, b, wide, k)) % mod
        a[4], b[8] = need // 7, need % 7
    lo = _step_lo(a, b, wide, k)
    assert (lo if mod == 1 << 32 else lo & MASK) == target
    return a, b


def mul_digit_targets(wide, k):
    return WIDE_TARGETS if is_wide(wide, k) else NARROW_TARGETS


# ---- digit edges: fe_mul_sd -------------------------------------------------------------------------------
SD_STEPS = 2 * NL - 1  # reduction steps 0..8 and the final carry pass 9..16
# A carry out of columns 15 and 16 is negative for every legal operand pair, so (15, +) and
# (16, +) are no catalogue targets (tests/test_fp29_model.py test_sd_top_carries_are_negative
# re-derives the bound): column 17's register is 2^29 + carry_16 and holds the result's top limb
# (< 2^22), and column 15's register is its true column less 2^58, where the true column -- two
# limb products, the bias, two reduction products and a carry -- stays below 2^57.2.
SD_ONE_SIGN_STEPS = (15, 16)


def rand_sd_pair(rnd, kind):
    x, y, z, w = (rnd.randrange(2 * P) for _ in range(4))
    a = fe_sub_s(limbs_of(x), limbs_of(y))
    if kind == 0:    # A = (Y - X) ymx: ymx normalised, up to 10p
        return a, limbs_of(rnd.randrange(10 * P))
    if kind == 1:    # X3 = E F
        return a, fe_sub_s(limbs_of(z), limbs_of(w))
    return a, fe_add(limbs_of(z), limbs_of(w))  # T3 = E H, Z3 = F G


def steer_sd(rnd, wide, k, t_lo):
    """A (signed, S)-form pair whose step-k register lies in [t_lo, t_lo + 2^30): t_lo = 0 makes
    the signed high word exactly 0 (and a narrow step's carry non-negative), t_lo = -2^32 makes it
    exactly -1 (the carry negative).  Only a[k] is solved, against b[0]: a[k] b[0] is the one
    product of a[k] in column k, and a[k] touches no lower column."""
    for _ in range(20000):
        a, b = rand_sd_pair(rnd, 2)
        if k == 0:
            b0 = b[0] | (1 << 29)
            a0 = ((1 << 58) - (1 << 32) + 1 + t_lo + b0 - 1) // b0  # smallest a0 with the register >= t_lo
            if a0 > MASK:
                continue
            a[0], b[0] = a0, b0
        else:
            if b[0] < 1 << 28:
                continue
            a[k] = 0
            tr = []
            fe_mul_sd_exact(a, b, wide, tr)
            v = (tr[k][3] << 32) | tr[k][0]
            ak = -((v - t_lo) // b[0])  # ceil((t_lo - v) / b0)
            if abs(ak) > MASK:
                continue
            a[k] = ak & M32
        tr = []
        try:
            fe_mul_sd_exact(a, b, wide, tr)
        except AssertionError:
            continue
        reg = (tr[k][3] << 32) | tr[k][0]
        if t_lo <= reg < t_lo + (1 << 30):
            return a, b
    raise AssertionError(f"no signed operand pair found for step {k}, register floor {t_lo}")


def sd_marks(tr, wide):
    """What one traced fe_mul_sd run covers: (step, 'hi', sign | 0 | -1) at wide steps, (step,
    'carry', sign) at narrow and final steps; sign is +1 for >= 0."""
    out = set()
    for k, (_, _, carry, hi) in enumerate(tr):
        if is_wide(wide, k):
            out.add((k, "hi", 1 if hi >= 0 else -1))
            if hi in (0, -1):
                out.add((k, "hi", "zero" if hi == 0 else "minus_one"))
        else:
            out.add((k, "carry", 1 if carry >= 0 else -1))
    return out


def sd_targets(wide):
    t = set()
    for k in range(SD_STEPS):
        if is_wide(wide, k):
            t |= {(k, "hi", 1), (k, "hi", -1), (k, "hi", "zero"), (k, "hi", "minus_one")}
        else:
            t |= {(k, "carry", -1)} | (set() if k in SD_ONE_SIGN_STEPS else {(k, "carry", 1)})
    return t


# ---- points ---------------------------------------------------------------------------------------------------
SQRT_M1 = O.sqrt_mod(P - 1)
ORDER2 = (0, P - 1)
ORDER4 = ((SQRT_M1, 0), (P - SQRT_M1, 0))


def ext_point(aff, z=1, high=False):
    """Extended Montgomery coordinates (X, Y, T, Z) of an affine point scaled by z; `high` puts all
    four in [p, 2p)."""
    x, y = aff
    c = [mont(x * z % P), mont(y * z % P), mont(x * y * z % P), mont(z % P)]
    return tuple(plus_p(v) if high else v for v in c)


def halved_record(aff, lift=(0, 0, 0)):
    """The record of an affine point as pt_madd reads it: ((y-x)/2, (y+x)/2, d x y) in Montgomery
    form; lift adds multiples of p (the record's fields are normalised values up to 10p, 4p, 2p)."""
    x, y = aff
    h = pow(2, -1, P)
    vals = ((y - x) * h % P, (y + x) * h % P, O.EDWARDS_D * x * y % P)
    return tuple(limbs_of(v * R % P + k * P) for v, k in zip(vals, lift))


def curve_points(rnd, n):
    return [O.scalar_mul(O.G, rnd.randrange(1, O.R_ORDER)) for _ in range(n)]


def point_pairs(rnd):
    """(P, Q, note) affine pairs: the special points of the unified addition, then random ones."""
    pts = curve_points(rnd, 6)
    pairs = [(pts[0], pts[0], "P + P"), (pts[1], O.aff_neg(pts[1]), "P + (-P)"),
             (O.IDENTITY, pts[2], "identity + Q"), (pts[2], O.IDENTITY, "P + identity"),
             (O.IDENTITY, O.IDENTITY, "identity + identity"),
             (ORDER2, pts[3], "order 2 + Q"), (pts[3], ORDER2, "P + order 2"), (ORDER2, ORDER2, "order 2 doubled"),
             (ORDER4[0], pts[4], "order 4 + Q"), (pts[4], ORDER4[1], "P + order 4"),
             (ORDER4[0], ORDER4[0], "order 4 doubled"), (ORDER4[0], ORDER4[1], "order 4 + its negative")]
    pairs += [(pts[i], pts[5 - i], "random") for i in range(3)]
    return pairs


QUAD_COUNTS = (1, 15, 16, 17, 65)  # partial waves and dead quads


@functools.lru_cache(maxsize=None)
def catalogue(masks=DEFAULT_MASKS):
    rnd = random.Random(0x29F)
    w_all = masks[0]
    fm = form_maxima()
    cat = {}

    # --- fe_mul_w per mask: form extremes, N edges, digit edges, random fill in the call sites' forms
    cat["mul"] = {}
    for name, wide in mul_masks(masks).items():
        cases = [(a, b) for a in N_EDGES for b in N_EDGES]
        ext = {"all": (("s", "s"), ("v", "s"), ("u", "n"), ("v", "n")), "gh": (("g", "s"),), "eh": (("u", "s"),),
               "ef": (("v", "v"),), "gheh": (("g", "s"), ("u", "s"))}[name]
        cases += [(fm[x] if x != "n" else N_MAX, fm[y] if y != "n" else N_MAX) for x, y in ext]
        for k in range(NL):
            for t in mul_digit_targets(wide, k):
                cases.append(steer_mul(rnd, wide, k, t))
        for fa, fb in MASK_FORMS[name]:
            cases += [(rand_form(rnd, fa), rand_form(rnd, fb)) for _ in range(600 // len(MASK_FORMS[name]))]
        cat["mul"][name] = cases

    # --- fe_mul_sd: interval corners, steered high words and carries, random fill per call site
    neg = [(-x) & M32 for x in N_MAX]
    s_max = [2 * x for x in N_MAX]
    sd = [(a, b) for a in (N_MAX, neg) for b in (N_MAX, neg, s_max)]
    # (the centring offsets SD_OFF58 suit the wide digits' reduction terms: a narrow-digit A/B build
    # keeps its middle registers far below zero, so the steered entries exist for the shipped masks only)
    for k in range(NL - 1 if masks == DEFAULT_MASKS else 0):  # step 8's carry takes both signs in the random fill
        for t_lo in (0, -(1 << 32)):
            sd.append(steer_sd(rnd, w_all, k, t_lo))
    sd += [rand_sd_pair(rnd, kind) for kind in range(3) for _ in range(700)]
    cat["mul_sd"] = sd

    # --- scaling by 2d and d: Barrett boundaries (both sides), the edge list, random fill
    edge = [0, 1, P - 1, P, 2 * P - 1, (1 << 254) - 1, (1 << 253), (1 << 252) - 1]
    v2d = list(edge) + [x for q in range(0, K2D_INT * 2, 97) for dv in (-2, -1, 0, 1)
                        for x in [(q * P) // K2D_INT + dv] if 0 <= x < 1 << 254]
    vd = list(edge) + [x for q in range(0, KD_INT * 2 + 2, 7) for dv in (-2, -1, 0, 1)
                       for x in [(q * P) // KD_INT + dv] if 0 <= x < 1 << 254]
    cat["mul_2d"] = [limbs_of(v) for v in v2d + [rnd.randrange(2 * P) for _ in range(1500)]
                     + [rnd.randrange(1 << 254) for _ in range(500)]]
    cat["mul_d"] = [limbs_of(v) for v in vd + [rnd.randrange(2 * P) for _ in range(1500)]
                    + [rnd.randrange(1 << 254) for _ in range(500)]]

    # --- carries: fe_sub / fe_neg / fe_add_n / fe_dbl_n
    b_max = [MASK] * (NL - 1) + [K8P29[NL - 1]]  # the largest subtrahend K8P dominates limb-wise
    ripple_b = [K8P29[0] - (1 << LB)] + [k - MASK for k in K8P29[1:NL - 1]] + [0]  # 0 - b + 8p = 2^29, MASK, ..., MASK
    zero = [0] * NL
    sub = [(zero, ripple_b), (N_MAX, N_MAX), (zero, zero), (zero, b_max), (fm["s"], b_max), (N_MAX, b_max),
           (fm["s"], zero)]
    sub += [(a, a) for a in N_EDGES] + [(a, b) for a in N_EDGES[:6] for b in N_EDGES[:6]]
    sub += [(rand_form(rnd, "s"), rand_n(rnd)) for _ in range(500)] + [(rand_n(rnd), limbs_of(rnd.randrange(8 * P)))
                                                                        for _ in range(500)]
    cat["sub"] = sub
    cat["neg"] = [zero, ripple_b, b_max] + N_EDGES + [limbs_of(rnd.randrange(4 * P)) for _ in range(800)]
    one = [1] + [0] * (NL - 1)
    cat["add_n"] = ([(N_MAX, one), (one, N_MAX), (N_MAX, N_MAX), (zero, zero)] + [(a, a) for a in N_EDGES]
                    + [(a, b) for a in N_EDGES[:6] for b in N_EDGES[:6]]
                    + [(rand_n(rnd), rand_n(rnd)) for _ in range(800)])
    cat["dbl_n"] = ([zero, N_MAX, [1 << 28] * (NL - 1) + [TOP2P], [(1 << 28) - 1] * (NL - 1) + [0]] + N_EDGES
                    + [rand_n(rnd) for _ in range(800)])

    # --- canonicalisation: results that are exactly p before the conditional subtraction, p - 1, 1
    mult_p = [list(P29), limbs_of(2 * P), limbs_of(8 * P), list(K8P29)]
    cat["to_std"] = (mult_p + [limbs_of(v) for v in ((P - 1) * R % P, (P - 1) * R % P + P, R % P, R % P + P, 0)]
                     + N_EDGES + [rand_n(rnd) for _ in range(800)])
    cat["to_host_mont"] = (mult_p + [limbs_of(v) for v in (32, 32 + P, P - 32, 2 * P - 32, 0, 64, P - 64)]
                           + N_EDGES + [rand_n(rnd) for _ in range(800)])
    cat["inv"] = ([mont(v) for v in (1, 2, P - 1)] + [plus_p(mont(v)) for v in (1, 2, P - 1, 3)]
                  + [plus_p(mont(rnd.randrange(1, P))) for _ in range(12)] + [mont(rnd.randrange(1, P)) for _ in range(12)]
                  + [list(N_MAX)])

    # --- words
    wv = [0, 1, P - 1, P, P + 1, (1 << 256) - 1]
    for k in range(1, NL):
        wv += [1 << (LB * k - 1), 1 << (LB * k)]
    wv += [rnd.randrange(1 << 256) for _ in range(300)] + [rnd.randrange(P) for _ in range(300)]
    le = lambda v: [(v >> (32 * i)) & M32 for i in range(8)]  # noqa: E731
    cat["from_words"] = [le(v) for v in wv]
    cat["to_words"] = [limbs_of(v) for v in wv]
    lt = [le(v) for v in wv]
    pw = le(P)
    for i in range(8):
        for d in (-1, 1):
            if 0 <= pw[i] + d <= M32:
                lt.append(pw[:i] + [pw[i] + d] + pw[i + 1:])
    cat["words_lt_p"] = lt

    # --- points: raw extended coordinates, canonical and in [p, 2p), z = 1 and z != 1
    pairs = point_pairs(rnd)
    cat["pairs"] = pairs
    ext = []
    for pa, qa, note in pairs:
        z1, z2 = rnd.randrange(2, P), rnd.randrange(2, P)
        for hp, hq, zp, zq in ((False, False, 1, 1), (True, True, 1, 1), (True, False, z1, z2), (False, True, z1, 1)):
            ext.append((ext_point(pa, zp, hp), ext_point(qa, zq, hq), (pa, qa, note)))
    cat["pt_add"] = ext
    cat["pt_dbl"] = [(p, (pa, pa, note)) for p, _, (pa, _, note) in ext] + [(q, (qa, qa, note)) for _, q, (_, qa, note) in ext]
    madd = []
    for pa, qa, note in pairs:
        z1 = rnd.randrange(2, P)
        for hp, zp, lift in ((False, 1, (0, 0, 0)), (True, 1, (8, 2, 1)), (True, z1, (0, 0, 0)), (False, z1, (9, 3, 1))):
            for ng in (0, 1):
                madd.append((ext_point(pa, zp, hp), halved_record(qa, lift), ng, (pa, qa, note)))
    cat["pt_madd"] = madd
    quad = {}
    for cnt in QUAD_COUNTS:
        quad[cnt] = [ext[(7 * i + cnt) % len(ext)] for i in range(cnt)]
    cat["pt_add_quad"] = quad

    # --- records: inputs in the three formats (z = 1 and z != 1), entries of both signs
    rec_pts = [O.IDENTITY, ORDER2, ORDER4[0], ORDER4[1]] + curve_points(rnd, 5)
    recs = {}
    for fmt in (PT_FMT_WIRE, PT_FMT_XY, PT_FMT_XYZ):
        inputs, affs = [], []
        for i, (x, y) in enumerate(rec_pts):
            z = 1 if fmt == PT_FMT_XY or i % 2 == 0 else rnd.randrange(2, P)
            xs, ys, ts = x * z % P, y * z % P, x * y * z % P
            words = be_words(xs) + be_words(ys)
            if fmt == PT_FMT_WIRE:
                words += be_words(ts) + be_words(z)
            elif fmt == PT_FMT_XYZ:
                words += be_words(z)
            inputs.append(words)
            affs.append((x, y))
        accs_aff = curve_points(rnd, 2) + [O.IDENTITY]
        ents, accs, notes = [], [], []
        for i in range(len(rec_pts)):
            for sgn in (0, 1):
                for j, acc in enumerate(accs_aff):
                    ents.append(i << 1 | sgn)
                    accs.append(ext_point(acc, 1 if j else rnd.randrange(2, P), high=bool((i + j) & 1)))
                    notes.append((acc, affs[i], sgn))
        # an accumulator that equals the record, and its negative: P + P and P + (-P) through the gather
        for sgn in (0, 1):
            ents.append(5 << 1 | sgn)
            accs.append(ext_point(affs[5], 1, high=True))
            notes.append((affs[5], affs[5], sgn))
        recs[fmt] = dict(inputs=inputs, affine=affs, entries=ents, accs=accs, notes=notes)
    cat["records"] = recs
    return cat
