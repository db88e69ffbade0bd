"""Python restatement of the resident-bases fold (include/msm.h msm_bases_*) and the
decoding of a handle's point records, for tests/test_bases_plan.py and tests/test_gpu_bases.py.

The limb arithmetic and the record layout come from tests/_fp29_model.py."""
import _fp29_model as F

MAIN_BITS = 254  # msm_dev.h: bits the main windows cover; one 3-bit overflow window follows


def geometry(c):
    """The library's balanced windows at width c (host_plan.h make_plan): widths and bit offsets of
    the Wm = wm + 1 windows, least significant first."""
    wm = (MAIN_BITS + c - 1) // c
    q = MAIN_BITS // wm
    nhi = MAIN_BITS - q * wm
    bits = [q + 1 if w < nhi else q for w in range(wm)] + [3]
    off = [w * q + min(w, nhi) for w in range(wm + 1)]
    return bits, off


def fold(c, k):
    """(Wc, S) of k levels at width c: Wc the smallest window count with k (off(Wc) - 1) >= 256,
    S = off(Wc) - 1.  k = 1: every window, no cut (S reported as 256)."""
    bits, off = geometry(c)
    if k == 1:
        return len(bits), 256
    for w in range(1, len(off)):
        if k * (off[w] - 1) >= 256:
            return w, off[w] - 1
    raise AssertionError("no fold")


def recode(v, c, windows):
    """The library's carry recode (msm_kernels.hip recode) of v over the first `windows` windows:
    (digits, carry out of the last of them, bits of v above them)."""
    bits, _ = geometry(c)
    digits, carry = [], 0
    for w in range(windows):
        b = bits[w]
        x = (v & ((1 << b) - 1)) + carry
        v >>= b
        if x > 1 << (b - 1):
            digits.append(x - (1 << b))
            carry = 1
        else:
            digits.append(x)
            carry = 0
    return digits, carry, v


def cut(s, k, S):
    """The k virtual scalars of s: bits [j S, (j + 1) S)."""
    return [(s >> (j * S)) & ((1 << S) - 1) for j in range(k)]


def decode_record(rec):
    """A 32-word record -> ((y-x)/2, (y+x)/2, d x y) as field values, plus its three limb vectors;
    checks the duplicated top limbs and the zero words of the layout (msm_dev.h PRE_WORDS)."""
    rec = [int(x) for x in rec]
    ymx = rec[0:F.NL]
    ypx = rec[F.PRE_HALF:F.PRE_HALF + F.NL]
    kt = rec[F.PRE_KT:F.PRE_KT + F.NL - 1] + [rec[F.NL]]
    assert rec[F.PRE_HALF + F.NL] == kt[F.NL - 1]
    assert rec[F.NL + 1] == ypx[F.NL - 1] and rec[F.PRE_HALF + F.NL + 1] == ymx[F.NL - 1]
    assert rec[11] == 0 and rec[23] == 0
    vals = tuple(F.value_of(l) * F.RINV % F.P for l in (ymx, ypx, kt))
    return vals, (ymx, ypx, kt)


def expected_record_values(pt):
    """((y-x)/2, (y+x)/2, d x y) of an affine point."""
    x, y = pt
    h = pow(2, -1, F.P)
    return ((y - x) * h % F.P, (y + x) * h % F.P, F.D_COEFF * x * y % F.P)


# The limb bounds k_shift_bases' comment cites (tests/test_limb_bounds.py test_madd_bounds' record
# operand): limbs 0..7 normalised, and the value -- hence the top limb -- below 10p for (y-x)/2
# (fe_sub of two fe_mul outputs), 4p for (y+x)/2 (their normalised sum), 2p for d t (N_MUL).
RECORD_VALUE_BOUNDS = (10 * F.P, 4 * F.P, 2 * F.P)


def check_record_bounds(limbs3):
    for limbs, vmax in zip(limbs3, RECORD_VALUE_BOUNDS):
        assert all(0 <= x <= F.MASK for x in limbs[:F.NL - 1]), limbs
        assert F.value_of(limbs) < vmax, (limbs, vmax)
