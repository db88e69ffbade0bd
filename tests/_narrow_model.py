"""The narrow-scalar geometry (include/msm.h MSM_FLAG_SCALAR_BITS) restated in plain Python, for
tests/test_narrow_plan.py and tests/test_gpu_narrow.py: the windows of a b-bit scalar at width c, the
signed recode over them, and the scalars that sit on its carry edges."""


def geometry(b, c):
    """Window widths (least significant first) of a b-bit scalar, b <= 253, at width c: balanced
    over T = max(b + 1, 4) bits, the lowest T mod W' windows one bit wider."""
    T = max(b + 1, 4)
    W = -(-T // c)
    q, nhi = divmod(T, W)
    return [q + 1 if w < nhi else q for w in range(W)]


def auto_width(n, b, c0):
    """The width a narrow launch of n terms takes with window_bits = 0, from the size's usual width
    c0: 17 where the widest window at c0 would hold 64 entries per bucket or more and 17 widens it."""
    widest = lambda c: max(geometry(b, c))  # noqa: E731
    if c0 < 17 and n >> (widest(c0) - 1) >= 64 and widest(17) > widest(c0):
        return 17
    return c0


def offsets(widths):
    off, out = 0, []
    for w in widths:
        out.append(off)
        off += w
    return out


def recode(s, widths):
    """Signed digits of s over `widths`, digit in [-(2^(w-1) - 1), 2^(w-1)], and the carry out of
    the top window."""
    digits, carry = [], 0
    for w in widths:
        v = (s & ((1 << w) - 1)) + carry
        s >>= w
        if v > 1 << (w - 1):
            digits.append(v - (1 << w))
            carry = 1
        else:
            digits.append(v)
            carry = 0
    return digits, carry + s


def edge_scalars(b, c):
    """0, 1, 2^b - 1 (the full carry ripple), 2^(b-1), and for every window the values that put
    2^(w-1) - 1, 2^(w-1) and 2^(w-1) + 1 into it (the carry edge of the signed recode), alone and
    under an all-ones tail (a carry arriving from below); only values below 2^b."""
    vals = {0, 1, (1 << b) - 1, 1 << (b - 1)}
    widths = geometry(b, c)
    for w, off in zip(widths, offsets(widths)):
        for v in ((1 << (w - 1)) - 1, 1 << (w - 1), (1 << (w - 1)) + 1):
            vals.add(v << off)
            vals.add((v << off) | ((1 << off) - 1))
    return sorted(v for v in vals if v < 1 << b)
