"""A catalogue of bucket layouts for the bucket reduction (tests/_red_model.py), and the MSM inputs
that produce each of them on the device.

A shape is a window width c and the entries of a few buckets, (window, bucket, entries), each the
smallest that reaches its branch classes of the reduction: tests/test_red_model.py checks that the
union of the shapes' classes is the model's whole list and that every condition the model can flip is
caught by some shape.  Points and scalars come from tests/_acc_catalogue.py (Rec, Shape, inputs):
P_i = (K0 + i STEP) G, and scalars whose signed digits are exactly the recipe.

The chunk length L is the plan's own (8 up to c = 16, 16 above, on the default device shape) unless a
shape names one: those run only with MSM_RED_L set, in a child process (`env`).  `slow` marks the two
shapes with large bucket tables.
"""
import numpy as np

import _acc_catalogue as C
import _acc_model as A
import _red_model as RM

K = 16  # run_length of every shape but the crossing one


def _shape(name, c, entries, doc, L=None, env=None, slow=False, K=K):
    r = C.Rec(c, K)
    for w, b, size in sorted(entries):
        key = w * r.B + b
        r.to_key(key)
        assert r.reachable(key), (name, w, b)
        r.sizes.append(size)
        r.pos += size
    s = C.Shape(name, r, doc)
    s.L, s.env, s.slow = L, dict(env or {}), slow
    return s


def _c8_bucket0():
    """c = 8 (B = 128, 16 chunks, one group, 4 chunk bits < RG_LOG): only bucket 0 of window 0."""
    return _shape("c8_bucket0", 8, [(0, 0, 3)], _c8_bucket0.__doc__)


def _c8_bucket_top():
    """Only bucket B - 1 of a full-width window (digit 2^(c-1)): the last chunk, every bit of its index set,
    the bucket at the top of its chunk."""
    return _shape("c8_bucket_top", 8, [(0, 127, 2), (3, 127, 1)], _c8_bucket_top.__doc__)


def _c8_sweep():
    """A position sweep: chunk j of window 0 holds only bucket j mod 8; window 1 has chunks holding {0, 7},
    {3, 4} and all 8; windows 2 to 5 one bucket each, at the top, the bottom and the middle of a chunk."""
    e = [(0, 8 * j + j % 8, 1 + j % 2) for j in range(16)]
    e += [(1, 0, 1), (1, 7, 2), (1, 8 + 3, 1), (1, 8 + 4, 1)] + [(1, 16 + i, 1 + i % 3) for i in range(8)]
    e += [(2, 31, 2), (3, 40, 1), (4, 77, 1), (4, 78, 1), (5, 5, 3)]
    return _shape("c8_sweep", 8, e, _c8_sweep.__doc__)


def _c8_empty_mid():
    """Windows 0 and 5 populated, 1 to 4 empty: run right after c8_sweep on the same slot, so that red_G of
    windows 1 to 4 still holds the sweep's group points when k_red2_terms runs."""
    return _shape("c8_empty_mid", 8, [(0, 9, 2), (0, 100, 1), (5, 64, 2), (5, 65, 1)], _c8_empty_mid.__doc__)


def _c8_top7bit():
    """The top reachable bucket of a 7-bit window in the 8-bit table, number 63 of window 31 (the last live
    chunk), the chunks above it empty; window 31's offset is 30 * 8 + 7, not 31 * 8."""
    return _shape("c8_top7bit", 8, [(31, 63, 2), (31, 56, 1), (30, 63, 1), (2, 1, 1)], _c8_top7bit.__doc__)


def _c8_overflow():
    """Three non-canonical scalars (>= 2^254) that fill buckets 0 to 2 of the overflow window: entries in a
    chunk that red1_lane counts dead.  (The lower buckets' keys are multiples of 3: positive digits.)"""
    return _shape("c8_overflow", 8, [(32, 0, 1), (32, 1, 1), (32, 2, 1), (0, 3, 2), (7, 121, 1)], _c8_overflow.__doc__)


def _c4_one_chunk():
    """c = 4 (B = 8 = L): one chunk per window, one V slice, no bit term (nterms = 1), 65 windows."""
    return _shape("c4_one_chunk", 4, [(0, 3, 1), (0, 7, 1), (5, 0, 2), (63, 2, 1), (64, 1, 1)], _c4_one_chunk.__doc__)


def _c12_edges():
    """c = 12 (B = 2048, 256 chunks, two groups): entries in chunks 0, 127, 128 and 255 of window 0, and one
    chunk per single set bit 2^k in window 1."""
    e = [(0, 8 * 0 + 1, 1), (0, 8 * 127 + 3, 2), (0, 8 * 128, 1), (0, 8 * 255 + 7, 1)]
    e += [(1, 8 * (1 << k) + k, 1 + k % 2) for k in range(8)]
    return _shape("c12_edges", 12, e, _c12_edges.__doc__)


def _c13_groups():
    """c = 13 (B = 4096, 512 chunks, four groups): window 0 has one live chunk per group, window 1 leaves
    group 2 without an entry, window 15 (12 bits in the 13-bit table) only its lower half's last chunk."""
    e = [(0, 8 * (128 * g + 17 * g + 1) + g, 1) for g in range(4)]
    e += [(1, 8 * 5, 1), (1, 8 * 200 + 2, 2), (1, 8 * 511 + 7, 1)]
    e += [(15, 2047, 1)]
    return _shape("c13_groups", 13, e, _c13_groups.__doc__)


def _c17_groups():
    """c = 17 (B = 65,536, L = 16, 4,096 chunks, 32 groups): chunks 0 and 4,095 of window 0, and one chunk in
    each of groups 1, 2, 4, 8, 16 and 31 of window 1."""
    e = [(0, 5, 2), (0, 16 * 4095 + 15, 1)]
    e += [(1, 16 * (128 * g + g) + g % 16, 1 + g % 2) for g in (1, 2, 4, 8, 16, 31)]
    return _shape("c17_groups", 17, e, _c17_groups.__doc__, slow=True)


def _c19_direct():
    """c = 19 (B = 2^18, L = 16, 16,384 chunks, 128 groups: k_bucket_reduce_2 by size): chunk 0, every chunk
    2^k, and the last chunk (every bit set)."""
    e = [(0, 2, 1)] + [(0, 16 * (1 << k) + k, 1) for k in range(14)] + [(0, 16 * 16383 + 15, 1), (1, 16 * 9000 + 4, 2)]
    return _shape("c19_direct", 19, e, _c19_direct.__doc__, slow=True)


def _crossing():
    """The accumulation catalogue's wholewg_k1 (c = 8, K = 1): buckets that leave their accumulation
    workgroup, first and last in chunks whose other buckets are live too (the lead_val add)."""
    a = C.shape("wholewg_k1")
    s = C.Shape.__new__(C.Shape)
    s.__dict__.update(a.__dict__)
    s.name, s.doc, s.L, s.env, s.slow, s._inputs = "crossing", _crossing.__doc__, None, {}, False, None
    return s


# ---- shapes that need MSM_RED_L ----
def _c13_L12():
    """c = 13 with L = 12: 342 chunks, three groups (the V slices hold two and one), a partial last group, and
    four buckets in the last chunk; window 15's last live chunk holds bucket 2,047 alone of its lower half."""
    e = [(0, 4092, 1), (0, 4095, 1), (0, 12 * 130 + 11, 2), (0, 12 * 7, 1), (0, 12 * 300 + 5, 1)]
    e += [(1, 0, 1), (1, 1, 2), (1, 2, 1), (1, 12 * 256, 1), (15, 2047, 1), (15, 2040, 1)]
    return _shape("c13_L12", 13, e, _c13_L12.__doc__, L=12, env={"MSM_RED_L": "12"})


def _c14_L10():
    """c = 14 with L = 10: 820 chunks, seven groups (the bit terms enumerate four groups each and skip the
    eighth), a last chunk of two buckets, a last group of 52 chunks."""
    e = [(0, 10 * (128 * g + 11 * g) + g, 1 + g % 2) for g in (0, 3, 5, 6)] + [(0, 8191, 1), (0, 8190, 1)]
    e += [(1, 10 * 128 * 4 + 9, 1), (1, 10 * 128 * 5, 2), (8, 4095, 1)]
    return _shape("c14_L10", 14, e, _c14_L10.__doc__, L=10, env={"MSM_RED_L": "10"})


def _c17_L8():
    """c = 17 with L = 8: 8,192 chunks, exactly 64 groups (k_red2_terms on 256 threads)."""
    e = [(0, 1, 1), (0, 8 * 8191 + 7, 1)] + [(1, 8 * (128 * g + g) + g % 8, 1) for g in (1, 2, 4, 8, 16, 32, 63)]
    return _shape("c17_L8", 17, e, _c17_L8.__doc__, L=8, env={"MSM_RED_L": "8"}, slow=True)


def _c17_L4():
    """c = 17 with L = 4: 16,384 chunks, 128 groups: k_bucket_reduce_2 by size."""
    e = [(0, 2, 1), (0, 4 * 16383 + 3, 1)] + [(1, 4 * (1 << k) + k % 4, 1) for k in range(14)]
    return _shape("c17_L4", 17, e, _c17_L4.__doc__, L=4, env={"MSM_RED_L": "4"}, slow=True)


def _c8_short(L):
    last = 128 - (-(-128 // L) - 1) * L
    doc = ("c = 8 with L = %d: %s; window 1's first buckets are live, so a last chunk read at full length is seen."
           % (L, "the last chunk is short (%d buckets), and the last live chunk of the 7-bit windows straddles "
                 "bucket 64" % last if last < L else "32 chunks of the shortest chain"))
    e = [(0, 127, 1), (0, 126, 2), (0, 0, 1), (0, L, 1), (0, 2 * L - 1, 1)]
    e += [(1, i, 1 + i % 2) for i in range(7)] + [(31, 63, 1), (31, 60, 2), (30, min(63, 64 - 64 % L), 1)]
    return _shape("c8_short_L%d" % L, 8, e, doc, L=L, env={"MSM_RED_L": str(L)})


_BUILDERS = [_c8_bucket0, _c8_bucket_top, _c8_sweep, _c8_empty_mid, _c8_top7bit, _c8_overflow, _c4_one_chunk,
             _c12_edges, _c13_groups, _crossing, _c17_groups, _c19_direct, _c13_L12, _c14_L10, _c17_L8, _c17_L4]
_BUILDERS += [(lambda L=L: _c8_short(L)) for L in (4, 9, 10, 12, 17, 20)]
_cache = {}


def shapes():
    if not _cache:
        for f in _BUILDERS:
            s = f()
            _cache[s.name] = s
    return list(_cache.values())


def shape(name):
    shapes()
    return _cache[name]


def plain():
    """The shapes that need no knob."""
    return [s for s in shapes() if not s.env]


def small():
    """The knob-free shapes with small tables: what every knob child runs besides its own."""
    return [s for s in plain() if not s.slow]


def for_env(env):
    """The knob-only shapes of one setting."""
    return [s for s in shapes() if s.env and s.env == {k: v for k, v in env.items() if k in s.env}]


def chunk_len(s):
    """The shape's chunk length: its own, or the plan's (needs the library; no GPU)."""
    return s.L or C.chunk_len(s)


def plan(s, tree_knob=True, L=None):
    return RM.Plan(s.widths, s.B, L or chunk_len(s), s.cw, tree_knob=tree_knob)


def model_inputs(s, L=None):
    """{sizes, weight, lead} for _red_model.execute: per non-empty bucket its entry count and the signed
    sum of its entries' multipliers; lead: for a crossing bucket, the part that lies past its accumulation
    workgroup's end (in the model's entry order; the device's order within a bucket may differ)."""
    inp = C.inputs(s)
    uk, first = np.unique(inp["key"], return_index=True)
    tot = np.add.reduceat(inp["weight"], first)
    sizes = {int(k): int(s.sizes[k]) for k in uk}
    weight = {int(k): int(v) for k, v in zip(uk, tot)}
    lead = {}
    if s.K == 1:
        lay = s.layout(L or chunk_len(s))
        for k in A.execute(lay).crossing:
            a, b = int(lay.bucket_start[k]), int(lay.bucket_start[k + 1])
            cut = ((a // lay.K) // A.ACC_THREADS + 1) * A.ACC_THREADS * lay.K
            lead[int(k)] = int(inp["weight"][cut:b].sum())
    return {"sizes": sizes, "weight": weight, "lead": lead}


def expected_scalar(s):
    """sum_i s_i k_i mod r of the shape's inputs."""
    inp = C.inputs(s)
    return sum(sc * (C.K0 + i * C.STEP) for i, sc in enumerate(inp["ints"])) % RM.R
