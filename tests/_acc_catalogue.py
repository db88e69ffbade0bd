"""A catalogue of bucket layouts for the run accumulation's joins (tests/_acc_model.py), and the MSM
inputs that produce each of them on the device.

A shape is a short recipe: a window width c, a run length K and bucket sizes by key, written with
Rec below as a walk along the sorted list ("a bucket of 6 entries from lane 253 of workgroup 1").
Every shape is the smallest that reaches its events; tests/test_acc_model.py checks that the union of
the shapes' events is the model's whole list, and that every condition the model can flip is caught
by some shape.  When a join changes, add its shape here.

inputs(shape) turns a recipe into points and scalars: P_i = (k0 + i step) G, and one 8-word scalar
per point whose signed digits over the balanced windows (Wm = ceil(254 / c) main windows, the lowest
254 mod Wm one bit wider, then the 3-bit overflow window) are exactly the recipe's entries: window w's
entries go to points 0, 1, 2, ... in key order, the scalar is sum_w digit_w 2^off(w), and the recode is
unique, so the device's digits are the wanted ones (checked against _narrow_model.recode).  A point's
top digit is positive, so that the scalar is; below it both signs occur, one sign per bucket, so that
no stretch of a bucket's entries sums to zero in any order.  Zero digits make no entry.
"""
import numpy as np

import _acc_model as A
from _narrow_model import recode

K0, STEP = 1000003, 977  # P_i = (K0 + i STEP) G


def geometry(c):
    """(widths of every window, overflow window included; B; the table's width)."""
    wm = -(-254 // c)
    q, nhi = divmod(254, wm)
    widths = [q + 1 if w < nhi else q for w in range(wm)] + [3]
    cw = q + 1 if nhi else q
    return widths, 1 << (cw - 1), cw


class Rec:
    """A recipe under construction: buckets appended in key order."""

    def __init__(self, c, K):
        self.c, self.K = c, K
        self.widths, self.B, _ = geometry(c)
        self.nkeys = len(self.widths) * self.B
        self.sizes = []
        self.pos = 0

    def reachable(self, key):
        w, b = divmod(key, self.B)
        return b < 3 if w == len(self.widths) - 1 else b < 1 << (self.widths[w] - 1)

    def b(self, *sizes):
        """Buckets of these sizes at the next keys a digit can reach."""
        for sz in sizes:
            while not self.reachable(len(self.sizes)):
                assert self.K == 1 or self.pos % self.K == 0, "an implicit gap inside a run"
                self.sizes.append(0)
            self.sizes.append(sz)
            self.pos += sz
        return self

    def skip(self, n=1):
        self.sizes.extend([0] * n)
        return self

    def to_key(self, key):
        assert key >= len(self.sizes)
        return self.skip(key - len(self.sizes))

    def lane(self, wg, lt):
        """The position where run `lt` of workgroup `wg` starts."""
        return (wg * A.ACC_THREADS + lt) * self.K

    def fill(self, target, size):
        """Buckets of `size` entries up to position `target` (the last one shorter)."""
        assert target >= self.pos, (target, self.pos)
        while self.pos + size <= target:
            self.b(size)
        if self.pos < target:
            self.b(target - self.pos)
        return self

    def until(self, target):
        """One bucket from here to position `target`."""
        assert target > self.pos
        return self.b(target - self.pos)

    def done(self):
        assert len(self.sizes) <= self.nkeys, (len(self.sizes), self.nkeys)
        return np.array(self.sizes + [0] * (self.nkeys - len(self.sizes)), dtype=np.int64)


class Shape:
    def __init__(self, name, rec, doc, large=False):
        self.name, self.c, self.K, self.doc, self.large = name, rec.c, rec.K, doc, large
        self.widths, self.B, self.cw = rec.widths, rec.B, geometry(rec.c)[2]
        self.sizes = rec.done()
        self.nkeys = rec.nkeys
        self._inputs = None

    def layout(self, L=8):
        return A.Layout(self.sizes, self.K, B=self.B, L=L)

    @property
    def n(self):
        per_window = self.sizes.reshape(-1, self.B).sum(axis=1)
        return int(per_window.max())


def inputs(shape):
    """{n, scalars [n, 8] BE words, key / word / weight of every entry in the model's sorted order
    (by key, then by point)}; word = (point << 1) | sign, weight = +-(K0 + point STEP)."""
    if shape._inputs is not None:
        return shape._inputs
    B, widths = shape.B, shape.widths
    per = shape.sizes.reshape(-1, B)
    cnt = per.sum(axis=1)
    n = int(cnt.max())
    above = np.zeros(len(widths) + 1, dtype=np.int64)  # above[w]: points with an entry in a window past w
    for w in range(len(widths) - 1, -1, -1):
        above[w] = max(above[w + 1], cnt[w])
    scal = [0] * n
    keys, words, weights = [], [], []
    off = 0
    for w, width in enumerate(widths):
        m = int(cnt[w])
        if m:
            pt = np.arange(m, dtype=np.int64)
            bucket = np.repeat(np.arange(B, dtype=np.int64), per[w])
            mag = bucket + 1
            assert int(mag.max()) <= 1 << (width - 1), (shape.name, w)
            # one sign per bucket (two buckets in three negative where that can be): a head, a tail, a chain
            # or a lead is a stretch of ONE bucket's entries in whatever order the device's sort leaves
            # them, so with one sign it is a sum of positive multipliers below r, never zero.  A negative
            # digit needs a positive one above it in the same scalar and a magnitude below 2^(width - 1).
            last_pt = np.cumsum(per[w]) - 1  # the last point of every bucket of the window
            can = (last_pt < above[w + 1]) & (np.arange(B) + 1 < (1 << (width - 1))) & ((w * B + np.arange(B)) % 3 != 0)
            neg = can[bucket]
            digit = np.where(neg, -mag, mag)
            for i, d in zip(pt.tolist(), digit.tolist()):
                scal[i] += d << off
            keys.append(w * B + bucket)
            words.append((pt << 1) | neg)
            weights.append(np.where(neg, -1, 1) * (K0 + pt * STEP))
        off += width
    assert all(0 < s < 1 << 256 for s in scal), shape.name
    raw = b"".join(s.to_bytes(32, "big") for s in scal)
    sc = np.frombuffer(raw, dtype=">u4").astype(np.uint32).reshape(n, 8)
    shape._inputs = {"n": n, "scalars": sc, "ints": scal, "key": np.concatenate(keys), "word": np.concatenate(words),
                     "weight": np.concatenate(weights)}
    return shape._inputs


def check_recode(shape, sample=None):
    """The scalars' digits under _narrow_model.recode are the recipe's entries (all points, or a sample)."""
    inp = inputs(shape)
    B = shape.B
    got = np.zeros(shape.nkeys, dtype=np.int64)
    idx = range(inp["n"]) if sample is None else sample
    for i in idx:
        digits, carry = recode(inp["ints"][i], shape.widths)
        assert carry == 0
        for w, d in enumerate(digits):
            if d:
                got[w * B + abs(d) - 1] += 1
    return got


# ---- the shapes ---------------------------------------------------------------------------------------
def _kinds_k3():
    """Every run kind at K = 3 (scalar entry loads), M no multiple of K, one workgroup (last in between)."""
    r = Rec(4, 3)
    r.b(2, 1)        # run 0 [0, 3): two whole buckets with no empty key between them (gap 0)
    r.b(3)           # run 1 [3, 6): a bucket that starts on the run's first entry and ends on its last
    r.b(4)           # run 2 [6, 9): a tail of 3 (nwalk 1) ...
    r.b(1, 3)        # run 3: ... its head of 1, a whole bucket, a tail of 1: head and tail; run 4: head of 2 ...
    r.b(8)           # ... and a tail of 1 (nwalk 3); runs 5, 6: pass heads; run 7 [21, 24): the head of 1 ...
    r.b(2)           # ... and a bucket that ends on the run's last entry
    r.b(5)           # run 8 [24, 27): a tail from the run's first entry; run 9: head of 2 ...
    r.b(2)           # ... and a tail of 1; run 10 is short (M = 31): a head that ends on the list's last entry
    return Shape("kinds_k3", r, _kinds_k3.__doc__)


def _gaps_k4():
    """Empty keys walked inside a run at K = 4 (vector entry loads): gaps of 0, 1, 2, 3, 4, 6, 12 keys, a gap
    over two whole empty windows, and next_nonempty's clamp at nkeys - 1 in front of the overflow window;
    M a multiple of K, 257 runs: the second workgroup has one live run (last == 0)."""
    r = Rec(4, 4)
    r.b(1, 1)
    r.skip(1).b(1).skip(2).b(1)            # run 0: gap 0, gap 1 (first probe), gap 2 (one doubling)
    r.b(1).skip(3).b(1).skip(4).b(1).b(1)  # run 1: gaps of 3 and 4 (several doublings, binary search)
    r.b(1).skip(6).b(1).skip(12).b(2)      # run 2: gaps of 6 and 12
    r.b(1).skip(2 * r.B + 5).b(3)          # run 3: a gap over two whole empty windows
    r.fill(r.lane(1, 0) - 2, 4)            # whole buckets of one run each
    last_key = (len(r.widths) - 1) * r.B + 2
    r.b(3)                                 # run 255 ends with the first entry of this bucket ...
    assert r.pos == r.lane(1, 0) + 1
    r.to_key(last_key - 10).b(1)           # ... and run 256 walks a gap, then the clamp in front of ...
    r.to_key(last_key).b(2)                # ... the overflow window's digit 3
    return Shape("gaps_k4", r, _gaps_k4.__doc__)


def _last1_k4():
    """258 runs at K = 4: the second workgroup has two live runs (last == 1); a bucket crosses into its lane 0."""
    r = Rec(5, 4)
    r.fill(r.lane(0, 255) + 1, 4)
    r.b(6)                                 # tail of 3 at lane 255, head of 3 in lane 0 of workgroup 1
    r.until(r.lane(1, 2) - 1)
    return Shape("last1_k4", r, _last1_k4.__doc__)


def _unskewed_k1():
    """The straight-line joins at K = 1, no workgroup skewed: tails with nwalk 1, 2, 3 that close inside
    the workgroup; across 0 | 1 a tail at lane 254 whose chain leaves through lane 255 (nwalk 1, plain lead);
    across 1 | 2 the straddle (tail at 253, passes at 254, 255, 0, 1, closing at lane 2: nwalk 2 cut at
    `last`, lead joined over two); across 2 | 3 a tail at lane 255 itself (nwalk 0) and a lead joined over
    one pass head."""
    r = Rec(8, 1)
    r.b(2, 3, 4, 1, 2, 3, 4)               # nwalk 1, 2, 3 closing
    r.fill(r.lane(0, 254), 2)
    r.b(3)                                 # lanes 254 (tail), 255 (pass) | lane 0 closes
    r.fill(r.lane(1, 253), 3)
    assert r.pos == r.lane(1, 253)
    r.b(6)                                 # the straddle
    r.fill(r.lane(2, 255), 4)
    assert r.pos == r.lane(2, 255)
    r.b(3)                                 # lane 255 (tail) | lane 0 pass, lane 1 closes
    r.fill(r.lane(3, 100), 1)
    return Shape("unskewed_k1", r, _unskewed_k1.__doc__)


def _chains_k1():
    """One skewed workgroup at K = 1 with chains of 3, 4, 5, 7, 8, 9, 16 and 17 pass heads (buckets of two
    entries more), and ordinary one-head joins (buckets of 2) between them."""
    r = Rec(4, 1)
    for npass in (3, 4, 5, 7, 8, 9, 16, 17):
        r.b(2, npass + 2, 1)
    return Shape("chains_k1", r, _chains_k1.__doc__)


def _edges_k1():
    """Skew at the workgroup's edges, K = 1.  Workgroup 0: passes at lanes 253-255 (tail at 252), the chain
    leaves through lane 255; workgroup 1: it goes on over lanes 0-2 and closes at lane 3 (three passes at
    lanes 0-2), then a tail owner at lane 255 whose bucket closes at lane 1 of workgroup 2; workgroup 2 is
    not skewed (lead joined over one pass), workgroup 3 is skewed again by a chain in its middle."""
    r = Rec(8, 1)
    r.fill(r.lane(0, 252), 2)
    r.until(r.lane(1, 4))                  # tail at 252, passes 253..255 | passes 0..2, closes at 3
    r.fill(r.lane(1, 255), 3)
    assert r.pos == r.lane(1, 255)
    r.b(3)                                 # tail at lane 255 of a skewed workgroup | pass, close
    r.fill(r.lane(3, 40), 2)
    r.b(9)
    r.fill(r.lane(3, 77), 1)
    return Shape("edges_k1", r, _edges_k1.__doc__)


def _wholewg_k1():
    """Leads that stay open, K = 1.  A bucket from lane 0 of workgroup 1 (its start an exact multiple of
    K 256) with 255 pass heads at lanes 1-255, leaving through lane 255 and closing at lane 2 of workgroup 2
    (unskewed: lead joined over two).  A bucket from lane 200 of workgroup 3 through all 256 lanes of
    workgroup 4 (256 pass heads: the lead stays open through one workgroup) that closes at lane 1 of
    workgroup 5 (unskewed, joined lead).  A bucket from lane 250 of workgroup 6 through workgroups 7 and 8
    (open through two) that ends on lane 0 of workgroup 9 (unskewed, plain lead).  The crossing buckets sit
    first and last in their reduction chunks of 8."""
    r = Rec(8, 1)
    r.fill(r.lane(1, 0), 2)
    r.to_key((len(r.sizes) + 7) // 8 * 8)      # first of its chunk
    r.until(r.lane(2, 3))
    r.fill(r.lane(3, 200), 2)
    r.to_key((len(r.sizes) + 8) // 8 * 8 - 1)  # last of its chunk
    r.until(r.lane(5, 2))
    r.fill(r.lane(6, 250), 2)
    r.until(r.lane(9, 1))
    r.fill(r.lane(9, 30), 1)
    return Shape("wholewg_k1", r, _wholewg_k1.__doc__)


def _chain255_k1():
    """A lead chain of 255 pass heads that closes at lane 255, K = 1: a bucket from lane 250 of workgroup 0
    to lane 255 of workgroup 1; then two whole windows left empty, and a bucket over the boundary 1 | 2."""
    r = Rec(8, 1)
    r.fill(r.lane(0, 250), 1)
    r.until(r.lane(2, 0))
    r.skip(2 * r.B)
    r.fill(r.lane(2, 9), 3)
    return Shape("chain255_k1", r, _chain255_k1.__doc__)


def _wide_k3():
    """A second width (c = 18: a 17-bit table, a longer reduction chunk): crossing buckets at K = 3, one out
    of an unskewed workgroup and one out of a skewed one."""
    r = Rec(18, 3)
    r.fill(r.lane(0, 254) + 1, 3)
    r.b(7)                                 # tail at 254, pass at 255 | head in lane 0
    r.fill(r.lane(1, 250), 5)
    r.until(r.lane(2, 1) + 2)              # tail at 250, passes 251..255 | pass, head
    r.fill(r.lane(2, 20), 2)
    return Shape("wide_k3", r, _wide_k3.__doc__)


def _tile_closes():
    """2^17 + 2^10 entries at K = 1 (516 workgroups, more than CJ_GRID of them skewed): a bucket whose open
    lead chain ends on workgroup 511, the last lead of the first scan tile; then one open through
    workgroups 512 and 513."""
    r = Rec(16, 1)
    r.b(7)
    r.until(r.lane(511, 10))
    r.to_key(r.B)                          # (the second bucket's entries in the next window: fewer points)
    r.until(r.lane(514, 4))
    r.fill((1 << 17) + (1 << 10), 2)
    return Shape("tile_closes", r, _tile_closes.__doc__, large=True)


def _tile_crosses():
    """2^17 + 2^10 entries at K = 1: an open lead chain from workgroup 4 that crosses the scan-tile boundary
    511 | 512 and ends in workgroup 513."""
    r = Rec(16, 1)
    r.fill(r.lane(3, 5), 3)
    r.to_key(r.B)
    r.until(r.lane(513, 100))
    r.to_key(2 * r.B)
    r.fill((1 << 17) + (1 << 10), 2)
    return Shape("tile_crosses", r, _tile_crosses.__doc__, large=True)


def _tile_whole():
    """2^18 + 2^12 entries at K = 1 (1,040 workgroups): a bucket over workgroups 0-499, then one from
    workgroup 500 to 1,031: open across 511 | 512, through the whole second tile, and across 1,023 | 1,024."""
    r = Rec(16, 1)
    r.b(1, 2)
    r.until(r.lane(500, 17))
    r.to_key(r.B)
    r.until(r.lane(1031, 3))
    r.to_key(2 * r.B)
    r.fill((1 << 18) + (1 << 12), 2)
    return Shape("tile_whole", r, _tile_whole.__doc__, large=True)


SEQ_N = 512  # the points of every seq_* shape: one plan, so that the slot's captured graph is replayed


def _seq(name, doc, body):
    r = Rec(8, 1)
    body(r)
    r.fill(max(r.pos, r.lane(3, 7)), 2)     # (no multiple of 256 runs: in a shared launch the next member's
                                            # runs start inside this one's last workgroup)
    r.to_key((len(r.sizes) + r.B - 1) // r.B * r.B)
    r.fill(r.pos + SEQ_N, 4)               # a window of SEQ_N entries: the shape's n, whatever came before
    s = Shape(name, r, doc)
    assert s.n == SEQ_N, (name, s.n)
    return s


def _seq_a():
    """First of three shapes of one plan (c = 8, K = 1, 512 points) that run one after the other on one
    slot: workgroups 0 and 1 skewed by one bucket from lane 100 to lane 50 of the next."""
    return _seq("seq_a", _seq_a.__doc__, lambda r: r.fill(r.lane(0, 100), 2).until(r.lane(1, 51)))


def _seq_b():
    """Second of the three: no workgroup skewed (buckets of 3: tails with nwalk 2), more entries than seq_a."""
    return _seq("seq_b", _seq_b.__doc__, lambda r: r.fill(r.lane(3, 40), 3))


def _seq_c():
    """Third of the three: workgroup 2 alone skewed (a chain of 9 in its middle), and a bucket that leaves the
    unskewed workgroup 0 through lane 255."""
    return _seq("seq_c", _seq_c.__doc__,
                lambda r: r.fill(r.lane(0, 254), 2).b(4).fill(r.lane(2, 60), 1).b(11))


_BUILDERS = (_kinds_k3, _gaps_k4, _last1_k4, _unskewed_k1, _chains_k1, _edges_k1, _wholewg_k1, _chain255_k1, _wide_k3,
             _seq_a, _seq_b, _seq_c, _tile_closes, _tile_crosses, _tile_whole)
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


def chunk_len(s):
    """The reduction's chunk length L of the shape's launch, from the library's plan."""
    import msm_amd as M

    return M.launch_plan(s.n, window_size=s.c, run_length=s.K)["chunk_len"]
