"""Model of the bucket reduction (webgpu-msm_amd/csrc/msm_kernels.hip: red1_chunk / k_bucket_reduce_1,
red2_tree_steps / k_red2_groups, red2_term / k_red2_terms, k_bucket_reduce_2; csrc/host_tail.h:
collect_terms / horner_run), on integers mod r.

Every bucket carries an integer weight in the place of its point (the signed sum of its entries'
multipliers).  From the bucket sizes and weights the model derives every intermediate the device
holds -- U_c and T_c per chunk, V_g, S_g and R_{g,k} per group, the window terms in both second-stage
forms, the tail's (position, term) list and the total -- and names the branch classes the input
reaches (EVENTS).  One Python condition stands for one device condition; FLIPS lists the ones a test
may turn into their nearest wrong form.  The model says which branch an input takes and which
integer a point must be a multiple of G by; the reference for a point is O.scalar_mul(O.G, weight).
"""
R = 2111115437357092606062206234695386632838870926408408195193685246394721360383  # the group order r
RG_LOG = 7
RG_CH = 1 << RG_LOG
RG_OUT = 2 + RG_LOG
RG_MAXG = 64
RED1_LS = (4, 8, 9, 10, 12, 16, 17, 20)

FLIPS = {
    "weight_i": "red1_chunk: the running sums weigh bucket i by i + 1  ->  by i",
    "short_full": "red1_chunk: nb = min(RL, B - c RL)  ->  RL (a short last chunk read at full length)",
    "cross_dropped": "red1_chunk: b = pt_add(b, lead_val[g0 + 1]) for a crossing bucket  ->  b",
    "dead_skipped": "red1_lane: the dead chunks after the live ones  ->  no lane for them",
    "tree_r_index": "red2_group_point: R_k from shA[2^k]  ->  shA[2^k + 1]",
    "tree_partial": "red2_group_tree: identity for c >= nchunks  ->  chunk c - 1's sums again",
    "vslice_bound": "red2_term: g1 = min(ngroups, g0 + sl)  ->  g0 + sl - 1",
    "vslice_bound2": "k_bucket_reduce_2: c = term vslice + j, j < vslice  ->  j < vslice - 1",
    "s_for_v": "red2_term: a V slice reads group point 0 (V_g)  ->  point 1 (S_g)",
    "kbit_spread": "red2_term_group: (j >> kbit) << (kbit + 1)  ->  << kbit",
    "kbit_spread2": "k_bucket_reduce_2: (j >> kbit) << (kbit + 1)  ->  << kbit",
    "bit_past_end": "k_red2_terms: g < ngroups  ->  group g - ngroups read again",
    "npts_half": "red2_term: npts = pow2ceil(ngroups) / 2  ->  pow2floor(ngroups) / 2",
    "l_lowest_bit": "collect_terms: R_k once per set bit of L  ->  for L's lowest set bit only",
    "off_from_c": "collect_terms: off = win_off(d, w)  ->  w c",
    "empty_stale": "k_red2_terms: an empty window's terms are identities  ->  read red_G (stale)",
}

EVENTS = (
    "chunk:empty", "chunk:one_at_0", "chunk:one_at_top", "chunk:gaps", "chunk:full", "chunk:short_last",
    "chunk:cross", "chunk:dead_entry", "chunk:last_live_straddles_half",
    "window:empty", "window:empty_after_populated",
    "group:partial_last", "group:no_entry",
    "ngroups:1", "ngroups:2", "ngroups:odd", "ngroups:64",
    "term:vslice_no_group", "term:vslice_uneven", "term:bit_group_past_end", "term:cbits<RG_LOG",
    "nchunks:1", "L:two_bits",
    "path:groups+terms", "path:reduce_2",
)
UNREACHABLE = {
    "a live bucket at index 31 of the live mask":
        "the longest chunk is 20 buckets, so 1u << i never reaches the sign bit",
    "ngroups > RG_MAXG in k_red2_terms":
        "red2_tree sends such a plan to k_bucket_reduce_2; the 128 quads of k_red2_terms' largest block are "
        "never asked for more than 64 group points",
    "an entry above bucket 3 of the overflow window":
        "its digit is at most 4 (bits 254, 255 and a carry); dead chunks past chunk 0 of that window stay empty",
    "nv = 1 with nchunks >= 2":
        "finish_plan takes two V slices whenever there are two chunks",
    "a V slice with no chunk in k_bucket_reduce_2":
        "nv = 2 needs nchunks >= 2, and then both slices of ceil(nchunks / 2) chunks hold one",
}


def pow2ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


class Plan:
    """The reduction's view of a launch: window widths (overflow window last), the table's B, the chunk
    length L, and whether the tree form of the second stage is allowed (MSM_RED2_TREE)."""

    def __init__(self, widths, B, L, c, tree_knob=True):
        self.widths, self.B, self.L, self.c = list(widths), B, L, c
        self.W = len(widths)
        self.nchunks = -(-B // L)
        self.ngroups = -(-self.nchunks // RG_CH)
        self.nv = 2 if self.nchunks >= 2 else 1
        self.cbits = 0
        while (1 << self.cbits) < self.nchunks:
            self.cbits += 1
        self.nterms = self.nv + self.cbits
        self.tree = tree_knob and self.ngroups <= RG_MAXG
        self.path = "groups+terms" if self.tree else "reduce_2"
        self.off = [sum(self.widths[:w]) for w in range(self.W)]
        nfull = sum(1 for x in self.widths[:-1] if (1 << (x - 1)) == B)
        self.nhi = 0 if nfull == self.W - 1 else nfull

    def live_chunks(self, w):
        """red1_live_chunks: the chunks of window w a canonical scalar's digit can reach."""
        if w + 1 == self.W:
            return 0
        if self.nhi == 0 or w < self.nhi:
            return self.nchunks
        return (self.B // 2 + self.L - 1) // self.L


class Result:
    pass


def spread(j, kbit, wrong=False):
    return ((j >> kbit) << (kbit if wrong else kbit + 1)) | (1 << kbit) | (j & ((1 << kbit) - 1))


def tree_steps(A, Bv):
    """red2_tree_steps on integers: T in A, U in Bv (RG_CH each); in place."""
    for s in range(RG_LOG):
        lp = RG_LOG - 1 - s
        for Q in range((2 + s) << lp):
            kind, i = Q >> lp, Q & ((1 << lp) - 1)
            arr = Bv if kind == 1 else A
            if kind < 2:
                dst = i << (s + 1)
                src = dst + (1 << s)
            else:
                j = kind - 2
                l = s - j - 1
                md = i << (l + 1)
                ms = md + (1 << l)
                dst, src = (2 * md + 1) << j, (2 * ms + 1) << j
            arr[dst] = (arr[dst] + arr[src]) % R


def execute(plan, sizes, weight, lead=None, flips=(), prev_nonempty=()):
    """sizes: {flat key: entries} of the non-empty buckets (key = w B + b); weight: {key: the bucket's
    total weight}; lead: {key: the part of a crossing bucket that sits in lead_val}.  prev_nonempty: the
    windows the previous launch on the slot populated (for the stale-read event and flip)."""
    flips = set(flips)
    assert flips <= set(FLIPS), flips - set(FLIPS)
    lead = lead or {}
    B, L, W = plan.B, plan.L, plan.W
    ev = set()
    res = Result()
    res.U, res.T, res.G, res.terms_tree, res.terms_direct = {}, {}, {}, {}, {}
    res.empty = set()
    if plan.nchunks <= 1:
        ev.add("nchunks:1")
    if bin(L).count("1") == 2:
        ev.add("L:two_bits")
    ev.add("path:" + plan.path)
    ng = plan.ngroups
    ev.update(e for e, on in (("ngroups:1", ng == 1), ("ngroups:2", ng == 2), ("ngroups:odd", ng > 1 and ng % 2),
                              ("ngroups:64", ng == 64)) if on and plan.tree)
    if plan.cbits < RG_LOG and plan.tree:
        ev.add("term:cbits<RG_LOG")
    by_window = {}
    for k in sizes:
        assert sizes[k] > 0
        by_window.setdefault(k // B, []).append(k)

    # ---- first stage: U_c, T_c of every chunk that holds a live bucket (the others are 0) ----
    def value(k):
        v = weight[k]
        if k in lead:
            ev.add("chunk:cross")
            v = (weight[k] - lead[k]) + (0 if "cross_dropped" in flips else lead[k])
        return v

    for w in range(W):
        keys = by_window.get(w, [])
        if not keys:
            res.empty.add(w)
            ev.add("window:empty")
            if w in prev_nonempty:
                ev.add("window:empty_after_populated")
            continue
        chunks = {(k - w * B) // L for k in keys}
        if "short_full" in flips and B % L:  # the short last chunk then reads window w + 1's first buckets
            chunks.add(plan.nchunks - 1)
        chunks = sorted(chunks)
        for c in chunks:
            key0 = w * B + c * L
            nb = min(L, B - c * L)
            if "short_full" in flips:
                nb = L
            live = [i for i in range(nb) if key0 + i in sizes]
            if not live:
                continue
            if c >= plan.live_chunks(w):
                ev.add("chunk:dead_entry")
                if "dead_skipped" in flips:
                    continue
            if nb < L:
                ev.add("chunk:short_last")
            if len(live) == 1:
                if live[0] == 0:
                    ev.add("chunk:one_at_0")
                if live[0] == L - 1:
                    ev.add("chunk:one_at_top")
            elif len(live) == L:
                ev.add("chunk:full")
            if any(b - a > 1 for a, b in zip(live, live[1:])):
                ev.add("chunk:gaps")
            lc = plan.live_chunks(w)
            if 0 < lc < plan.nchunks and c == lc - 1 and (B // 2) % L:
                ev.add("chunk:last_live_straddles_half")
            wi = 0 if "weight_i" in flips else 1
            res.U[(w, c)] = sum((i + wi) * value(key0 + i) for i in live) % R
            res.T[(w, c)] = sum(value(key0 + i) for i in live) % R
        if len(chunks) < plan.nchunks:  # a chunk with no entry in a window that has some: the `!live` exit
            ev.add("chunk:empty")

    # ---- second stage, tree form: group points, then terms ----
    def group_points(w, g):
        A = [0] * RG_CH
        Bv = [0] * RG_CH
        for q in range(RG_CH):
            c = g * RG_CH + q
            if c >= plan.nchunks:
                ev.add("group:partial_last")
                if "tree_partial" in flips:
                    c = c - 1
                else:
                    continue
            A[q] = res.T.get((w, c), 0)
            Bv[q] = res.U.get((w, c), 0)
        plain = [sum(Bv) % R, sum(A) % R] + [sum(A[q] for q in range(RG_CH) if (q >> k) & 1) % R for k in range(RG_LOG)]
        tree_steps(A, Bv)
        off = 1 if "tree_r_index" in flips else 0
        pts = [Bv[0], A[0]] + [A[(1 << k) + off] for k in range(RG_LOG)]
        if not ({"tree_r_index", "tree_partial"} & flips):
            assert pts == plain, (w, g)
        return pts

    for w in range(W):
        if w in res.empty:
            for t in range(plan.nterms):
                res.terms_tree[(w, t)] = res.terms_direct[(w, t)] = 0
            if "empty_stale" in flips and w in prev_nonempty:
                res.terms_tree[(w, 0)] = res.terms_direct[(w, 0)] = 1  # whatever the table held: not the identity
            continue
        live_groups = {c // RG_CH for (ww, c) in res.U if ww == w}
        zero = [0] * RG_OUT
        if plan.tree:
            for g in range(ng):
                if g in live_groups or (g * RG_CH + RG_CH > plan.nchunks and "tree_partial" in flips):
                    res.G[(w, g)] = group_points(w, g)
                else:
                    if g * RG_CH + RG_CH > plan.nchunks:
                        ev.add("group:partial_last")
                    ev.add("group:no_entry")
                    res.G[(w, g)] = zero
            for t in range(plan.nterms):
                if t < plan.nv:
                    sl = -(-ng // plan.nv)
                    g0 = min(ng, t * sl)
                    g1 = min(ng, g0 + sl - (1 if "vslice_bound" in flips else 0))
                    if g1 <= g0:
                        ev.add("term:vslice_no_group")
                    elif plan.nv == 2 and ng > 1 and ng % 2:
                        ev.add("term:vslice_uneven")
                    idx = 1 if "s_for_v" in flips else 0
                    v = sum(res.G[(w, g)][idx] for g in range(g0, g1))
                elif t - plan.nv < RG_LOG:
                    v = sum(res.G[(w, g)][2 + t - plan.nv] for g in range(ng))
                else:
                    kbit = t - plan.nv - RG_LOG
                    npts = pow2ceil(ng) // 2 if ng > 1 else 1
                    if "npts_half" in flips:
                        npts = max(1, (1 << (ng.bit_length() - 1)) // 2)
                    v = 0
                    for j in range(npts):
                        g = spread(j, kbit, "kbit_spread" in flips)
                        if g >= ng:
                            ev.add("term:bit_group_past_end")
                            if "bit_past_end" not in flips or g - ng >= ng:
                                continue
                            g -= ng
                        v += res.G[(w, g)][1]
                res.terms_tree[(w, t)] = v % R
        # the direct form (k_bucket_reduce_2), whatever path the plan takes
        vslice = -(-plan.nchunks // plan.nv)
        half_n = pow2ceil(plan.nchunks) // 2 if plan.nchunks > 1 else 1
        mine = {c: (res.U[(w, c)], res.T[(w, c)]) for (ww, c) in res.U if ww == w}
        for t in range(plan.nterms):
            if t < plan.nv:
                hi = vslice - (1 if "vslice_bound2" in flips else 0)
                v = sum(u for c, (u, _) in mine.items() if t * vslice <= c < t * vslice + hi and c < plan.nchunks)
            else:
                kbit = t - plan.nv
                v = 0
                if "kbit_spread2" in flips:
                    for j in range(half_n):
                        c = spread(j, kbit, True)
                        if c < plan.nchunks and c in mine:
                            v += mine[c][1]
                else:
                    v = sum(tt for c, (_, tt) in mine.items() if (c >> kbit) & 1)
            res.terms_direct[(w, t)] = v % R
    res.terms = res.terms_tree if plan.tree else res.terms_direct

    # ---- the host tail ----
    def tail(terms):
        at = []
        for w in range(W):
            off = w * plan.c if "off_from_c" in flips else plan.off[w]
            for t in range(plan.nterms):
                v = terms[(w, t)]
                if v == 0:
                    continue  # identity terms are skipped
                if t < plan.nv:
                    at.append((off, (w, t)))
                else:
                    bits = [b for b in range(L.bit_length()) if (L >> b) & 1]
                    if "l_lowest_bit" in flips:
                        bits = bits[:1]
                    at.extend((off + (t - plan.nv) + b, (w, t)) for b in bits)
        return at

    res.tail = tail(res.terms)
    res.total = sum(terms_v << pos for pos, terms_v in ((p, res.terms[k]) for p, k in res.tail)) % R
    res.total_direct = sum(res.terms_direct[k] << p for p, k in tail(res.terms_direct)) % R
    res.total_tree = sum(res.terms_tree[k] << p for p, k in tail(res.terms_tree)) % R if plan.tree else None
    res.events = ev
    return res


def plain_total(plan, weight):
    """sum_w 2^off_w sum_b (b + 1) B_{w,b}."""
    return sum(((k % plan.B) + 1) * v << plan.off[k // plan.B] for k, v in weight.items()) % R
