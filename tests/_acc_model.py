"""Control-flow model of the run accumulation's bucket joins (webgpu-msm_amd/csrc/msm_kernels.hip:
acc_tile / k_accumulate, next_nonempty, k_chain_join, k_lead_scan and the cross_key / lead_val add
of red1_chunk), in plain Python.

From the bucket sizes by key, the run length K and the key count it derives what the device holds
(bucket_start, run_key, the workgroups and their `last`), says which branch every run, workgroup
and bucket takes, and names those branches as events.  One Python condition stands for one device
condition, by name.  The model restates control flow only: it is never the reference for a value.

It also executes the joins symbolically: every sorted entry carries an integer weight in the place
of its point, the model's own pieces -- heads, tails, walks, the chain scan, the lead scan, the
cross adds -- are summed mod r, and every bucket's total comes back.  The plain sum of a bucket's
weights checks that on the CPU (tests/test_acc_model.py); with a condition flipped (FLIPS) some
catalogue shape's totals must come out wrong, which shows that the catalogue (tests/_acc_catalogue.py)
reaches the condition.  Whatever the device would read without having written it this launch -- LDS
past a workgroup's heads, a stale lead_val, a bucket never stored -- reads as POISON here.
"""
import numpy as np

R = 2111115437357092606062206234695386632838870926408408195193685246394721360383  # the group order r
ACC_THREADS = 256   # runs per k_accumulate workgroup
CJ_GRID = 256       # k_chain_join workgroups
LS_THREADS = 512    # leads per k_lead_scan tile
KEY_INVALID = None
POISON = 0x5A17ED5A17ED5A17ED5A17ED5A17ED5A17ED5A17ED5A17ED % R

# Conditions of the device code that a test may flip, each to the nearest wrong form.  A flip that
# cannot change a bucket's total is not listed; BENIGN says why.
FLIPS = {
    "started_before": "acc_tile: bucket_start[cur] < s  ->  <=",
    "cont": "acc_tile: cont = bend > e  ->  >=",
    "flush_seg_first": "acc_tile: the flush's `seg_first && started_before`  ->  started_before",
    "gallop_probe": "next_nonempty: bucket_start[hi + 1] == pos  ->  bucket_start[hi] == pos",
    "nwalk_tail_last": "acc_tile nwalk: lt < last ? ... : 0  ->  lt <= last",
    "nwalk_clip1": "acc_tile nwalk: nxt_pass && lt + 1 < last  ->  nxt_pass",
    "nwalk_clip2": "acc_tile nwalk: nxt2_pass && lt + 2 < last  ->  nxt2_pass, with nxt2_pass's own lt + 1 <= last",
    "lead_join_one": "acc_tile nwalk of the lead: 1 + nxt_pass  ->  1",
    "lead_join_two": "acc_tile nwalk of the lead: 1 + nxt_pass  ->  2",
    "skew_three": "acc_tile skew trigger: three pass heads in a row  ->  four",
    "cj_take": "k_chain_join: take = open && lt + d < ACC_THREADS  ->  <=",
    "cj_steps": "k_chain_join: for (d = 1; d < ACC_THREADS; ...)  ->  d < ACC_THREADS / 2",
    "cj_close": "k_chain_join: open = nopen  ->  open stays",
    "cj_tail": "k_chain_join: the tail owner's lt + 1 < ACC_THREADS  ->  <=",
    "cj_lead_open": "k_chain_join: lead_open[wg] = lopen  ->  0",
    "cj_grid_loop": "k_chain_join: li += gridDim.x over the skewed list  ->  one pass of CJ_GRID",
    "ls_take": "k_lead_scan: take = ... i + d < LS_THREADS  ->  <=",
    "ls_absorb": "k_lead_scan: the absorb of the next tile's first lead  ->  none",
    "ls_absorb_index": "k_lead_scan: gn = (tile + 1) LS_THREADS  ->  + 1",
    "ls_tile_order": "k_lead_scan: tiles from the last to the first  ->  from the first to the last",
    "red_group": "red1_chunk: cross_key[bucket_start / (K 256)]  ->  cross_key[(bucket_start - 1) / (K 256)]",
    "red_lead": "red1_chunk: lead_val[g0 + 1]  ->  lead_val[g0]",
}
BENIGN = {
    "nxt_pass: lt < last": "past `last` the head keys are KEY_INVALID (sh_hkey is initialised by all 256 lanes) and "
                           "with last == 255 lane 255's nxt_pass feeds only the skew trigger: a workgroup skewed "
                           "without need still joins right",
    "nxt2_pass: lt + 1 < last": "repeated by nwalk's own lt + 1 < last; alone it feeds the skew trigger",
    "lead store: !lead_join": "the same lane overwrites lead_val[wg] with the joined lead",
    "k_lead_scan take: g + d < nwg": "past nwg a tile holds identities that are not open: adding one closes the "
                                     "chain, which in the last tile is closed anyway (the last run never continues)",
    "k_lead_scan absorb: gn < nwg": "a lead of the last workgroup is never open, so no lane of the last tile is open "
                                    "at its end",
    "k_lead_scan store: lead_open[g] != 0": "a lead that is not open keeps its value through the scan",
    "next_nonempty: min(cur + step, nkeys - 1)": "without the clamp the probe reads past the table; a value, not a "
                                                 "branch of the joins",
}

# Every branch class the catalogue must reach (test_acc_model.py: the union over the catalogue
# equals this list).  UNREACHABLE names the branches of the device code that no input can reach.
EVENTS = (
    # runs
    "run:K%4==0", "run:K%4!=0", "run:M%K==0", "run:M%K!=0",
    "run:whole", "run:head", "run:pass", "run:tail", "run:head+tail",
    "run:head_ends_on_last_entry", "run:bucket_starts_on_first_entry",
    # gaps of empty keys walked inside a run, and how next_nonempty resolves them
    "gap:0", "gap:1", "gap:2", "gap:3-4", "gap:5-8", "gap:>=9", "gap:whole_windows",
    "gallop:first_probe", "gallop:one_doubling", "gallop:several_doublings", "gallop:clamp",
    "gallop:binary_search",
    # joins of a workgroup that is not skewed
    "tail:nwalk1:closes", "tail:nwalk2:closes", "tail:nwalk3:closes",
    "tail:nwalk1:leaves", "tail:nwalk2:leaves", "tail:nwalk0:leaves",
    "lead:none", "lead:plain", "lead:join1", "lead:join2",
    "last:255", "last:1", "last:0", "last:mid",
    "join:straddle",
    # skew triggers
    "skew:three_mid", "skew:three_at_253", "skew:three_at_0",
    # k_chain_join
    "cj:chain3", "cj:chain4", "cj:chain5", "cj:chain7", "cj:chain8", "cj:chain9", "cj:chain16", "cj:chain17",
    "cj:chain255", "cj:chain256", "cj:leaves_255", "cj:tail_at_255", "cj:two_chains", "cj:one_head_join",
    "cj:more_than_grid",
    # k_lead_scan
    "ls:open1", "ls:open2", "ls:crosses_tile", "ls:closes_on_511", "ls:whole_tile",
    "ls:ends_plain_lead", "ls:ends_joined_lead",
    # neighbours
    "nb:skewed,unskewed", "nb:unskewed,skewed", "nb:skewed,unskewed,skewed",
    # reduction
    "red:cross_first_of_chunk", "red:cross_last_of_chunk", "red:cross_start_multiple_of_K256",
)
UNREACHABLE = {
    "skew trigger `lt == 0 && my_pass && last == 0`":
        "last == 0 means the workgroup's only live run is the last run of the list; its bucket ends at the "
        "total (bend <= e = M), so cont is false and the head cannot be pass",
    "skew trigger `lt == 0 && my_pass && nxt_pass && last == 1`":
        "lane 1 is then the list's last run and cannot be pass, for the same reason",
    "tail nwalk 3 cut short at lane last":
        "passes at lanes last - 2, last - 1 and last are three in a row: the workgroup is skewed",
    "the last key nkeys - 1 non-empty":
        "with 8-word scalars the last window is the 3-bit overflow window: its digit is at most 4, bucket 3 of "
        "B >= 8; the gallop's clamp at nkeys - 1 is still reached (gallop:clamp)",
    "the folded reduction k_bucket_reduce_1g and the lane-pair form 1p":
        "both are behind knobs that are off by default (MSM_RED_FOLD, MSM_RED1_PAIRS): no plan takes them",
}


class Layout:
    """Bucket sizes by key (key = w B + b), the run length K, and optionally the buckets per window B
    and the reduction's chunk length L (for the window and chunk events)."""

    def __init__(self, sizes, K, B=None, L=None):
        self.sizes = np.asarray(sizes, dtype=np.int64)
        self.nkeys = int(self.sizes.shape[0])
        self.K = int(K)
        self.B = B
        self.L = L
        bs = np.zeros(self.nkeys + 1, dtype=np.int64)
        np.cumsum(self.sizes, out=bs[1:])
        self.bucket_start = bs
        self.M = int(bs[-1])
        self.nruns = (self.M + self.K - 1) // self.K
        self.nwg = (self.nruns + ACC_THREADS - 1) // ACC_THREADS
        # run_key[t]: the key that owns position t K
        self.run_key = (np.searchsorted(bs, np.arange(self.nruns, dtype=np.int64) * self.K, side="right") - 1)

    def last(self, wg):
        return min(ACC_THREADS, self.nruns - min(self.nruns, wg * ACC_THREADS)) - 1


class Result:
    pass


def _next_nonempty(bs, cur, pos, nkeys, F, ev):
    """next_nonempty: bucket `cur` is empty; the first key above it whose end lies past pos."""
    lo, step, hi = cur, 1, cur + 1
    doublings = 0
    probe = (lambda h: bs[h] == pos) if "gallop_probe" in F else (lambda h: bs[h + 1] == pos)
    while probe(hi):
        lo = hi
        step <<= 1
        if cur + step > nkeys - 1:
            ev.add("gallop:clamp")
        hi = min(cur + step, nkeys - 1)
        doublings += 1
    ev.add("gallop:first_probe" if doublings == 0 else "gallop:one_doubling" if doublings == 1
           else "gallop:several_doublings")
    if hi - lo > 1:
        ev.add("gallop:binary_search")
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if bs[mid + 1] == pos:
            lo = mid
        else:
            hi = mid
    return hi


def execute(lay, weights=None, flips=(), pieces=None):
    """Walk the layout as the kernels would.  weights: one integer per sorted position (default 1).
    pieces: a function called with (what, value) for every intermediate sum, or None."""
    F = frozenset(flips)
    assert F <= set(FLIPS), F - set(FLIPS)
    K, M, nkeys, nruns, nwg = lay.K, lay.M, lay.nkeys, lay.nruns, lay.nwg
    bs = lay.bucket_start.tolist() + [M, M]  # (the device's table is padded: acc_tile prefetches cur + 2)
    run_key = lay.run_key.tolist()
    ev = set()
    res = Result()
    res.events = ev
    if weights is None:
        pre = list(range(M + 1))
    else:
        pre = [0] * (M + 1)
        acc = 0
        for i, w in enumerate(weights):
            acc += int(w)
            pre[i + 1] = acc

    def span(a, b):
        return (pre[b] - pre[a]) % R

    def note(what, v):
        if pieces is not None:
            pieces(what, v)
        return v

    ev.add("run:K%4==0" if K % 4 == 0 else "run:K%4!=0")
    if M:
        ev.add("run:M%K==0" if M % K == 0 else "run:M%K!=0")
    buckets = {}     # key -> value stored in the bucket table
    head = [None] * nruns   # (key, pass, value) of a run's leading piece
    tail = [None] * nruns   # (key, value) of a run's trailing piece
    cont_run = [False] * nruns
    cur_run = [0] * nruns
    kinds = [None] * nruns
    # ---- k_accumulate's main loop, run by run ---------------------------------------------------
    for t in range(nruns):
        s = t * K
        e = min(s + K, M)
        cur = run_key[t]
        started_before = bs[cur] <= s if "started_before" in F else bs[cur] < s
        if bs[cur] == s:
            ev.add("run:bucket_starts_on_first_entry")
        bend = bs[cur + 1]
        seg_first, seg_start = True, s
        while bend < e:  # pos == bend inside the loop: bucket `cur` ends here
            v = note("run part", span(seg_start, bend))
            if (seg_first or "flush_seg_first" in F) and started_before:
                head[t] = (cur, False, v)
            else:
                buckets[cur] = v
            pos = bend
            cur += 1
            bend = bs[cur + 1]
            if bend == pos:
                first_empty = cur
                cur = _next_nonempty(bs, cur, pos, nkeys, F, ev)
                gap = cur - first_empty
                ev.add("gap:1" if gap == 1 else "gap:2" if gap == 2 else "gap:3-4" if gap <= 4
                       else "gap:5-8" if gap <= 8 else "gap:>=9")
                if lay.B and (cur // lay.B) - ((first_empty + lay.B - 1) // lay.B) >= 1:
                    ev.add("gap:whole_windows")
                bend = bs[cur + 1]
            else:
                ev.add("gap:0")
            seg_start, seg_first = pos, False
        cont = bend >= e if "cont" in F else bend > e
        v = note("run part", span(seg_start, e))
        if seg_first and started_before:
            head[t] = (cur, cont, v)
            if not cont:
                ev.add("run:head_ends_on_last_entry")
        elif cont:
            tail[t] = (cur, v)
        else:
            buckets[cur] = v
        cont_run[t], cur_run[t] = cont, cur
        h, tl = head[t], tail[t]
        kinds[t] = ("pass" if h and h[1] else "head+tail" if h and tl else "head" if h else "tail" if tl else "whole")
        ev.add("run:" + kinds[t])
    res.run_kind = kinds
    # ---- the joins inside a workgroup ------------------------------------------------------------
    cross_key = [KEY_INVALID] * nwg
    lead_val = {}            # wg -> value (a slot never written this launch reads as POISON)
    lead_open = [0] * nwg
    skewed, triggers = [], {}
    res.tail_nwalk, res.lead_nwalk = {}, {}
    wg_pass = []
    for wg in range(nwg):
        t0 = wg * ACC_THREADS
        last = lay.last(wg)
        ev.add("last:255" if last == 255 else "last:1" if last == 1 else "last:0" if last == 0 else "last:mid")
        hk = [head[t0 + lt] if lt <= last else None for lt in range(ACC_THREADS)]
        passes = [h is not None and h[1] for h in hk]
        wg_pass.append(passes)
        cross_key[wg] = cur_run[t0 + last] if cont_run[t0 + last] else KEY_INVALID

        def is_pass(r):
            return True if r >= ACC_THREADS else passes[r]  # (past the array: whatever LDS holds)

        def sh_head(r):
            return hk[r][2] if r < ACC_THREADS and hk[r] is not None else POISON

        trig = set()
        for lt in range(ACC_THREADS):
            my = passes[lt]
            nxt = lt < last and is_pass(lt + 1)
            nxt2 = lt + 1 < last and is_pass(lt + 2)
            three = my and nxt and nxt2
            if "skew_three" in F:
                three = three and lt + 2 < last and is_pass(lt + 3)
            if three:
                trig.add("skew:three_at_0" if lt == 0 else "skew:three_at_253" if lt == 253 else "skew:three_mid")
            if lt == 0 and my and last == 0:
                trig.add("skew:lane0_last0")
            if lt == 0 and my and nxt and last == 1:
                trig.add("skew:lanes01_last1")
        if trig:
            skewed.append(wg)
            triggers[wg] = trig
            ev.update(trig)
            # the tail pieces go to the bucket table, heads and keys to g_head / g_hkey / g_tkey
            for lt in range(last + 1):
                if tail[t0 + lt]:
                    buckets[tail[t0 + lt][0]] = tail[t0 + lt][1]
            continue
        # not skewed: every chain has at most two pass heads
        lead_join = passes[0]
        lead_open[wg] = 0
        if hk[0] is None:
            ev.add("lead:none")
        elif not lead_join:
            lead_val[wg] = hk[0][2]
            ev.add("lead:plain")
        for lt in range(last + 1):
            tl = tail[t0 + lt]
            lj = lt == 0 and lead_join
            if not tl and not lj:
                continue
            nxt = lt < last and is_pass(lt + 1)
            nxt2 = (lt + 1 <= last if "nwalk_clip2" in F else lt + 1 < last) and is_pass(lt + 2)
            if lj:
                nwalk = 1 if "lead_join_one" in F else 2 if "lead_join_two" in F else 1 + (1 if nxt else 0)
                acc = hk[0][2]
            else:
                in_wg = lt <= last if "nwalk_tail_last" in F else lt < last
                c1 = nxt if "nwalk_clip1" in F else nxt and lt + 1 < last
                c2 = nxt2 if "nwalk_clip2" in F else nxt2 and lt + 2 < last
                nwalk = (1 + ((1 + (1 if c2 else 0)) if c1 else 0)) if in_wg else 0
                acc = tl[1]
            for j in range(1, nwalk + 1):
                acc = note("walk", (acc + sh_head(lt + j)) % R)
            if lj:
                lead_val[wg] = acc
                res.lead_nwalk[wg] = nwalk
                ev.add("lead:join%d" % nwalk)
            else:
                buckets[tl[0]] = acc
                res.tail_nwalk[t0 + lt] = nwalk
                leaves = lt + nwalk == last and (nwalk == 0 or passes[last])
                ev.add("tail:nwalk%d:%s" % (nwalk, "leaves" if leaves else "closes"))
    res.skewed, res.triggers = skewed, triggers
    res.second_pass = bool(skewed)
    for wg in range(nwg - 1):
        if (wg not in triggers and wg + 1 not in triggers and wg_pass[wg][254] and wg_pass[wg][255]
                and res.lead_nwalk.get(wg + 1) == 2):
            ev.add("join:straddle")
    sk = set(skewed)
    for wg in range(nwg - 1):
        if wg in sk and wg + 1 not in sk:
            ev.add("nb:skewed,unskewed")
            if wg + 2 in sk:
                ev.add("nb:skewed,unskewed,skewed")
        if wg not in sk and wg + 1 in sk:
            ev.add("nb:unskewed,skewed")
    # ---- k_chain_join over the skewed list -------------------------------------------------------
    if len(skewed) > CJ_GRID:
        ev.add("cj:more_than_grid")
    lead_flag = False
    joined = skewed[:CJ_GRID] if "cj_grid_loop" in F else skewed
    nsteps = ACC_THREADS // 2 if "cj_steps" in F else ACC_THREADS
    for wg in joined:
        t0 = wg * ACC_THREADS
        last = lay.last(wg)
        hk = [head[t0 + lt] if lt <= last else None for lt in range(ACC_THREADS)]
        val = [h[2] if h is not None else POISON for h in hk]      # sh_head (unwritten where no head)
        pbit = [h[1] if h is not None else True for h in hk]       # KEY_INVALID has the pass bit set
        # the chains as they are (events): maximal stretches of pass heads
        stretches, lt = [], 0
        while lt < ACC_THREADS:
            if hk[lt] is not None and hk[lt][1]:
                a = lt
                while lt < ACC_THREADS and hk[lt] is not None and hk[lt][1]:
                    lt += 1
                stretches.append((a, lt - a))
            else:
                lt += 1
        for a, n in stretches:
            if n in (3, 4, 5, 7, 8, 9, 16, 17, 255, 256):
                ev.add("cj:chain%d" % n)
            if a + n == ACC_THREADS:
                ev.add("cj:leaves_255")
        if sum(1 for _, n in stretches if n >= 3) >= 2:
            ev.add("cj:two_chains")
        open_ = [h is not None and h[1] for h in hk]
        d = 1
        while d < nsteps:
            upd = []
            for lt in range(ACC_THREADS):
                if not open_[lt]:
                    continue
                if not (lt + d <= ACC_THREADS if "cj_take" in F else lt + d < ACC_THREADS):
                    continue
                r = lt + d
                nv, nopen = (val[r], pbit[r]) if r < ACC_THREADS else (POISON, True)
                upd.append((lt, note("chain", (val[lt] + nv) % R), nopen))
            for lt, v, nopen in upd:
                val[lt] = v
                if "cj_close" not in F:
                    open_[lt] = nopen
                pbit[lt] = open_[lt]
            d <<= 1
        if hk[0] is not None:
            lead_val[wg] = val[0]
            lopen = pbit[0]
        else:
            lopen = False
        lead_open[wg] = 0 if "cj_lead_open" in F else (1 if lopen else 0)
        if lopen:
            lead_flag = True
        for lt in range(last + 1):
            tl = tail[t0 + lt]
            if not tl:
                continue
            acc = buckets[tl[0]]
            if lt + 1 <= ACC_THREADS if "cj_tail" in F else lt + 1 < ACC_THREADS:
                acc = (acc + (val[lt + 1] if lt + 1 < ACC_THREADS else POISON)) % R
                if lt + 1 < ACC_THREADS and hk[lt + 1] is not None and not hk[lt + 1][1]:
                    ev.add("cj:one_head_join")
            if lt == ACC_THREADS - 1:
                ev.add("cj:tail_at_255")
            buckets[tl[0]] = note("chain join", acc)
    # ---- k_lead_scan ------------------------------------------------------------------------------
    res.lead_open = list(lead_open)
    res.open_chains = []
    g = 0
    while g < nwg:
        if lead_open[g]:
            a = g
            while g < nwg and lead_open[g]:
                g += 1
            res.open_chains.append((a, g - a))  # leads a .. g - 1 open, lead g ends the chain
            n = g - a
            if n == 1:
                ev.add("ls:open1")
            if n == 2:
                ev.add("ls:open2")
            for b in range(LS_THREADS, nwg, LS_THREADS):
                if a <= b - 1 < g:
                    ev.add("ls:crosses_tile")
                if g == b - 1:
                    ev.add("ls:closes_on_511")
                if a <= b and g >= b + LS_THREADS:
                    ev.add("ls:whole_tile")
            if g < nwg and g not in sk:
                ev.add("ls:ends_joined_lead" if g in res.lead_nwalk else "ls:ends_plain_lead")
        else:
            g += 1
    if lead_flag:
        ntiles = (nwg + LS_THREADS - 1) // LS_THREADS
        order = range(ntiles) if "ls_tile_order" in F else range(ntiles - 1, -1, -1)
        for tile in order:
            g0 = tile * LS_THREADS
            val = [lead_val.get(g0 + i, POISON) if g0 + i < nwg else 0 for i in range(LS_THREADS)]
            so = [g0 + i < nwg and lead_open[g0 + i] != 0 for i in range(LS_THREADS)]
            open_ = list(so)
            d = 1
            while d < LS_THREADS:
                upd = []
                for i in range(LS_THREADS):
                    if not open_[i]:
                        continue
                    in_tile = i + d <= LS_THREADS if "ls_take" in F else i + d < LS_THREADS
                    if not (in_tile and g0 + i + d < nwg):
                        continue
                    r = i + d
                    nv, nopen = (val[r], so[r]) if r < LS_THREADS else (POISON, True)
                    upd.append((i, note("lead chain", (val[i] + nv) % R), nopen))
                for i, v, nopen in upd:
                    val[i], open_[i], so[i] = v, nopen, nopen
                d <<= 1
            gn = (tile + 1) * LS_THREADS + (1 if "ls_absorb_index" in F else 0)
            for i in range(LS_THREADS):
                if open_[i] and gn < nwg and "ls_absorb" not in F:
                    val[i] = note("lead chain", (val[i] + lead_val.get(gn, POISON)) % R)
            for i in range(LS_THREADS):
                if g0 + i < nwg and lead_open[g0 + i] != 0:
                    lead_val[g0 + i] = val[i]
    res.cross_key = cross_key
    res.lead_val = lead_val
    res.buckets = buckets
    # ---- red1_chunk: a bucket that left its accumulation workgroup takes the next lead ------------
    totals, crossing = {}, []
    KA = K * ACC_THREADS
    for key in np.nonzero(lay.sizes)[0].tolist():
        b0 = bs[key]
        g = (max(b0, 1) - 1) // KA if "red_group" in F else b0 // KA
        v = buckets.get(key, POISON)
        if cross_key[g] == key:
            g0 = (b0 // K) // ACC_THREADS
            crossing.append(key)
            v = (v + lead_val.get(g0 if "red_lead" in F else g0 + 1, POISON)) % R
            if b0 % KA == 0:
                ev.add("red:cross_start_multiple_of_K256")
            if lay.L and lay.B:
                i = (key % lay.B) % lay.L
                nb = min(lay.L, lay.B - (key % lay.B) // lay.L * lay.L)
                if i == 0:
                    ev.add("red:cross_first_of_chunk")
                if i == nb - 1:
                    ev.add("red:cross_last_of_chunk")
        totals[key] = v
    res.totals, res.crossing = totals, crossing
    if pieces is not None:
        for wg, v in lead_val.items():
            pieces("lead_val", v)
        for t in range(nruns):
            if head[t]:
                pieces("head", head[t][2])
            if tail[t]:
                pieces("tail", tail[t][1])
    return res


def events(lay):
    """The named branch classes the layout reaches."""
    return execute(lay).events


def plain_totals(lay, weights=None):
    """Every non-empty bucket's plain sum of weights mod r: what execute's totals must equal."""
    bs = lay.bucket_start
    if weights is None:
        return {int(k): int(lay.sizes[k]) % R for k in np.nonzero(lay.sizes)[0]}
    pre = [0]
    for w in weights:
        pre.append(pre[-1] + int(w))
    return {int(k): (pre[int(bs[k + 1])] - pre[int(bs[k])]) % R for k in np.nonzero(lay.sizes)[0]}
