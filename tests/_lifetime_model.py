"""Lifetime sweep: seeded sequences of operations on live handles, and the model that follows them
(test infrastructure; pure Python: neither torch nor the library is imported here).

Every base the sweep uses is a known multiple k_i G of the subgroup generator and every feature is linear,
so a handle is a list of integers mod r, an Fr vector a list of integers with a form tag, and every output
(value mod r) G -- the closed form of tests/_closed_form.py, followed through a whole sequence.

generate(seed, steps) draws `steps` moves with random.Random(seed) from the state as the model has advanced
it and returns the op records they made.  A move is one op and the records it forces: the audit after an op
that makes a handle, the refused use after a close, a chain's producer, the three calls of a sandwich.  A
record is a plain dict -- printable, replayable -- whose "expect" holds what Model.apply gave:

    {"type": "msm", "values": [v, ..]}        each result is (v mod r) G
    {"type": "points", "ks": ks}              the m points are k_i G
    {"type": "handle", "name": h, "ks": ks}   a new handle of those points (the audit that follows reads them)
    {"type": "table", "ks": [..]}             a new table over those bases
    {"type": "fr", "name": v, "values": [..], "form": f}   the vector's residues, canonical in form f
    {"type": "error", "code": c}              the call is refused with MsmError(c) (or "ValueError")
    {"type": "closed", "open": [names]}       the handles that stay open

and "classes" the transitions the record realises, worked out from the records before it:

    T1  grow            a buffer class (MSM terms, per-point outputs, table rows, Fr elements) larger than ever before
    T2  return          the plan of an earlier launch, with another plan in between: a cached graph is hit
    T3  repeat          the same plan back to back on other inputs: a graph repointed
        T3:shift        back to back the same launch but for a range's first base
    T4  cross           an MSM directly after an op that used dx_pts or fx_proj, or the reverse
    T5  after-refusal   an accepted call directly after a refused one (T5:same entry, T5:other)
    T6  device operand  a chain: the scalars are the device vector the call before wrote, unread in between
    T7  reuse           a handle closed, one of its size and levels created, a plan of the old one run on it
    T8  after-pipeline  a per-point op (T8:point) or a lone MSM (T8:msm) directly after a compute_many* of >= 3
    T9  dense/run       a dense launch directly before or after an 8-word launch on the same handle
    T10 two owners      an op on handle B between two identical ops on handle A, three handles open

`ks` is a list, or ("prog", k0, step, n) for an arithmetic progression.  Large inputs are specs -- a kind,
a seed and a length -- that ks_of / scalar_values / index_values expand, so a record stays small.  The
library call of a record lives in tests/test_gpu_lifetime.py.

    python tests/_lifetime_model.py --seed S [--steps K]      prints the trace with the expected integers
"""
import random

R = 0x04aad957a68b2955982d1347970dec005293a3afc43c8afeb95aee9ac33fd9ff  # the subgroup's order
TOP = 1 << 256
SIZES = (1, 2, 63, 64, 65, 130, 257)      # per-point outputs and handles: each mechanism's smallest change
MSM_SIZES = SIZES + (4097, 16385)         # past one RC_SPAN, past one partition chunk
DENSE_N = 32773                           # at 8 bits the smallest class of n on the dense path (n >> 8 >= 128)
SMALL_SIZES = (1, 2, 3, 4, 6, 8)          # generate(.., small=True): handles a long-way check can afford
WINDOWS = (None, 4, 9, 13, 16, 17, 20)
RUN_LENGTHS = (None, 1, 16)
NARROW_BITS = (1, 8, 33, 64, 128, 253)
NATIVE_BITS = {"bit": 1, "u8": 8, "u16": 16, "u32": 32, "u64": 64, "i8": 8, "i16": 16, "i32": 32, "i64": 64}
WIDE_BITS = {"u128": 128, "i128": 128, "u256": 256, "fr_mont": 256}
TABLE_K = {"fixed": (1, 8), "vector": (1, 8, 9, 20)}
ROWS = (1, 2, 63, 64, 65, 130)
ORACLE_BUDGET = 2500
OP_KINDS = ("create", "close", "msm", "subset", "scale", "combine", "fold", "table", "fr", "chain", "audit",
            "refused")
REFUSALS = ("stray_bit", "device_index", "mont_ge_r", "too_few", "misaligned", "closed")
REFUSAL_CODE = {"stray_bit": -1, "device_index": -1, "mont_ge_r": -1, "too_few": "ValueError", "misaligned": -1,
                "closed": -1}
FR_FNS = ("combine", "fold", "mul", "convert", "powers", "dot")
CLASSES = ("T1", "T2", "T3", "T4", "T5", "T6", "T7", "T8", "T9", "T10")
SCALAR_KINDS = ["full"] + [f"narrow{b}" for b in NARROW_BITS] + list(NATIVE_BITS) + list(WIDE_BITS)
MSM_ENTRIES = ("compute", "compute_device", "compute_many", "compute_many_device")
SUBSET_ENTRIES = ("compute_subset", "compute_subset_device", "compute_subset_many", "compute_subset_many_device")
POINT_OPS = ("scale", "combine", "fold", "audit")


# ---- specs -----------------------------------------------------------------------------------------------
def is_spec(ks):
    return bool(ks) and isinstance(ks[0], str)


def ks_of(spec):
    """A handle's multipliers: a list as it is, ("prog", k0, step, n), or ("list", seed, n): seeded residues
    with 0 (the identity), 1 and r - 1 among them."""
    if not is_spec(spec):
        return spec
    if spec[0] == "prog":
        _, k0, step, n = spec
        return [k0 + i * step for i in range(n)]
    _, seed, n = spec
    rnd = random.Random(seed)
    ks = [rnd.randrange(2, R - 1) for _ in range(n)]
    for j, pos in enumerate(sorted({0, n // 2, n - 1})):
        ks[pos] = (0, 1, R - 1)[(seed + j) % 3]
    return ks


def scalar_kind(spec):
    return spec["kind"] + str(spec["bits"]) if spec["kind"] == "narrow" else spec.get("type") or spec["kind"]


def scalar_values(spec):
    """The integers a scalar vector multiplies by (negative for a signed type's negative elements)."""
    rnd = random.Random(spec["seed"])
    m, kind = spec["m"], spec["kind"]
    at = lambda: rnd.randrange(m)
    if not m:
        return []
    if kind == "full":  # wire words: a fifth at r and above, one 2^256 - 1
        v = [rnd.randrange(R, TOP) if i % 5 == 4 else rnd.randrange(R) for i in range(m)]
        v[at()] = TOP - 1
    elif kind == "narrow":
        b = spec["bits"]
        v = [rnd.getrandbits(b) for _ in range(m)]
        v[at()] = (1 << b) - 1
    elif kind == "native":
        e = NATIVE_BITS[spec["type"]]
        if spec["type"][0] == "i":
            v = [rnd.randrange(-(1 << (e - 1)), 1 << (e - 1)) for _ in range(m)]
            v[at()] = -(1 << (e - 1))
        else:
            v = [rnd.getrandbits(e) for _ in range(m)]
            v[at()] = (1 << e) - 1
    elif kind == "wide":
        t = spec["type"]
        if t == "fr_mont":  # canonical
            v = [rnd.randrange(R) for _ in range(m)]
            v[at()] = R - 1
        elif t == "i128":
            v = [rnd.randrange(-(1 << 127), 1 << 127) for _ in range(m)]
            v[at()] = -(1 << 127)
        else:
            e = WIDE_BITS[t]
            v = [rnd.getrandbits(e) for _ in range(m)]
            v[at()] = (1 << e) - 1
    else:
        raise ValueError(kind)
    return v


def index_values(spec):
    """Base indices below n; m may exceed n, and from m = 2 on one index repeats."""
    if spec is None:
        return None
    rnd = random.Random(spec["seed"])
    idx = [rnd.randrange(spec["n"]) for _ in range(spec["m"])]
    if spec["m"] >= 2:
        idx[rnd.randrange(1, spec["m"])] = idx[0]
    return idx


def compact(ks, prog=None):
    return list(prog) if prog else ks


# ---- the model -------------------------------------------------------------------------------------------
class Handle:
    def __init__(self, ks, levels, prog=None):
        self.ks, self.levels, self.open, self.prog = ks, levels, True, prog

    @property
    def n(self):
        return len(self.ks)


class FrVec:
    def __init__(self, vals, form, where):
        self.vals, self.form, self.where = vals, form, where  # wire: any integer < 2^256, meaning its residue


class Model:
    """Named handles, tables and Fr vectors as integers.  apply(rec) advances the state by one record and
    returns its expectation.  flip=True negates the first non-zero value the op takes in (one sign), so that
    a check of the model can be shown to see each op."""

    def __init__(self):
        self.handles, self.tables, self.frs = {}, {}, {}
        self._flip = False

    def apply(self, rec, flip=False):
        self._flip = flip
        return getattr(self, "_" + rec["op"])(rec)

    def _take(self, values):
        values = list(values)
        if self._flip:
            for i, v in enumerate(values):
                if v % R:
                    values[i] = -v % R
                    self._flip = False
                    break
        return values

    def _bases(self, h, first, idx, m):
        ks = self.handles[h].ks
        return [ks[i] for i in idx] if idx is not None else ks[first:first + m]

    def _scalars(self, sc):
        """A scalar operand: a spec, or {"ref": name} for a live Fr vector (its residues)."""
        if "ref" in sc:
            return [v % R for v in self.frs[sc["ref"]].vals]
        return scalar_values(sc)

    def _new_handle(self, rec, ks):
        self.handles[rec["new"]] = Handle(ks, rec.get("levels") or 1)
        return {"type": "handle", "name": rec["new"], "ks": ks}

    def _create(self, rec):
        spec = rec["ks"]
        ks = self._take(ks_of(spec))
        prog = tuple(spec) if is_spec(spec) and spec[0] == "prog" and ks == ks_of(spec) else None
        self.handles[rec["new"]] = Handle([k % R for k in ks], rec["levels"] or 1, prog)
        return {"type": "handle", "name": rec["new"], "ks": compact(ks, prog)}

    def _close(self, rec):
        if not self._flip:
            self.handles[rec["h"]].open = False
        return {"type": "closed", "open": sorted(k for k, h in self.handles.items() if h.open)}

    def _audit(self, rec):
        h = self.handles[rec["h"]]
        ks = self._take(h.ks)
        return {"type": "points", "ks": compact(ks, h.prog if ks == h.ks else None)}

    def _dots(self, bases, vectors):
        return [sum(s * k for s, k in zip(self._scalars(sc), bases)) % R for sc in vectors]

    def _msm(self, rec):
        return {"type": "msm", "values": self._dots(self._take(self.handles[rec["h"]].ks), rec["sc"])}

    def _subset(self, rec):
        out = []
        for j, sc in enumerate(rec["sc"]):
            ix = rec["idx"][j % len(rec["idx"])] if rec.get("idx") else None
            bases = self._take(self._bases(rec["h"], rec["first"], index_values(ix), rec["m"]))
            out += self._dots(bases, [sc])
        return {"type": "msm", "values": out}

    def _points(self, rec, ks):
        if rec.get("new"):
            return self._new_handle(rec, ks)
        return {"type": "points", "ks": ks}

    def _scale(self, rec):
        bases = self._take(self._bases(rec["h"], rec["first"], index_values(rec.get("idx")), rec["m"]))
        return self._points(rec, [s * k % R for s, k in zip(self._scalars(rec["sc"]), bases)])

    def _side(self, mode, sc, m):
        if mode == "none":
            return [1] * m
        v = self._scalars(sc)
        return v * m if mode == "bcast" else v

    def _combine(self, rec):
        m = rec["m"]
        ka = self._take(self._bases(rec["h"], rec["a_first"], index_values(rec.get("a_idx")), m))
        kb = self._bases(rec["other"] or rec["h"], rec["b_first"], index_values(rec.get("b_idx")), m)
        a, b = self._side(rec["a"], rec.get("a_sc"), m), self._side(rec["b"], rec.get("b_sc"), m)
        sign = -1 if rec["sub"] else 1
        return self._points(rec, [(a[i] * ka[i] + sign * b[i] * kb[i]) % R for i in range(m)])

    def _fold(self, rec):
        ks = self._take(self.handles[rec["h"]].ks)
        h = len(ks) // 2
        xi = 1 if rec["x_inv"] is None else rec["x_inv"]
        return self._new_handle(rec, [(xi * ks[i] + rec["x"] * ks[i + h]) % R for i in range(h)])

    def _table(self, rec):
        if rec["act"] == "create":
            ks = self._take(self._bases(rec["h"], rec["first"], rec.get("idx"), rec["k"]))
            self.tables[rec["new"]] = ks
            return {"type": "table", "ks": ks}
        if rec["act"] == "close":
            del self.tables[rec["t"]]
            return {"type": "closed", "open": sorted(k for k, h in self.handles.items() if h.open)}
        kb = self._take(self.tables[rec["t"]])
        sc, k = self._scalars(rec["sc"]), len(kb)
        return self._points(rec, [sum(sc[i * k + j] * kb[j] for j in range(k)) % R for i in range(rec["m"])])

    def _chain(self, rec):
        return getattr(self, "_" + rec["via"])(rec)

    def _fr_operand(self, o):
        """None, an int, a spec, or {"ref": name}: the integers as the operand's form holds them."""
        if o is None or isinstance(o, int):
            return o
        return list(self.frs[o["ref"]].vals) if "ref" in o else scalar_values(o)

    def _fr(self, rec):
        fn = rec["fn"]
        if fn == "powers":
            g, first = self._take([rec["g"]])[0], 1 if rec["first"] is None else rec["first"]
            out = [first * pow(g, i, R) % R for i in range(rec["m"])]
        else:
            a = self._take(self._fr_operand(rec["a"]))
            b, x, y = (self._fr_operand(rec.get(k)) for k in ("b", "x", "y"))
            if fn == "fold":
                h = len(a) // 2
                a, b = a[:h], a[h:]
            at = lambda v, i: 1 if v is None else v if isinstance(v, int) else v[i % len(v)]
            sign = -1 if rec.get("sub") else 1
            if fn == "dot":
                out = [sum(u * (1 if b is None else b[i]) for i, u in enumerate(a)) % R]
            else:
                out = [(at(x, i) * a[i] + (sign * at(y, i) * b[i] if b is not None else 0)) % R for i in range(len(a))]
        name = rec.get("out") or rec.get("new")
        if rec.get("out"):  # in place: into an operand, or a fold into its own low half
            vec = self.frs[name]
            vec.vals[:len(out)] = out
            out = list(vec.vals)
        elif rec["where"] == "device" and fn != "dot":
            self.frs[name] = FrVec(out, rec["out_form"], "device")
        return {"type": "fr", "name": name, "values": [v % R for v in out], "form": rec["out_form"]}

    def _refused(self, rec):
        code = REFUSAL_CODE[rec["why"]]
        return {"type": "error", "code": -2 if self._flip else code}


# ---- the generator -----------------------------------------------------------------------------------------
def _core(rec):
    return {k: v for k, v in rec.items() if k not in ("expect", "classes", "i", "twin", "defer")}


class Generator:
    def __init__(self, seed, steps, small=False):
        self.rnd, self.seed, self.steps, self.small = random.Random(seed), seed, steps, small
        self.model, self.recs = Model(), []
        self.oracle, self.seen = 0, set()
        self.uid = 0
        self.decks = {}
        self.maxsize = {}      # T1: the largest size each buffer class has seen
        self.plans = []        # T2: the plan keys of the msm launches, in order
        self.hplans = {}       # T7: handle -> its plans without the handle's name
        self.reuse = {}        # T7: handle -> the closed handle of equal size and levels it follows
        self.moves_left = steps
        self.sizes = SMALL_SIZES if small else SIZES

    # -- bookkeeping --
    def name(self, prefix):
        self.uid += 1
        return f"{prefix}{self.uid}"

    def deal(self, items):
        """The next of a shuffled deck of `items` (a new shuffle when it runs out): every one comes up in turn."""
        deck = self.decks.setdefault(tuple(items), [])
        if not deck:
            deck += self.rnd.sample(list(items), len(items))
        return deck.pop()

    def seed_(self):
        return self.rnd.randrange(1 << 30)

    def left(self):
        return ORACLE_BUDGET - self.oracle

    def cap(self):
        """The largest per-point output this move may ask for: every later move keeps a dozen multiplications."""
        return max(2, self.left() - 12 * self.moves_left)

    def size(self, pool=None, at_most=None):
        cap = self.cap() if at_most is None else min(self.cap(), at_most)
        ok = [s for s in (pool or self.sizes) if s <= cap] or [1]
        return self.rnd.choice(ok)

    def _need(self, values):
        for v in values:
            v %= R
            if v not in self.seen:
                self.seen.add(v)
                self.oracle += 1

    def _count(self, e):
        if e["type"] == "msm":
            self._need(e["values"])
        elif e["type"] == "points" and not is_spec(e["ks"]):
            self._need(e["ks"])

    def open_handles(self, pred=lambda h: True):
        return [k for k, h in self.model.handles.items() if h.open and pred(h)]

    def emit(self, rec):
        rec["expect"] = self.model.apply(rec)
        self._count(rec["expect"])
        rec["i"] = len(self.recs)
        rec["classes"] = self._classes(rec)
        self.recs.append(rec)
        if rec["expect"]["type"] == "handle":
            self.emit({"op": "audit", "h": rec["expect"]["name"], "entry": "scale", "bufs": ["dx"],
                       "grow": ["pt", self.model.handles[rec["expect"]["name"]].n]})
        return rec

    def _classes(self, rec):
        out, prev = [], self.recs[-1] if self.recs else None
        if rec.get("grow"):
            cls, size = rec["grow"]
            if cls in self.maxsize and size > self.maxsize[cls]:
                out.append("T1")
            self.maxsize[cls] = max(size, self.maxsize.get(cls, 0))
        plan = rec.get("plan")
        if plan:
            if plan in self.plans:
                last = len(self.plans) - 1 - self.plans[::-1].index(plan)
                if any(p != plan for p in self.plans[last + 1:]):
                    out.append("T2")
            if prev and prev.get("plan") == plan and prev["sc"] != rec["sc"]:
                out.append("T3")
            # T3:shift -- back to back the same launch but for the range's first base, a dimension of the plan
            # that no size or grid depends on: only a cached graph's key tells the two apart
            if prev and prev.get("plan") and prev["plan"] != plan and "|range" in plan and \
                    prev["plan"].rsplit("|range", 1)[0] == plan.rsplit("|range", 1)[0]:
                out.append("T3:shift")
            self.plans.append(plan)
            bare = plan.split("|", 1)[1]
            if rec["h"] in self.reuse and bare in self.hplans.get(self.reuse[rec["h"]], ()):
                out.append("T7")
            self.hplans.setdefault(rec["h"], set()).add(bare)
        if prev:
            pb, rb = set(prev.get("bufs", ())), set(rec.get("bufs", ()))
            if ("msm" in rb and pb & {"dx", "fx"}) or ("msm" in pb and rb & {"dx", "fx"}):
                out.append("T4")
            if prev["op"] == "refused" and rec["op"] != "refused":
                out += ["T5", "T5:same" if rec.get("entry") == prev.get("entry") else "T5:other"]
            sc = rec.get("sc")
            ref = (sc[0] if isinstance(sc, list) else sc or {}).get("ref")
            if rec["op"] == "chain" and prev.get("defer") and prev["expect"].get("name") == ref:
                out.append("T6")
            if prev.get("plan") and prev.get("count", 1) >= 3 and "many" in prev["entry"]:
                if rec.get("plan") and rec["count"] == 1 and "many" not in rec["entry"]:
                    out += ["T8", "T8:msm"]
                elif rec["op"] in POINT_OPS or rec.get("via") in ("scale", "table") or rec.get("act") == "mul":
                    out += ["T8", "T8:point"]
            # 8-word scalars never take the dense path, so such a launch accumulates by runs (k_accumulate)
            runs = lambda r: not r.get("dense") and r["sc"][0].get("kind") == "full"
            if prev.get("plan") and plan and prev["h"] == rec["h"] and \
                    ((prev.get("dense") and runs(rec)) or (runs(prev) and rec.get("dense"))):
                out += ["T9", "T9:dense>run" if prev.get("dense") else "T9:run>dense"]
        if "twin" in rec:
            first = self.recs[rec["twin"]]
            between = self.recs[rec["twin"] + 1:]
            if _core(first) == _core(rec) and any(r.get("h", rec["h"]) != rec["h"] for r in between) and \
                    len(self.open_handles()) >= 3:
                out.append("T10")
        return out

    # -- operands --
    def sc_spec(self, m, kind=None):
        kind = kind or self.deal(SCALAR_KINDS)
        if kind == "full":
            return {"kind": "full", "seed": self.seed_(), "m": m}
        if kind.startswith("narrow"):
            return {"kind": "narrow", "bits": int(kind[6:]), "seed": self.seed_(), "m": m}
        return {"kind": "native" if kind in NATIVE_BITS else "wide", "type": kind, "seed": self.seed_(), "m": m}

    def point_sc(self, m):
        """scale, combine and the tables take wire words or narrow ones."""
        return self.sc_spec(m, self.rnd.choice(["full", "full"] + [f"narrow{b}" for b in NARROW_BITS]))

    def idx_spec(self, n, m):
        return {"seed": self.seed_(), "n": n, "m": m}

    def handle(self, pred=lambda h: True, make=None):
        """An open handle that fits, or a new one (made by an extra create)."""
        ok = self.open_handles(pred)
        if ok:
            return self.rnd.choice(ok)
        return (make or self.create)()

    # -- moves: every one emits at least one record and returns the handle or record it was about --
    def create(self, n=None, levels=None, prog=None):
        n = n or self.deal(self.sizes if self.small else MSM_SIZES)
        if not prog:  # a seeded list costs the oracle one multiplication per point
            prog = n > max(SIZES) or n > self.cap() or (prog is None and self.rnd.random() < 0.5)
        spec = ["prog", self.rnd.randrange(1, 1000), self.rnd.randrange(1, 50), n] if prog else ["list", self.seed_(), n]
        rec = {"op": "create", "how": self.rnd.choice(["wire", "device", "x"]), "new": self.name("h"), "ks": spec,
               "levels": self.rnd.choice([0, 1, 2]) if levels is None else levels,
               "entry": "create", "grow": ["pt", n]}
        rec["bufs"] = ["dx"] if rec["how"] == "x" else []
        name = rec["new"]
        for old, h in self.model.handles.items():
            if not h.open and h.n == n and h.levels == (rec["levels"] or 1) and old in self.hplans:
                self.reuse[name] = old
        self.emit(rec)
        return name

    def close(self):
        if len(self.open_handles()) < 2:
            self.create()
        with_plans = [h for h in self.open_handles() if h in self.hplans]
        h = self.rnd.choice(with_plans or self.open_handles())
        self.emit({"op": "close", "h": h, "entry": "destroy"})
        self.refused("closed", h)
        return h

    def _plan(self, rec, n_terms):
        sc = rec["sc"][0]
        kind = ("ref_mont" if sc.get("mont") else "ref") if "ref" in sc else scalar_kind(sc)
        sub = "none" if rec["op"] not in ("subset",) else ("idx" if rec.get("idx") else f"range{rec['first']}")
        return "|".join(str(v) for v in (rec["h"], n_terms, self.model.handles[rec["h"]].levels, rec["entry"], rec["count"],
                                         rec["window"], rec["run_length"], kind, sub))

    def msm(self, h=None, like=None, kind=None, entry=None, count=None, window=0, dense=False):
        """One MSM record on h; `like` repeats that record's plan with new scalars."""
        if like:
            rec = dict(_core(like))
            rec["sc"] = [dict(sc, seed=self.seed_()) for sc in like["sc"]]
            return self.emit(rec)
        if not h and self.rnd.random() < 0.5:  # a handle no MSM has run on yet, where there is one
            fresh = [k for k in self.open_handles(lambda x: x.n != DENSE_N) if k not in self.hplans]
            h = self.rnd.choice(fresh) if fresh else None
        h = h or self.handle(lambda x: x.n != DENSE_N)
        hd = self.model.handles[h]
        entry = entry or self.rnd.choice(MSM_ENTRIES)
        count = count or (self.rnd.randrange(1, 6) if "many" in entry else 1)
        if "many" not in entry:
            count = 1
        kind = kind or self.deal(SCALAR_KINDS)
        if window == 0:
            window = self.rnd.choice(WINDOWS)
        if kind == "full" and hd.levels > 1:
            window = None  # a folded handle keeps its own width for the 8-word call
        rec = {"op": "msm", "h": h, "entry": entry, "count": count, "window": window,
               "run_length": None if dense else self.rnd.choice(RUN_LENGTHS),
               "sc": [self.sc_spec(hd.n, kind) for _ in range(count)], "bufs": ["msm"], "grow": ["msm", hd.n * count]}
        if dense:
            rec["dense"] = True
        rec["plan"] = self._plan(rec, hd.n)
        return self.emit(rec)

    def subset(self):
        h = self.handle()
        hd = self.model.handles[h]
        entry = self.rnd.choice(SUBSET_ENTRIES)
        count = self.rnd.randrange(1, 6) if "many" in entry else 1
        kind = self.deal(SCALAR_KINDS)
        window = None if kind == "full" and hd.levels > 1 else self.rnd.choice(WINDOWS)
        if self.rnd.random() < 0.5:  # an index list: repeats, m above n, m = 1
            m = self.rnd.choice([1] + list(self.sizes if self.small else MSM_SIZES[:8]))
            per = self.rnd.random() < 0.5
            idx, first = [self.idx_spec(hd.n, m) for _ in range(count if per else 1)], 0
        else:
            m = self.rnd.choice([s for s in (self.sizes if self.small else MSM_SIZES) if s <= hd.n])
            idx, first = None, self.rnd.randrange(0, hd.n - m + 1)
        rec = {"op": "subset", "h": h, "entry": entry, "count": count, "window": window,
               "run_length": self.rnd.choice(RUN_LENGTHS), "first": first, "m": m, "idx": idx,
               "sc": [self.sc_spec(m, kind) for _ in range(count)], "bufs": ["msm"], "grow": ["msm", m * count]}
        rec["plan"] = self._plan(rec, m)
        return self.emit(rec)

    def _pick(self, hd, m):
        """m bases of a handle as a range, or as an index list (the only way past its end): (first, idx spec)."""
        if hd.n < m or self.rnd.random() < 0.4:
            return 0, self.idx_spec(hd.n, m)
        return self.rnd.randrange(0, hd.n - m + 1), None

    def scale(self, sc=None, h=None):
        """sc given: a chain's consumer of that device vector, over all of h."""
        if sc:
            hd = self.model.handles[h]
            first, idx, m = 0, None, hd.n
            entry = self.rnd.choice(["scale_device", "scaled_device"])
        else:
            h = self.handle(lambda x: x.n <= 257)
            hd = self.model.handles[h]
            m = self.size()
            first, idx = self._pick(hd, m)
            entry = self.rnd.choice(["scale", "scale_device", "scaled", "scaled_device"])
        rec = {"op": "chain" if sc else "scale", "h": h, "entry": entry, "first": first, "idx": idx, "m": m,
               "sc": sc or self.point_sc(m), "grow": ["pt", m]}
        if sc:
            rec["via"] = "scale"
        rec["bufs"] = ["dx"] if entry == "scale" else []
        if entry.startswith("scaled"):
            rec.update(new=self.name("h"), levels=self.rnd.choice([0, 1, 2]))
        return self.emit(rec)

    def combine(self):
        a = self.handle(lambda x: x.n <= 257)
        b = self.rnd.choice([None] + self.open_handles(lambda x: x.n <= 257))
        ha, hb = self.model.handles[a], self.model.handles[b or a]
        m = self.size()
        (a_first, a_idx), (b_first, b_idx) = self._pick(ha, m), self._pick(hb, m)
        entry = self.rnd.choice(["combine", "combine_device", "combined", "combined_device"])
        kind = self.rnd.choice(["full", "full"] + [f"narrow{b}" for b in NARROW_BITS])
        rec = {"op": "combine", "h": a, "other": b, "entry": entry, "m": m, "a_first": a_first, "b_first": b_first,
               "a_idx": a_idx, "b_idx": b_idx, "sub": self.rnd.random() < 0.5, "grow": ["pt", m],
               "bufs": ["fx", "dx"] if entry == "combine" else ["fx"]}
        for side in "ab":
            rec[side] = mode = self.rnd.choice(["none", "bcast", "each"])
            if mode != "none":
                rec[side + "_sc"] = self.sc_spec(1 if mode == "bcast" else m, kind)
        if rec["a"] == rec["b"] == "none":
            rec["b"], rec["b_sc"] = "each", self.sc_spec(m, kind)
        if entry.startswith("combined"):
            rec.update(new=self.name("h"), levels=self.rnd.choice([0, 1, 2]))
        return self.emit(rec)

    def fold(self):
        even = lambda x: x.n % 2 == 0 and x.n // 2 <= self.cap() and x.n <= 257
        pool = [s for s in self.sizes if s % 2 == 0 and s // 2 <= self.cap()] or [2]
        h = self.handle(even, lambda: self.create(n=self.rnd.choice(pool)))
        x = self.rnd.randrange(2, R)
        x_inv = self.rnd.choice([None, pow(x, -1, R), self.rnd.randrange(R)])
        return self.emit({"op": "fold", "h": h, "x": x, "x_inv": x_inv, "new": self.name("h"), "entry": "combined",
                          "levels": self.rnd.choice([0, 1, 2]), "bufs": ["fx"], "grow": ["pt", self.model.handles[h].n // 2]})

    def table(self, sc=None, t=None, m=None):
        """A table op: a mul on a live table, which a create precedes when there is none to reuse (or by choice)."""
        if t is None and (not self.model.tables or self.rnd.random() < 0.5):
            kind = self.rnd.choice(["fixed", "vector"])
            k = self.rnd.choice(TABLE_K[kind] if not self.small else (1, 2, 3))
            h = self.handle(lambda x: x.n <= 257)
            hd = self.model.handles[h]
            rec = {"op": "table", "act": "create", "kind": kind, "h": h, "k": k, "new": self.name("t"), "first": 0,
                   "idx": None, "entry": "table_create", "bufs": ["dx"]}
            if hd.n < k or self.rnd.random() < 0.5:
                rec["idx"] = index_values(self.idx_spec(hd.n, k))
            else:
                rec["first"] = self.rnd.randrange(0, hd.n - k + 1)
            self.emit(rec)
            if len(self.model.tables) > 3:
                self.emit({"op": "table", "act": "close", "t": next(iter(self.model.tables)), "entry": "table_destroy"})
            t = rec["new"]
        t = t or self.rnd.choice(sorted(self.model.tables))
        k = len(self.model.tables[t])
        m = m or self.size((1, 2, 3) if self.small else ROWS)
        entry = self.rnd.choice(["mul_device", "mul_bases_device"] if sc else ["mul", "mul_device", "mul_bases", "mul_bases_device"])
        rec = {"op": "chain" if sc else "table", "act": "mul", "t": t, "m": m, "entry": entry, "sc": sc or self.point_sc(m * k),
               "grow": ["fx", m], "bufs": ["fx", "dx"] if entry == "mul" else ["fx"]}
        if sc:
            rec["via"] = "table"
        if "bases" in entry:
            rec.update(new=self.name("h"), levels=self.rnd.choice([0, 1, 2]))
        return self.emit(rec)

    def fr_operand(self, m, form, where, rec=None):
        """A fresh vector, or a live device vector of that length and form (none that `rec` already reads: an
        in-place result may overlap no other operand)."""
        used = [o["ref"] for o in (rec or {}).values() if isinstance(o, dict) and "ref" in o]
        live = [k for k, v in self.model.frs.items() if len(v.vals) == m and v.form == form and k not in used]
        if where == "device" and live and self.rnd.random() < 0.6:
            return {"ref": self.rnd.choice(live)}
        return self.sc_spec(m, "full" if form == "wire" else "fr_mont")

    def fr(self, m=None, where=None, out_form=None, defer=False, fn=None):
        """One Fr op.  A chain's producer (defer) is a device op of length m whose result is a new vector."""
        fn = fn or self.rnd.choice(FR_FNS if not defer else ("combine", "mul", "convert", "powers", "fold"))
        where = where or self.rnd.choice(["host", "device"])
        form = self.rnd.choice(["wire", "fr_mont"])
        free = out_form is None  # no caller has fixed the result's form
        out_form = out_form or self.rnd.choice(["wire", "fr_mont"])
        m = m or self.rnd.choice(self.sizes if self.small else SIZES + (4097,))
        into = None  # in place: the result goes into a live device vector, which is then an operand
        if where == "device" and free and not defer and fn in ("combine", "mul", "convert", "fold") and self.model.frs and \
                self.rnd.random() < 0.5:
            name = self.rnd.choice(sorted(self.model.frs))
            vec = self.model.frs[name]
            if fn != "fold" or len(vec.vals) % 2 == 0:
                into, form, out_form, m = name, vec.form, vec.form, len(vec.vals) // (2 if fn == "fold" else 1)
        rec = {"op": "fr", "fn": fn, "where": where, "form": form, "out_form": out_form, "m": m,
               "entry": "fr_" + ("powers" if fn == "powers" else "dot" if fn == "dot" else "combine") +
               ("_device" if where == "device" else ""), "grow": ["fr", m]}
        rec["bufs"] = ["dx"] if where == "host" else []
        mult = lambda: self.rnd.choice([None, self.rnd.randrange(TOP if form == "wire" else R),
                                        self.fr_operand(1, form, where, rec), self.fr_operand(m, form, where, rec)])
        if fn == "powers":
            rec.update(g=self.rnd.choice([0, 1, R - 1, 2, self.rnd.randrange(TOP)]),
                       first=self.rnd.choice([None, self.rnd.randrange(TOP)]))
            del rec["form"]
        elif fn == "fold":
            rec["a"] = {"ref": into} if into else self.fr_operand(2 * m, form, where)
            rec["x"] = self.rnd.randrange(2, R)
            rec["y"] = self.rnd.choice([None, pow(rec["x"], -1, R)])
        elif fn == "mul":
            rec["a"] = {"ref": into} if into else self.fr_operand(m, form, where)
            rec["x"] = mult() or 5
        elif fn == "convert":
            rec["a"] = {"ref": into} if into else self.fr_operand(m, form, where)
        elif fn == "dot":
            rec["a"] = self.fr_operand(m, form, where)
            rec["b"] = self.rnd.choice([None, self.fr_operand(m, form, where, rec)])
        else:
            second = into and self.rnd.random() < 0.5  # the result into the second operand
            rec["a"] = {"ref": into} if into and not second else self.fr_operand(m, form, where, {"b": {"ref": into}})
            rec["x"] = mult()
            if second or self.rnd.random() < 0.7:
                rec["b"] = {"ref": into} if second else self.fr_operand(m, form, where, rec)
                rec.update(y=mult(), sub=self.rnd.random() < 0.5)
        if fn != "dot" and where == "device":
            if into:
                rec["out"] = into
            else:
                rec["new"] = self.name("v")
            if defer:
                rec["defer"] = True
        self.emit(rec)
        while len(self.model.frs) > 4:  # the oldest vector is forgotten, unread
            del self.model.frs[next(iter(self.model.frs))]
        return rec

    def chain(self):
        """A device Fr vector made by one library call and consumed by the next, with no readback between."""
        via = self.rnd.choice(["msm", "msm", "scale", "table"])
        if via == "msm":
            h = self.handle(lambda x: x.n <= 4097)
            n = self.model.handles[h].n
            mont = self.rnd.random() < 0.3  # the consumer reads Montgomery memory itself
            prod = self.fr(m=n, where="device", out_form="fr_mont" if mont else "wire", defer=True)
            hd = self.model.handles[h]
            entry = self.rnd.choice(["compute_device", "compute_many_device"])
            window = None if not mont and hd.levels > 1 else self.rnd.choice(WINDOWS)
            rec = {"op": "chain", "via": "msm", "h": h, "entry": entry, "count": 1, "window": window,
                   "run_length": self.rnd.choice(RUN_LENGTHS), "sc": [{"ref": prod["new"], "mont": mont}],
                   "bufs": ["msm"], "grow": ["msm", n]}
            rec["plan"] = self._plan(rec, n)
            return self.emit(rec)
        if via == "scale":
            h = self.handle(lambda x: x.n <= min(257, self.cap()), lambda: self.create(n=self.size()))
            n = self.model.handles[h].n
        else:
            if not self.model.tables:
                self.table()
            t = self.rnd.choice(sorted(self.model.tables))
            rows = self.size((1, 2, 3) if self.small else ROWS)
            n = rows * len(self.model.tables[t])
        if self.rnd.random() < 0.4:  # Montgomery memory goes through fr_convert, which is then the producer
            first = self.fr(m=n, where="device", out_form="fr_mont", fn=self.rnd.choice(["powers", "mul"]))
            src = first.get("new") or first["out"]
            prod = self.emit({"op": "fr", "fn": "convert", "where": "device", "form": "fr_mont", "out_form": "wire", "m": n,
                              "a": {"ref": src}, "new": self.name("v"), "defer": True, "entry": "fr_combine_device",
                              "grow": ["fr", n], "bufs": []})
        else:
            prod = self.fr(m=n, where="device", out_form="wire", defer=True)
        sc = {"ref": prod["new"]}
        return self.scale(sc, h) if via == "scale" else self.table(sc, t, rows)

    def refused(self, why=None, h=None):
        why = why or self.deal(REFUSALS[:-1])
        rec = {"op": "refused", "why": why}
        if why == "closed":
            rec.update(h=h, entry=self.rnd.choice(["compute", "compute_device", "compute_subset", "scale", "info"]))
        elif why == "stray_bit":
            h = self.handle()
            n = self.model.handles[h].n
            rec.update(h=h, entry=self.rnd.choice(MSM_ENTRIES), sc=self.sc_spec(n, "narrow33"), bad_at=self.rnd.randrange(n))
        elif why == "device_index":
            h = self.handle()
            n = self.model.handles[h].n
            m = self.size()
            rec.update(h=h, entry="compute_subset_device", idx=self.idx_spec(n, m), sc=self.sc_spec(m, "full"),
                       bad_at=self.rnd.randrange(m), bad=self.rnd.choice([n, (1 << 32) - 1]))
        elif why == "mont_ge_r":
            m = self.rnd.choice(self.sizes)
            rec.update(entry=self.rnd.choice(["fr_combine_device", "fr_dot_device", "compute_device"]),
                       sc=self.sc_spec(m, "fr_mont"), bad_at=self.rnd.randrange(m), bad=R + self.rnd.randrange(1000))
            if rec["entry"] == "compute_device":
                h = self.handle()
                m = self.model.handles[h].n
                rec.update(h=h, sc=self.sc_spec(m, "fr_mont"), bad_at=self.rnd.randrange(m))
        elif why == "too_few":
            h = self.handle()
            rec.update(h=h, entry=self.rnd.choice(["compute", "compute_many"]),
                       sc=self.sc_spec(self.model.handles[h].n - 1, "full"))
        elif why == "misaligned":
            rec.update(entry=self.rnd.choice(["fr_combine_device", "fr_dot_device", "fr_powers_device"]),
                       m=self.rnd.choice(self.sizes))
        return self.emit(rec)

    # -- the transitions that chance alone would not promise --
    def t2_return(self):
        a = self.msm()
        self.msm(h=self.handle(lambda x: x.n != DENSE_N))
        if self.recs[-1]["plan"] == a["plan"]:
            self.subset()
        return self.msm(like=a)

    def t3_repeat(self):
        return self.msm(like=self.msm())

    def t3_shift(self):
        """Two ranges of one length in one handle, one launch after the other."""
        big = lambda x: 130 <= x.n <= 4097
        h = self.handle(big, lambda: self.create(n=self.rnd.choice([130, 257, 4097]), prog=True))
        hd = self.model.handles[h]
        m = self.rnd.choice([s for s in MSM_SIZES if 63 <= s <= hd.n - 3])
        firsts = self.rnd.sample(range(1, hd.n - m + 1), 2)  # neither is 0: the range [0, m) is the plain launch
        entry = self.rnd.choice(SUBSET_ENTRIES)
        count = self.rnd.randrange(1, 4) if "many" in entry else 1
        kind = self.deal(SCALAR_KINDS)
        base = {"op": "subset", "h": h, "entry": entry, "count": count,
                "window": None if kind == "full" and hd.levels > 1 else self.rnd.choice(WINDOWS),
                "run_length": self.rnd.choice(RUN_LENGTHS), "m": m, "idx": None, "bufs": ["msm"], "grow": ["msm", m * count]}
        for first in firsts:
            rec = dict(base, first=first, sc=[self.sc_spec(m, kind) for _ in range(count)])
            rec["plan"] = self._plan(rec, m)
            self.emit(rec)

    def t5_same(self):
        """A refused device call, then the same entry accepted."""
        h = self.handle(lambda x: x.n != DENSE_N)
        n = self.model.handles[h].n
        entry = self.rnd.choice(["compute_device", "compute_many_device", "compute"])
        self.emit({"op": "refused", "why": "stray_bit", "h": h, "entry": entry, "sc": self.sc_spec(n, "narrow33"),
                   "bad_at": self.rnd.randrange(n)})
        return self.msm(h=h, kind="narrow33", entry=entry)

    def t5_other(self):
        self.refused()
        return self.rnd.choice([self.scale, self.fr, self.subset])()

    def t7_reuse(self):
        n, lv = self.rnd.choice(self.sizes if self.small else MSM_SIZES[:8]), self.rnd.choice([1, 2])
        h = self.create(n=n, levels=lv, prog=True)
        a = self.msm(h=h)
        self.emit({"op": "close", "h": h, "entry": "destroy"})
        self.refused("closed", h)
        h2 = self.create(n=n, levels=lv, prog=True)
        rec = dict(_core(a), h=h2, sc=[dict(sc, seed=self.seed_()) for sc in a["sc"]])
        rec["plan"] = self._plan(rec, n)
        return self.emit(rec)

    def t8_after_pipeline(self):
        h = self.handle(lambda x: x.n != DENSE_N)
        self.msm(h=h, entry=self.rnd.choice(["compute_many", "compute_many_device"]), count=self.rnd.randrange(3, 6))
        if self.rnd.random() < 0.5:
            return self.msm(h=h, entry=self.rnd.choice(["compute", "compute_device"]))
        return self.rnd.choice([self.scale, self.combine])()

    def t9_dense_run(self):
        n = 8 if self.small else DENSE_N
        h = self.handle(lambda x: x.n == n, lambda: self.create(n=n, levels=1, prog=True))
        dense = lambda: self.msm(h=h, kind=self.rnd.choice(["narrow8", "u8"]), entry=self.rnd.choice(["compute", "compute_device"]),
                                 window=None, dense=True)
        run = lambda: self.msm(h=h, kind="full", entry=self.rnd.choice(["compute", "compute_device"]), window=None)
        order = [dense, run, dense] if self.rnd.random() < 0.5 else [run, dense, run]
        for f in order:
            f()

    def t10_two_owners(self):
        while len(self.open_handles(lambda x: x.n != DENSE_N)) < 3:
            self.create(prog=True)
        a, b = self.rnd.sample(self.open_handles(lambda x: x.n != DENSE_N), 2)
        first = self.msm(h=a)
        if self.rnd.random() < 0.5:
            self.msm(h=b)
        else:  # its points are in the oracle's cache since the audit that followed its creation
            self.emit({"op": "audit", "h": b, "entry": "scale", "bufs": ["dx"], "grow": ["pt", self.model.handles[b].n]})
        return self.emit(dict(_core(first), twin=first["i"]))

    FREE = ("fr", "refused", "close")  # moves that need no oracle work

    def run(self):
        kinds = [k for k in OP_KINDS if k != "audit"]
        if self.small:
            plan = kinds + ["t3_repeat"]
        else:
            plan = kinds * 2 + ["refused", "t2_return", "t3_repeat", "t3_shift", "t5_same", "t5_other", "t7_reuse", "t8_after_pipeline",
                                "t9_dense_run", "t10_two_owners"]
        self.rnd.shuffle(plan)
        weights = kinds + ["msm", "subset", "chain", "fr", "t2_return", "t3_repeat", "t5_same", "t8_after_pipeline"]
        while len(plan) < self.steps:
            plan.insert(self.rnd.randrange(len(plan) + 1), self.rnd.choice(weights))
        self.create()
        for move in plan[:self.steps]:
            self.moves_left -= 1
            if self.left() < 12 and move not in self.FREE:
                move = self.rnd.choice(self.FREE)
            getattr(self, move)()
        for h in self.open_handles():  # every live handle, at the end (points the oracle has already made)
            self.emit({"op": "audit", "h": h, "entry": "scale", "bufs": ["dx"], "grow": ["pt", self.model.handles[h].n]})
        return self.recs


def generate(seed, steps=40, small=False):
    """(records, distinct oracle multiplications the expectations need)."""
    g = Generator(seed, steps, small)
    return g.run(), g.oracle


SEEDS = (101, 202, 303, 404, 505, 606)  # the committed sequences, 40 steps each
STEPS = 40


def _short(v):
    if isinstance(v, dict):
        return {k: _short(x) for k, x in v.items()}
    if isinstance(v, list) and len(v) > 6 and all(isinstance(x, int) for x in v):
        return f"[{v[0]:#x}, {v[1]:#x}, .. {len(v)} values .. {v[-1]:#x}]"
    if isinstance(v, list):
        return [_short(x) for x in v]
    return hex(v) if isinstance(v, int) and v > 1 << 32 else v


def show(rec, full=False):
    return repr(rec if full else _short(rec))


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description="print a lifetime sequence with the expected integers (CPU only)")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--full", action="store_true", help="every integer of every list")
    args = ap.parse_args()
    recs, count = generate(args.seed, args.steps)
    for r in recs:
        print(f"{r['i']:3d} {r['op']:8s} {' '.join(r['classes']):24s} {show(r, args.full)}")
    print(f"{len(recs)} records, {count} oracle multiplications")
