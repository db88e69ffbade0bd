"""CPU checks of the lifetime sweep's generator and model (tests/_lifetime_model.py): the committed seeds
realise every op kind, refusal, scalar kind and transition class the GPU test relies on, inside the oracle
budget and reproducibly; and the model is held to a reference of its own -- on short sequences over handles
of at most 8 points every expectation is recomputed the long way, on actual points with oracle.scalar_mul and
oracle.aff_add and on Fr values with plain integers, and a sign flipped in any op's apply is seen at that op."""
import collections
import functools
import subprocess
import sys

import pytest

import _lifetime_model as L
from oracle import oracle as O

R = L.R
SHORT = (11, 12)  # two sequences of 12 moves on small handles


@functools.lru_cache(maxsize=None)
def _sequence(seed):
    return L.generate(seed, L.STEPS)


def _operands(rec):
    sc = rec.get("sc")
    specs = list(sc) if isinstance(sc, list) else [sc] if sc else []
    specs += [rec[k] for k in ("a_sc", "b_sc") if rec.get(k)]
    return [s for s in specs if "ref" not in s]


# ---- conditions on the generator ---------------------------------------------------------------------------
def test_constants_match_the_library():
    import msm_amd as M

    assert L.R == M.FR_MODULUS == O.R_ORDER
    assert set(L.NATIVE_BITS) == set(M.SCALAR_TYPES) and all(M.SCALAR_TYPES[k][2] == e for k, e in L.NATIVE_BITS.items())
    assert set(L.WIDE_BITS) == set(M.WIDE_TYPES) and all(M.WIDE_TYPES[k][1] == e for k, e in L.WIDE_BITS.items())


@pytest.mark.parametrize("seed", L.SEEDS)
def test_every_sequence_has_every_op_kind_and_its_own_transitions(seed):
    recs, count = _sequence(seed)
    ops = collections.Counter(r["op"] for r in recs)
    assert all(ops[k] >= 2 for k in L.OP_KINDS), ops
    classes = collections.Counter(c for r in recs for c in r["classes"])
    assert all(classes[c] >= 1 for c in ("T2", "T3", "T3:shift", "T5", "T6")), classes
    assert count <= L.ORACLE_BUDGET
    made, closed = [], set()
    for r in recs:
        if r["expect"]["type"] == "handle":  # an audit directly after every op that makes a handle
            made.append(r["expect"]["name"])
            assert recs[r["i"] + 1]["op"] == "audit" and recs[r["i"] + 1]["h"] == made[-1]
        if r["op"] == "close":
            closed.add(r["h"])
    live = sorted(set(made) - closed)  # and one of every live handle at the end
    assert live and sorted(r["h"] for r in recs[-len(live):]) == live
    assert all(r["op"] == "audit" for r in recs[-len(live):])
    for r in recs:  # a closed handle is used once more, and refused
        if r["op"] == "close":
            nxt = recs[r["i"] + 1]
            assert nxt["op"] == "refused" and nxt["why"] == "closed" and nxt["h"] == r["h"] and nxt["expect"]["code"] == -1


def test_the_set_has_every_refusal_scalar_kind_and_class():
    recs = [r for s in L.SEEDS for r in _sequence(s)[0]]
    assert {r["why"] for r in recs if r["op"] == "refused"} == set(L.REFUSALS)
    msm_kinds = {L.scalar_kind(s) for r in recs if r["op"] in ("msm", "subset") for s in _operands(r)}
    assert msm_kinds == set(L.SCALAR_KINDS)
    classes = collections.Counter(c for r in recs for c in r["classes"])
    assert all(classes[c] >= 2 for c in L.CLASSES), classes
    for sub in ("T5:same", "T5:other", "T8:point", "T8:msm", "T9:dense>run", "T9:run>dense"):
        assert classes[sub] >= 1, sub
    assert {r["fn"] for r in recs if r["op"] == "fr"} == set(L.FR_FNS)
    assert any(r.get("out") for r in recs if r["op"] == "fr")  # in place
    assert {r["form"] for r in recs if r["op"] == "fr" and "form" in r} == {"wire", "fr_mont"}
    assert {r["via"] for r in recs if r["op"] == "chain"} == {"msm", "scale", "table"}
    assert {r["how"] for r in recs if r["op"] == "create"} == {"wire", "device", "x"}
    assert {r["levels"] for r in recs if r["op"] == "create"} == {0, 1, 2}
    assert {r["entry"] for r in recs if r["op"] == "msm"} == set(L.MSM_ENTRIES)
    assert {r["entry"] for r in recs if r["op"] == "subset"} == set(L.SUBSET_ENTRIES)
    assert {r["window"] for r in recs if r["op"] == "msm"} == set(L.WINDOWS)
    subsets = [r for r in recs if r["op"] == "subset"]
    assert any(r["idx"] for r in subsets) and any(not r["idx"] for r in subsets)
    assert any(r["idx"] and r["m"] > r["idx"][0]["n"] for r in subsets) and any(r["m"] == 1 for r in subsets)
    assert {r["kind"] for r in recs if r.get("act") == "create"} == {"fixed", "vector"}
    sizes = {int(r["plan"].split("|")[1]) for r in recs if r["op"] == "msm"}  # the launch's terms
    assert {4097, 16385, L.DENSE_N} <= sizes


def test_full_wire_scalars_reach_past_r():
    v = L.scalar_values({"kind": "full", "seed": 3, "m": 50})
    assert sum(x >= R for x in v) >= 10 and (1 << 256) - 1 in v
    for t, e in L.NATIVE_BITS.items():
        if t[0] == "i":
            assert -(1 << (e - 1)) in L.scalar_values({"kind": "native", "type": t, "seed": 1, "m": 9})
    ks = L.ks_of(["list", 5, 9])
    assert {0, 1, R - 1} <= set(ks)


def test_dense_labels_are_the_plans():
    import msm_amd as M

    assert M._test_dense_plan(L.DENSE_N, 1, False, 8, 0)["dense"] == 1
    assert M._test_dense_plan(max(L.MSM_SIZES), 1, False, 8, 0)["dense"] == 0  # the next size down is not
    for s in L.SEEDS:
        for r in _sequence(s)[0]:
            if r.get("dense"):
                assert r["grow"][1] == L.DENSE_N and r["window"] is None and L.scalar_kind(r["sc"][0]) in ("narrow8", "u8")


def test_the_same_seed_gives_the_same_sequence():
    assert L.generate(L.SEEDS[0], L.STEPS) == L.generate(L.SEEDS[0], L.STEPS)
    assert L.generate(L.SEEDS[0], L.STEPS)[0] != L.generate(L.SEEDS[1], L.STEPS)[0]


def test_replay_prints_the_trace():
    r = subprocess.run([sys.executable, L.__file__, "--seed", "7", "--steps", "6"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0 and "oracle multiplications" in r.stdout.splitlines()[-1], r.stderr[-500:]


# ---- the model against the long way ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mul(point, s):
    """s P for any integer: a negative scalar multiplies the negated point by its magnitude."""
    return O.scalar_mul(O.aff_neg(point), -s) if s < 0 else O.scalar_mul(point, s)


def _g(k):
    return _mul(O.G, k % R)


def _sum(points):
    acc = O.IDENTITY
    for p in points:
        acc = O.aff_add(acc, p)
    return acc


class LongWay:
    """The same sequence on actual points: nothing here knows a base's multiplier."""

    def __init__(self):
        self.handles, self.open, self.tables, self.frs = {}, set(), {}, {}

    def scalars(self, sc):
        return [v % R for v in self.frs[sc["ref"]]] if "ref" in sc else L.scalar_values(sc)

    def bases(self, h, first, idx, m):
        pts = self.handles[h]
        return [pts[i] for i in idx] if idx is not None else pts[first:first + m]

    def new(self, rec, pts):
        if rec.get("new"):
            self.handles[rec["new"]] = pts
            self.open.add(rec["new"])
        return pts

    def points(self, rec):
        """The points a record must give (None: it gives none)."""
        op = rec.get("via") or rec["op"]
        if op == "create":
            return self.new(rec, [_mul(O.G, k) for k in L.ks_of(rec["ks"])])
        if op == "audit":
            return self.handles[rec["h"]]
        if op == "msm":
            return [_sum(_mul(p, s) for p, s in zip(self.handles[rec["h"]], self.scalars(sc))) for sc in rec["sc"]]
        if op == "subset":
            out = []
            for j, sc in enumerate(rec["sc"]):
                ix = L.index_values(rec["idx"][j % len(rec["idx"])]) if rec["idx"] else None
                out.append(_sum(_mul(p, s) for p, s in zip(self.bases(rec["h"], rec["first"], ix, rec["m"]), self.scalars(sc))))
            return out
        if op == "scale":
            pts = self.bases(rec["h"], rec["first"], L.index_values(rec["idx"]), rec["m"])
            return self.new(rec, [_mul(p, s) for p, s in zip(pts, self.scalars(rec["sc"]))])
        if op == "combine":
            m = rec["m"]
            pa = self.bases(rec["h"], rec["a_first"], L.index_values(rec["a_idx"]), m)
            pb = self.bases(rec["other"] or rec["h"], rec["b_first"], L.index_values(rec["b_idx"]), m)
            side = lambda mode, sc: [1] * m if mode == "none" else self.scalars(sc) * (m if mode == "bcast" else 1)
            a, b = side(rec["a"], rec.get("a_sc")), side(rec["b"], rec.get("b_sc"))
            out = []
            for i in range(m):
                second = _mul(pb[i], b[i])
                out.append(O.aff_add(_mul(pa[i], a[i]), O.aff_neg(second) if rec["sub"] else second))
            return self.new(rec, out)
        if op == "fold":
            pts = self.handles[rec["h"]]
            h = len(pts) // 2
            low = (lambda p: p) if rec["x_inv"] is None else (lambda p: _mul(p, rec["x_inv"]))
            return self.new(rec, [O.aff_add(low(pts[i]), _mul(pts[i + h], rec["x"])) for i in range(h)])
        if op == "table" and rec["act"] == "create":
            self.tables[rec["new"]] = self.bases(rec["h"], rec["first"], rec["idx"], rec["k"])
            return self.tables[rec["new"]]
        if op == "table" and rec["act"] == "mul":
            tb, sc = self.tables[rec["t"]], self.scalars(rec["sc"])
            k = len(tb)
            return self.new(rec, [_sum(_mul(tb[j], sc[i * k + j]) for j in range(k)) for i in range(rec["m"])])
        return None

    def fr(self, rec):
        """An Fr record with plain integers: the vector's residues after the op."""
        get = lambda o: o if o is None or isinstance(o, int) else list(self.frs[o["ref"]]) if "ref" in o else L.scalar_values(o)
        fn = rec["fn"]
        if fn == "powers":
            out, p = [], 1 if rec["first"] is None else rec["first"] % R
            for _ in range(rec["m"]):
                out.append(p)
                p = p * rec["g"] % R
        else:
            a, b, x, y = (get(rec.get(k)) for k in ("a", "b", "x", "y"))
            if fn == "fold":
                a, b = a[:len(a) // 2], a[len(a) // 2:]
            if fn == "dot":
                total = 0
                for i in range(len(a)):
                    total += a[i] * b[i] if b is not None else a[i]
                out = [total % R]
            else:
                out = []
                for i in range(len(a)):
                    xi = 1 if x is None else x if isinstance(x, int) else x[0] if len(x) == 1 else x[i]
                    t = xi * a[i]
                    if b is not None:
                        yi = 1 if y is None else y if isinstance(y, int) else y[0] if len(y) == 1 else y[i]
                        t = t - yi * b[i] if rec.get("sub") else t + yi * b[i]
                    out.append(t % R)
        if rec.get("out"):
            whole = self.frs[rec["out"]]
            whole[:len(out)] = out
            out = [v % R for v in whole]
        elif rec["where"] == "device" and fn != "dot":
            self.frs[rec["new"]] = list(out)
        return out

    def differs(self, rec, expect):
        """Whether the model's expectation of this record is not what the long way gives."""
        if rec["op"] == "close":
            self.open.discard(rec["h"])
            return expect["open"] != sorted(self.open)
        if rec["op"] == "refused":
            return expect != {"type": "error", "code": "ValueError" if rec["why"] == "too_few" else -1}
        if rec["op"] == "fr":
            return expect["values"] != self.fr(rec) or expect["form"] != rec["out_form"]
        pts = self.points(rec)
        if pts is None:
            if rec.get("act") == "close":
                del self.tables[rec["t"]]
            return False
        claimed = expect["values"] if expect["type"] == "msm" else L.ks_of(expect["ks"])
        return [_g(v) for v in claimed] != pts


def _first_difference(recs, flip_at=None):
    """Replay the records through a fresh model (one op's sign flipped) and the long way side by side."""
    model, long_way = L.Model(), LongWay()
    for i, rec in enumerate(recs):
        if long_way.differs(rec, model.apply(rec, flip=i == flip_at)):
            return i
    return None


@functools.lru_cache(maxsize=None)
def _short(seed):
    recs, _ = L.generate(seed, 12, small=True)
    assert max(len(L.ks_of(r["expect"]["ks"])) for r in recs if r["expect"]["type"] == "handle") <= 8
    return recs


@pytest.mark.parametrize("seed", SHORT)
def test_model_agrees_with_the_long_way(seed):
    recs = _short(seed)
    assert _first_difference(recs) is None
    model = L.Model()
    for rec in recs:  # and the generator stored what the model says
        assert model.apply(rec) == rec["expect"], rec["i"]


def test_short_sequences_hold_every_op_kind():
    assert {r["op"] for s in SHORT for r in _short(s)} == set(L.OP_KINDS)


@pytest.mark.parametrize("kind", L.OP_KINDS)
def test_a_flipped_sign_is_seen_at_its_op(kind):
    seen = 0
    for seed in SHORT:
        recs = _short(seed)
        for i, rec in enumerate(recs):
            if rec["op"] != kind:
                continue
            at = _first_difference(recs, flip_at=i)
            assert at in (i, None), (seed, i, at)  # never anywhere else: None only where the op takes in no non-zero value
            seen += at == i
    assert seen, kind
