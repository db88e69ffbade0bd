"""Lifetime sweep on the GPU: the seeded op sequences of tests/_lifetime_model.py run on one library context,
every step's result bit-exact against the model's integers ((value mod r) G from the oracle, raw words for Fr).

The sequences interleave what a prover interleaves on one slot -- creations, MSMs of every scalar kind,
subsets, per-point scales and combinations, folds, tables, Fr vectors, chains that hand a device vector from
one call to the next unread, closes and refused calls -- so a word one path leaves behind, a graph replayed
with the wrong dimension, a buffer sized by the previous shape or an error bit that outlives its call shows
as a wrong point.  The seeds run in one process, each on the context the previous ones left, on purpose.

MSM_LIFETIME_SEED / MSM_LIFETIME_STEPS run another or a longer sequence;
python tests/_lifetime_model.py --seed S prints a sequence with its expected integers.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import msm_amd as M
import _lifetime_model as L
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [int(os.environ["MSM_LIFETIME_SEED"])] if os.environ.get("MSM_LIFETIME_SEED") else list(L.SEEDS)
STEPS = int(os.environ.get("MSM_LIFETIME_STEPS", L.STEPS))
R = L.R

_POINTS = {0: (0, 1)}


def _pt(k):
    k %= R
    if k not in _POINTS:
        _POINTS[k] = O.scalar_mul(O.G, k)
    return _POINTS[k]


def _wire(ks):
    """Wire records of the points k_i G; a progression comes from the C oracle's generator."""
    if L.is_spec(ks) and ks[0] == "prog":
        return O.gen_points(ks[3], k0=ks[1], step=ks[2])
    return O.affine_to_wire([_pt(k) for k in L.ks_of(ks)])


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.uint8 if a.itemsize < 4 else np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _enc_fr(vals, form):
    """Fr memory: wire holds the integer itself (big-endian words), fr_mont v 2^256 mod r (little-endian)."""
    if form == "wire":
        return np.ascontiguousarray(M.scalars_to_wire([int(v) for v in vals])).reshape(-1, 8)
    return M.scalars_to_wide([int(v) % R for v in vals], "fr_mont").view(np.uint32).reshape(-1, 8)


def _enc_sc(spec):
    """A scalar vector's host array and the keywords that declare its format."""
    vals, kind = L.scalar_values(spec), spec["kind"]
    if kind == "full":
        return np.ascontiguousarray(M.scalars_to_wire(vals)), {}
    if kind == "narrow":
        return np.ascontiguousarray(M.scalars_to_wire(vals, scalar_bits=spec["bits"])), {"scalar_bits": spec["bits"]}
    if kind == "native":
        return M.scalars_to_native(vals, spec["type"]), {"scalar_type": spec["type"]}
    return M.scalars_to_wide(vals, spec["type"]), {"scalar_type": spec["type"]}


def _idx(spec):
    return None if spec is None else np.asarray(spec if isinstance(spec, list) else L.index_values(spec), dtype=np.uint32)


class Runner:
    """The library side of a sequence.  build(rec) makes every upload a record needs and returns its call;
    a chain's consumer is built before its producer runs, so nothing synchronises between the two."""

    def __init__(self):
        self.handles, self.tables, self.frs, self.n = {}, {}, {}, {}

    # -- operands --
    def scalars(self, sc, device):
        """(operand, keywords): a live device vector, or a fresh one."""
        if "ref" in sc:
            if sc.get("mont"):  # Montgomery memory as the wide type reads it: [n, 4] 64-bit
                import torch

                return (lambda: self.frs[sc["ref"]].view(torch.int64)), {"scalar_type": "fr_mont"}
            return (lambda: self.frs[sc["ref"]]), {}
        arr, kw = _enc_sc(sc)
        if device:
            arr = _dev(arr)
        return (lambda: arr), kw

    def fr_operand(self, o, form, device):
        if o is None or isinstance(o, int):
            return lambda: o
        if "ref" in o:
            return lambda: self.frs[o["ref"]]
        arr = _enc_fr(L.scalar_values(o), form)
        if device:
            arr = _dev(arr)
        return lambda: arr

    def made(self, rec, handle):
        self.handles[rec["new"]] = handle
        self.n[rec["new"]] = handle.info["n"]
        return handle

    # -- one builder per op --
    def build(self, rec):
        return getattr(self, "_" + rec["op"])(rec)

    def _create(self, rec):
        wire, lv = _wire(rec["ks"]), rec["levels"]
        n = wire.shape[0]
        if rec["how"] == "wire":
            return lambda: self.made(rec, M.Bases.from_wire(wire, levels=lv))
        if rec["how"] == "device":
            d = _dev(wire)
            return lambda: self.made(rec, M.Bases.from_device(d, n, levels=lv))
        xs = np.ascontiguousarray(wire[:, :8])
        return lambda: self.made(rec, M.Bases.from_x(xs, form="subgroup", levels=lv))

    def _close(self, rec):
        return lambda: self.handles[rec["h"]].close()

    def _audit(self, rec):
        return lambda: self.handles[rec["h"]].points()

    def _msm(self, rec):
        h, entry = self.handles[rec["h"]], rec["entry"]
        dev = entry.endswith("device")
        ops = [self.scalars(sc, dev) for sc in rec["sc"]]
        kw = dict(ops[0][1], window_size=rec["window"], run_length=rec["run_length"])
        if "many" in entry:
            return lambda: [tuple(_xy(r)) for r in getattr(h, entry)([o[0]() for o in ops], **kw)]
        return lambda: [getattr(h, entry)(ops[0][0](), **kw)]

    def _subset(self, rec):
        h, entry, m = self.handles[rec["h"]], rec["entry"], rec["m"]
        dev = entry.endswith("device")
        ops = [self.scalars(sc, dev) for sc in rec["sc"]]
        kw = dict(ops[0][1], window_size=rec["window"], run_length=rec["run_length"], first=rec["first"])
        if dev or kw.get("scalar_type") == "bit":
            kw["m"] = m
        idx = [_dev(_idx(s)) if dev else _idx(s) for s in rec["idx"]] if rec["idx"] else None
        if "many" in entry:
            if idx:
                kw["indices"] = idx if len(idx) > 1 or len(ops) == 1 else idx[0]
            return lambda: [tuple(_xy(r)) for r in getattr(h, entry)([o[0]() for o in ops], **kw)]
        if idx:
            kw["indices"] = idx[0]
        return lambda: [getattr(h, entry)(ops[0][0](), **kw)]

    def _out(self, m):
        import torch

        return torch.zeros((m, 32), dtype=torch.int32, device="cuda")

    def _scale(self, rec):
        h, entry, m = self.handles[rec["h"]], rec["entry"], rec["m"]
        dev = entry.endswith("device")
        sc, kw = self.scalars(rec["sc"], dev)
        kw = dict(kw, first=rec["first"])
        if rec["idx"]:
            kw["indices"] = _dev(_idx(rec["idx"])) if dev else _idx(rec["idx"])
        if entry == "scale":
            return lambda: h.scale(sc(), **kw)
        if entry == "scaled":
            return lambda: self.made(rec, h.scaled(sc(), levels=rec["levels"], **kw))
        if entry == "scaled_device":
            return lambda: self.made(rec, h.scaled_device(sc(), m=m, levels=rec["levels"], **kw))
        out = self._out(m)
        return lambda: (h.scale_device(sc(), out, m=m, **kw), out)[1]

    def _combine(self, rec):
        h, entry, m = self.handles[rec["h"]], rec["entry"], rec["m"]
        dev = entry.endswith("device")
        kw = {"other": self.handles[rec["other"]] if rec["other"] else None, "m": m, "sub": rec["sub"],
              "a_first": rec["a_first"], "b_first": rec["b_first"]}
        for side in "ab":
            spec = rec.get(side + "_sc")
            if spec:
                vals = L.scalar_values(spec)
                bits = spec.get("bits")
                kw["scalar_bits"] = bits
                if dev:
                    kw[side] = _dev(np.ascontiguousarray(M.scalars_to_wire(vals, bits)))
                    kw[side + "_broadcast"] = rec[side] == "bcast"
                else:
                    kw[side] = vals[0] if rec[side] == "bcast" else vals
            ix = rec.get(side + "_idx")
            if ix:
                kw[side + "_indices"] = _dev(_idx(ix)) if dev else _idx(ix)
        if entry == "combine":
            return lambda: h.combine(**kw)
        if entry.startswith("combined"):
            return lambda: self.made(rec, getattr(h, entry)(levels=rec["levels"], **kw))
        out = self._out(m)
        return lambda: (h.combine_device(out, **kw), out)[1]

    def _fold(self, rec):
        return lambda: self.made(rec, self.handles[rec["h"]].fold(rec["x"], rec["x_inv"], levels=rec["levels"]))

    def _table(self, rec):
        if rec["act"] == "close":
            return lambda: self.tables.pop(rec["t"]).close()
        if rec["act"] == "create":
            h = self.handles[rec["h"]]
            kw = {"indices": _idx(rec["idx"])} if rec["idx"] is not None else {"first": rec["first"], "count": rec["k"]}
            make = h.fixed_table if rec["kind"] == "fixed" else h.vector_table
            return lambda: self.tables.__setitem__(rec["new"], make(**kw))
        t, entry, m = self.tables[rec["t"]], rec["entry"], rec["m"]
        dev = entry.endswith("device")
        sc, kw = self.scalars(rec["sc"], dev)
        if entry == "mul":
            return lambda: t.mul(sc(), **kw)
        if entry == "mul_bases":
            return lambda: self.made(rec, t.mul_bases(sc(), levels=rec["levels"], **kw))
        if entry == "mul_bases_device":
            return lambda: self.made(rec, t.mul_bases_device(sc(), m, levels=rec["levels"], **kw))
        out = self._out(m)
        return lambda: (t.mul_device(sc(), out, m=m, **kw), out)[1]

    def _chain(self, rec):
        return getattr(self, "_" + rec["via"])(rec)

    def _fr(self, rec):
        fn, dev, fo = rec["fn"], rec["where"] == "device", rec["out_form"]
        if fn == "powers":
            call = lambda: M.fr_powers(rec["g"], rec["m"], first=rec["first"], out_form=fo, device=0 if dev else None)
        else:
            form = rec["form"]
            a, b, x, y = (self.fr_operand(rec.get(k), form, dev) for k in ("a", "b", "x", "y"))
            kw = {"form": form, "out_form": fo}
            if fn == "dot":
                return lambda: M.fr_dot(a(), b(), **kw).reshape(1, 8)
            if fn == "fold":
                half = lambda: self.frs[rec["out"]][:rec["m"]] if rec.get("out") else None
                call = lambda: M.fr_fold(a(), x(), y(), out=half(), **kw)
            elif fn == "mul":
                call = lambda: M.fr_mul(a(), x(), out=self.frs.get(rec.get("out")), **kw)
            elif fn == "convert":
                call = lambda: M.fr_convert(a(), out=self.frs.get(rec.get("out")), **kw)
            else:
                call = lambda: M.fr_combine(a(), b(), x=x(), y=y(), sub=bool(rec.get("sub")),
                                            out=self.frs.get(rec.get("out")), **kw)
        if not dev:
            return call
        if rec.get("out"):
            return lambda: (call(), self.frs[rec["out"]])[1]
        return lambda: self.frs.__setitem__(rec["new"], call()) or self.frs[rec["new"]]

    def _refused(self, rec):
        import torch

        why, entry = rec["why"], rec["entry"]
        h = self.handles.get(rec.get("h"))
        if why == "closed":
            n = self.n[rec["h"]]
            sc = M.gen_scalars(n, seed=5)
            d_sc = _dev(sc)
            return {"compute": lambda: h.compute(sc), "compute_device": lambda: h.compute_device(d_sc),
                    "compute_subset": lambda: h.compute_subset(sc), "scale": lambda: h.scale(sc),
                    "info": lambda: h.info}[entry]
        if why == "stray_bit":
            arr, kw = _enc_sc(rec["sc"])
            arr[rec["bad_at"], 0] |= 2  # bit 33 of a 33-bit scalar
            v = _dev(arr) if entry.endswith("device") else arr
            return lambda: getattr(h, entry)([v] if "many" in entry else v, **kw)
        if why == "device_index":
            arr, kw = _enc_sc(rec["sc"])
            idx = _idx(rec["idx"])
            idx[rec["bad_at"]] = rec["bad"]
            d_sc, d_idx = _dev(arr), _dev(idx)
            return lambda: h.compute_subset_device(d_sc, indices=d_idx, m=rec["sc"]["m"])
        if why == "mont_ge_r":
            arr = _enc_fr(L.scalar_values(rec["sc"]), "fr_mont")
            arr[rec["bad_at"]] = np.frombuffer(int(rec["bad"]).to_bytes(32, "little"), dtype="<u4")
            d = _dev(arr)
            if entry == "compute_device":
                return lambda: h.compute_device(d.view(torch.int64), scalar_type="fr_mont")
            if entry == "fr_dot_device":
                return lambda: M.fr_dot(d, form="fr_mont")
            return lambda: M.fr_convert(d, "fr_mont", "wire")
        if why == "too_few":
            arr, kw = _enc_sc(rec["sc"])
            return lambda: h.compute(arr) if entry == "compute" else h.compute_many([arr])
        m = rec["m"]
        odd = torch.zeros((m + 1, 8), dtype=torch.int32, device="cuda").view(-1)[1:1 + 8 * m]  # 4 bytes off
        return {"fr_combine_device": lambda: M.fr_combine(odd), "fr_dot_device": lambda: M.fr_dot(odd),
                "fr_powers_device": lambda: M.fr_powers(3, m, out=odd)}[entry]

    # -- checks --
    def check(self, rec, got):
        """None, or what differs."""
        e = rec["expect"]
        if e["type"] == "error":
            return None if got == ("raised", e["code"]) else f"expected MsmError {e['code']}, got {got!r}"
        if isinstance(got, tuple) and got and got[0] == "raised":
            return f"raised {got[1]!r}"
        if e["type"] == "msm":
            exp = [_pt(v) for v in e["values"]]
            return None if [tuple(g) for g in got] == exp else f"msm results {got!r}, expected {exp!r}"
        if e["type"] == "points":
            got = got if isinstance(got, np.ndarray) else _host(got)
            exp = _wire(e["ks"])
            if got.shape != exp.shape:
                return f"points of shape {got.shape}, expected {exp.shape}"
            bad = np.nonzero((got != exp).any(axis=1))[0]
            return None if not bad.size else f"{bad.size} of {exp.shape[0]} points differ, the first at {int(bad[0])}"
        if e["type"] == "handle":
            n = self.handles[e["name"]].info["n"]
            return None if n == len(L.ks_of(e["ks"])) else f"a handle of {n} points"
        if e["type"] == "fr":
            got = got if isinstance(got, np.ndarray) else _host(got)
            exp = _enc_fr(e["values"], e["form"])
            if got.shape != exp.shape:
                return f"an Fr vector of shape {got.shape}, expected {exp.shape}"
            bad = np.nonzero((got != exp).any(axis=1))[0]
            return None if not bad.size else f"{bad.size} of {exp.shape[0]} elements differ, the first at {int(bad[0])}"
        return None

    def close(self):
        for t in self.tables.values():
            t.close()
        for h in self.handles.values():
            h.close()


def _xy(row):
    return O.be_words_to_int(row[:8]), O.be_words_to_int(row[8:16])


def _call(call):
    try:
        return call()
    except M.MsmError as e:
        return ("raised", e.code)
    except ValueError:
        return ("raised", "ValueError")


def run_sequence(seed, steps, after_step=None):
    """Run one sequence on the library context as it stands: None, or (record index, what differs)."""
    import torch

    recs, _ = L.generate(seed, steps)
    run = Runner()
    calls = [None] * len(recs)
    try:
        deferred = None
        for i, rec in enumerate(recs):
            calls[i] = calls[i] or run.build(rec)
            if rec.get("defer") and i + 1 < len(recs):  # the consumer's own uploads come before the producer runs
                calls[i + 1] = run.build(recs[i + 1])
                torch.cuda.synchronize()
            got = _call(calls[i])
            calls[i] = None
            if rec.get("defer") and i + 1 < len(recs) and not (isinstance(got, tuple) and got[0] == "raised"):
                deferred = (i, rec, got)  # read back only after the consumer has run
                continue
            for j, r, g in ((i, rec, got),) + ((deferred,) if deferred else ()):
                diff = run.check(r, g)
                if diff:
                    return j, diff
                if after_step:
                    after_step(j, r)
            deferred = None
        return None
    finally:
        run.close()


def _message(seed, steps, failure):
    i, diff = failure
    recs, _ = L.generate(seed, steps)
    before = "\n".join(f"  {r['i']}: {L.show(r)}" for r in recs[max(0, i - 3):i])
    return (f"seed {seed}, step {i} ({' '.join(recs[i]['classes']) or 'no class'}): {diff}\n  {L.show(recs[i])}\n"
            f"the three records before it:\n{before}\nreplay: python tests/_lifetime_model.py --seed {seed} --steps {steps}")


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence(seed):
    t0 = time.time()
    failure = run_sequence(seed, STEPS)
    print(f"lifetime seed {seed}: {time.time() - t0:.2f} s")
    assert failure is None, _message(seed, STEPS, failure)


def test_sequence_guarded():
    """One sequence with guard bands round every device buffer: no step, a refused one included, writes past
    its buffers as they have grown so far."""
    lib = M.load()
    seed = SEEDS[0]
    hits = []

    def after_step(i, rec):
        found = M._test_guard_check()
        if found and not hits:
            hits.append((i, found))

    try:
        lib.msm_shutdown()
        M._test_guard(True)
        failure = run_sequence(seed, STEPS, after_step)
        assert failure is None, _message(seed, STEPS, failure)
        assert not hits, _message(seed, STEPS, (hits[0][0], f"guard bands written: {hits[0][1]}"))
        assert M._test_guard_check() == []
    finally:
        lib.msm_shutdown()
        M._test_guard(False)


CHILD = r"""
import json, sys
sys.path[:0] = [{root!r}, {root!r} + "/webgpu-msm_amd", {root!r} + "/tests"]
import test_gpu_lifetime as T
failure = T.run_sequence({seed}, {steps})
print(json.dumps(None if failure is None else [failure[0], failure[1]]))
"""


@pytest.mark.parametrize("env", [
    {"MSM_NO_GRAPH": "1"},                     # eager launches instead of captured graphs
    {"MSM_SLOTS": "1", "MSM_BATCH": "1"},      # one slot, one MSM per launch
], ids=["eager", "one_slot"])
def test_sequence_other_launch_paths(env):
    seed = SEEDS[-1]
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, seed=seed, steps=STEPS)], env=e,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    failure = json.loads(r.stdout.strip().splitlines()[-1])
    assert failure is None, (env, _message(seed, STEPS, tuple(failure)))
