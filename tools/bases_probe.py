"""Resident prepared bases (msm_amd.Bases) against the entries that take the points on every call:
the sweep behind the auto table in host_plan.h (BASES_AUTO) and DESIGN.md §9.

    python tools/bases_probe.py [--sizes 16,18,20] [--levels 1,2,4] [--count 20] [--out FILE]

Without --n the sizes run one after the other, each as a child process under its own `timeout`;
the sweep stops at the first child that fails (nothing more is started on the GPU after a fault
or a time limit).  With --n one size runs in this process and prints / appends JSON lines:

  {"entry": "msm_compute_shared_device", ...}  pipelined ms per MSM, base vector prepared per call
  {"entry": "msm_compute", ...}                one awaited MSM from host arrays (points + scalars)
  {"entry": "bases", "levels", "c", ...}       handle creation (ms), pipelined ms per MSM over
                                               `count` MSMs (compute_many_device), one awaited MSM
                                               from device scalars and from host scalars

With --subset the pass is the subset sweep of DESIGN.md §9 instead (msm_bases_compute_subset*): on
one handle of n points (--sizes, default 2^20), at levels 1 and at the handle's auto levels where
they differ, for m in --subset-sizes (log2; default 12,16,18,20) one line per way of computing an
m-term MSM:

  {"entry": "subset", "form": "padded", ...}        msm_bases_compute*, the scalar vector zero-padded to n
  {"entry": "subset", "form": "own_handle", ...}    a handle built from exactly those m points (the floor)
  {"entry": "subset", "form": "range", "first"}     the range form at first = 0 and at first = n - m
  {"entry": "subset", "form": "indexed", "order"}   the indexed form, sorted-unique and random indices

each with the awaited call from host arrays and from device-resident ones and the pipelined call
over `count` MSMs, both ways, plus the per-phase device times of one profiled awaited call
(msm_set_profiling(1)).

With --narrow the pass is the narrow-scalar sweep of DESIGN.md §9 (MSM_FLAG_SCALAR_BITS): on a
levels-1 handle of each size, for b in --narrow-bits (default 8,16,32,64,128,253) one line per way of
computing the MSM of n random b-bit scalars:

  {"entry": "narrow", "form": "extended", ...}   the existing entry on the scalars zero-extended to 8 words
  {"entry": "narrow", "form": "narrow", "c": 0}  Bases.compute*(scalar_bits=b) at the auto width
  {"entry": "narrow", "form": "narrow", "c": c}  the same at c in --narrow-widths (13..17 and 19)

with the same four timings and the per-phase times of one profiled awaited call.

With --dense the pass is the dense-bucket sweep of DESIGN.md §9 (the narrow launches whose buckets
hold DENSE_MIN entries or more, host_plan.h): the narrow pass at the auto width for b = 1, 4, 8, 12,
for b = 16 at the explicit width 16, and (at 2^20) for all-equal bytes, once as the library plans
it and once with the path turned off (MSM_DENSE_MIN, read once per process: each way is a child
process of its own; every line carries "dense_min", the variable's value, and "dense" / "E", the
lone launch's plan); then the threshold rows with the path forced on (MSM_DENSE_MIN=1) and off:
b = 8 at 2^13..2^16, b = 12 at 2^17..2^19, and b = 13 at 2^20.

With --native the pass is the native-type sweep of DESIGN.md §9 (MSM_FLAG_SCALAR_TYPE): on a levels-1
handle of each size, for the types bit, u8, i8, u16, i16, i32, i64 and u64, one line per way of
computing the MSM of n random values of the type:

  {"entry": "native", "type", "form": "narrow"}  (a) the existing narrow call on the magnitudes as big-endian
                                                 words (the points of negative values negated in a handle of
                                                 its own), with "convert_ms": the numpy conversion its
                                                 caller pays (magnitudes to [n, ceil(b / 32)] big-endian u32)
  {"entry": "native", "type", "form": "typed"}   (b) Bases.compute*(scalar_type=type) on the array as it is

with the narrow sweep's four timings and the per-phase times of one profiled awaited call.

With --wide the pass is the wide-type sweep of DESIGN.md §9 (MSM_FLAG_SCALAR_FIELD): on a levels-1 handle
of each size, for the types u128, i128, u256 and fr_mont, the MSM of n random values of the type (u256:
the full 256 bits; fr_mont: random a < r, the scalar being a 2^-256 mod r):

  {"entry": "wide", "type", "form": "words", "repeat": 0 | 1}
        (a) the existing call on the same values converted beforehand -- scalar_bits = 128 on big-endian
        words for the 128-bit types (i128: the magnitudes, the points of negative values negated in a handle
        of its own), the 8-word call for the 256-bit ones -- measured before and after (b): the two rows'
        spread is the run-to-run margin.  "convert_ms" is what the conversion costs THIS caller, in numpy
        (limb reversal, magnitudes) and, for fr_mont, in Python integers (one modular multiplication per
        element): informational, not a C baseline -- an arkworks prover's into_bigint() is a compiled loop
  {"entry": "wide", "type", "form": "wide"}   (b) Bases.compute*(scalar_type=type) on the array as it is

with the narrow sweep's four timings and the per-phase times of one profiled awaited call.

With --compressed the pass is the compressed-creation sweep of DESIGN.md §9 (MSM_POINTS_X_*): at each size,
for both forms, one line

  {"entry": "compressed", "form", "from_x_ms", "from_x_device_ms", "decompress_device_ms",
   "from_wire_ms", "from_device_ms", ...}

with the creation of a levels-1 handle from host x-coordinates (32 n bytes up, then k_decompress_x and the
preparation) and from device-resident ones, the awaited device-to-device msm_decompress_points_device on its
own (the kernel, one launch and the read-back of its error word), and -- the comparison that matters,
same points, same run -- the wire creations from host records (128 n bytes up) and from device-resident
ones.  Each creation is timed with its msm_bases_destroy; one MSM on the compressed handle is checked
against the closed form, and the decompressed records against the generator's.

With --scale the pass is the per-point scalar-multiple sweep of DESIGN.md §9 (msm_bases_scale*): for m in
--scale-sizes (log2; default 12..20) on a levels-1 handle of m points, and for b in --scale-bits (default
64,128,253,256), one line per form

  {"entry": "scale", "m", "bits", "form": "device_range" | "device_indexed" | "host", "ms", "ns_per_point"}

the awaited device-to-device call over the range, over a random index list, and the host entry (scalars
up, wire records back); six sampled points of each are checked against the oracle's scalar multiplication.
Then, in the same process, what the library offered for the same result before: m one-term MSMs through
compute_subset_many_device, at m in --scale-msm-sizes (default 2^10 and 2^12), as a row of its own
("form": "one_term_msms"), checked against the scale call.  All sizes run in one child process.

With --fixed the pass is the fixed-base table sweep of DESIGN.md §9 (msm_fixed_*): for b in --fixed-bits
(default 64,128,253,256), first the baseline in the same process on the same scalars -- Bases.scale_device
with an all-zero index vector, m in --fixed-sizes (log2; default 12..20), "form": "scale_zero_indices" --
then for w in --fixed-widths (default 6,8,10,12) and k in --fixed-bases (default 1,2) the table's build
("form": "table_build", timed with its destroy) and per m

  {"entry": "fixed", "m", "bits", "w", "k", "form": "device" | "host", "ms", "ns_per_point", "ratio_to_scale"}

the awaited device-to-device call and the host entry (scalars up, wire records back); four sampled rows are
checked against the oracle's scalar multiplication and the host result against the device one.
ratio_to_scale (k = 1, device) is the baseline's median over this row's.

With --combine the pass is the pairwise-combination sweep of DESIGN.md §9 (msm_bases_combine*), in one
process: for m in --combine-sizes (log2; default 12,16,18,20) the A_i are bases [0, m) and the B_i bases
[m, 2 m) of one handle, and for b in --combine-bits (default 64,128,256), on the same random scalars,

  {"entry": "combine", "m", "bits", "form", "ms", "ns_per_point", "runs_ms", "ratio", "spread"}

with "form" one of "scale_once" (Bases.scale_device on the B side: the one-scalar form's reference),
"scale_twice" (both sides, one call after the other: the joint form's), "one" (A_i + b_i B_i), "joint"
(a_i A_i + b_i B_i), "one_broadcast" and "joint_broadcast" (one scalar per side), and per m a "sum" row
(A_i + B_i, with "bytes" and "gb_per_s").  Every call is the awaited device-to-device entry; "ratio" is the
row's median over its reference's (one*: scale_once, joint*: scale_twice) and "spread" the runs' max - min.
Sampled rows are checked against the oracle.

With --vector the pass is the vector-table sweep of DESIGN.md §9 (msm_fixed_create_vector), in one process:
for every shape k:log2(m) in --vector-shapes (default 16:16,64:14,256:12,1024:10,4096:8) and b in
--vector-bits (default 256,64), on the same random scalars, first today's route -- m subset MSMs of the k
bases through compute_subset_many_device ("form": "subset_many", and at b < 256 its scalar_bits form
"subset_many_narrow"; the faster one is the baseline) -- then for w in --vector-widths (default
2,4,6,8,10,12; 0 is the library's choice) whose table fits 256 MiB the build ("form": "table_build", with the rule's "auto_w") and

  {"entry": "vector", "k", "m", "bits", "w", "auto_w", "form": "table", "forced_G", "G", "P", "passes", "slab_rows", "ms",
   "us_per_row", "runs_ms", "baseline", "baseline_ms", "ratio_to_baseline", "table_bytes", "correct"}

the awaited device-to-device call at the plan's own G ("forced_G": 0) and, at w = --vector-group-w (default
6), at every G in --vector-groups (default 1,2,4,8).  Every row's records are checked against the
baseline's points.

With --fr the scalar-field vector entries (msm_fr_*) are swept instead, every row in this one process: for every
n = 2^lg of --fr-sizes (default 16..22) one line per operation

  {"entry": "fr", "op", "n", "ms", "ns_per_elem", "runs_ms", "bytes", "gb_per_s", "torch_op", "torch_ms",
   "ratio_to_torch", "correct"}

"fold" (n elements in, n / 2 out, both multipliers broadcast), "fold_in_place", "hadamard", "scale", "add",
"convert" (fr_mont to wire), "powers" and "dot", device tensors in and out, beside a torch elementwise operation
on int32 tensors that moves the same bytes (the memory-rate yardstick; "torch_op" names it), and sampled elements
checked against Python integers.  At --fr-compare (default 20, 0: skip) two more lines: {"entry": "fr", "op":
"fold_vs_bases_fold", ...} with fr_fold's time beside Bases.fold's on a handle of as many bases, and {"op":
"srs", ...} with fr_powers + mul_bases_device beside host powers, scalars_to_wire, the upload and mul_bases.

With --frscan the second set of Fr entries (msm_fr_inverse*, msm_fr_scan*, msm_fr_tensor*) is swept, every row in
this one process: for every n = 2^lg of --frscan-sizes (default 16..22) one line per operation

  {"entry": "frscan", "op", "n", "ms", "ns_per_elem", "runs_ms", "fr_mul_ms", "ratio_to_fr_mul", "host_route_ms",
   "host_parts_ms", "correct"}

"inverse", "cumprod", "cumsum" and "tensor" (lg pairs), device tensors in and out, beside fr_mul (a Hadamard
product) on the same vector -- the yardstick for the products per element -- and beside the route a caller had
before: the vector down, Python integers (Montgomery's trick for the inverse), the result up; that route is run
once, its download and decode and its encode and upload shared by the operations ("host_parts_ms" has the three
parts).  Every device result is compared whole with the host route's.

c runs from the unfolded pipelined width to that + 2, capped at 16 (wider windows take the 32-bit
digit codes); --c17 adds c = 17 so that cap can be checked.  Every timed configuration is also
checked against the closed form.  Times are host wall clock around calls that return with the
result on the host; medians over --runs repeats after one warm-up call.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "webgpu-msm_amd"), os.path.join(ROOT, "tests")]


def timed(fn, runs):
    fn()  # warm-up: graph capture, allocations
    ts = []
    res = None
    for _ in range(runs):
        t0 = time.perf_counter()
        res = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), [round(t, 4) for t in ts], res


def one_size(a):
    import numpy as np
    import torch

    import msm_amd as M
    from _closed_form import as_xy, closed_form

    n, count = a.n, a.count
    lines = []

    def emit(d):
        d = {"n": n, **d}
        lines.append(d)
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()

    pts = M.gen_points(n, k0=3, step=5)
    distinct = min(count, 4)  # a few scalar vectors, cycled: the device holds 4, not `count`, of them
    scs = [M.gen_scalars(n, seed=500 + i) for i in range(distinct)]
    exp = [closed_form(3, 5, s) for s in scs]
    d_pts, d_scs = dev(pts), [dev(s) for s in scs]
    many = [d_scs[i % distinct] for i in range(count)]
    many_exp = [exp[i % distinct] for i in range(count)]
    torch.cuda.synchronize()

    def check(rows):
        return [as_xy(r) for r in rows] == many_exp

    # the comparison entries, same run, same box
    ms, runs, res = timed(lambda: M.compute_msm_shared_device(d_pts, many, n), a.runs)
    emit({"entry": "msm_compute_shared_device", "count": count, "ms_per_msm": round(ms / count, 4),
          "runs_ms": runs, "correct": check(res)})
    ms, runs, res = timed(lambda: M.compute_msm_device(d_pts, d_scs[0], n), a.runs)
    emit({"entry": "msm_compute_device", "ms": round(ms, 4), "runs_ms": runs, "correct": res == exp[0]})
    ms, runs, res = timed(lambda: M.compute_msm_wire(pts, scs[0]), a.runs)
    emit({"entry": "msm_compute", "ms": round(ms, 4), "runs_ms": runs, "correct": res == exp[0]})

    c0 = M.launch_plan(n, pipelined=True)["c"]
    widths = [c for c in range(c0, c0 + 3) if c <= 16] + ([17] if a.c17 else [])
    for levels in a.levels:
        for c in widths:
            t0 = time.perf_counter()
            b = M.Bases.from_device(d_pts, n, levels=levels, window_size=c)
            create_ms = (time.perf_counter() - t0) * 1e3
            with b:
                inf = b.info
                row = {"entry": "bases", "levels": levels, "c": c, "windows": inf["windows"] or M.window_count(c),
                       "chunk_bits": inf["chunk_bits"], "bytes": inf["bytes"], "create_ms": round(create_ms, 3)}
                ms, runs, res = timed(lambda: b.compute_many_device(many, window_size=c), a.runs)
                row.update(count=count, pipelined_ms_per_msm=round(ms / count, 4), pipelined_runs_ms=runs)
                ok = check(res)
                ms, runs, res = timed(lambda: b.compute_device(d_scs[0], window_size=c), a.runs)
                row.update(single_device_ms=round(ms, 4), single_device_runs_ms=runs)
                ok = ok and res == exp[0]
                ms, runs, res = timed(lambda: b.compute(scs[0], window_size=c), a.runs)
                row.update(single_host_ms=round(ms, 4), single_host_runs_ms=runs)
                ok = ok and res == exp[0]
                row["correct"] = ok
                emit(row)
            if levels == 1 and c == widths[0]:
                # creation from host arrays (upload + preparation), once per size
                t0 = time.perf_counter()
                with M.Bases.from_wire(pts, levels=1):
                    emit({"entry": "bases_create_host", "levels": 1, "create_ms": round((time.perf_counter() - t0) * 1e3, 3)})
    return 0 if all(d.get("correct", True) for d in lines) else 1


def subset_pass(a):
    import numpy as np
    import torch

    import msm_amd as M
    from _closed_form import as_xy, scalar_dot
    from oracle import oracle as O

    n, count, k0, step = a.n, a.count, 3, 5
    bad = []

    def emit(d):
        d = {"n": n, **d}
        if not d.get("correct", True):
            bad.append(d)
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()

    def closed(idx, sc):
        return O.scalar_mul(O.G, scalar_dot(k0 + step * np.asarray(idx, dtype=np.uint64), sc) % O.R_ORDER)

    phases = ("recode_count", "coarse_scatter", "fine_sort", "accumulate", "bucket_reduce_1", "bucket_reduce_2",
              "device_total")

    def profile(fn):
        M.set_profiling(1)
        try:
            fn()
            p = M.last_profile()
        finally:
            M.set_profiling(0)
        return {k: round(float(p[k]), 4) for k in phases}

    def measure(row, exp, host1, dev1, host_many, dev_many):
        """The four timings of one way of computing the MSM, each checked against the closed form."""
        ok = True
        for key, fn, many in (("single_host", host1, False), ("single_device", dev1, False),
                              ("pipelined_host", host_many, True), ("pipelined_device", dev_many, True)):
            ms, runs, res = timed(fn, a.runs)
            if many:
                row[key + "_ms_per_msm"] = round(ms / count, 4)
                ok = ok and [as_xy(r) for r in res] == [exp] * count
            else:
                row[key + "_ms"] = round(ms, 4)
                ok = ok and res == exp
            row[key + "_runs_ms"] = runs
        row["phases_ms"] = profile(dev1)
        row["correct"] = ok
        emit(row)

    pts = M.gen_points(n, k0=k0, step=step)
    d_pts = dev(pts)
    auto = M.Bases.from_device(d_pts, n)
    auto_levels = auto.info["levels"]
    auto.close()
    rnd = np.random.RandomState(17)
    for levels in sorted({1, auto_levels}):
        with M.Bases.from_device(d_pts, n, levels=levels) as b:
            for lg in a.subset_sizes:
                m = 1 << lg
                if m > n:
                    continue
                sc = M.gen_scalars(m, seed=900 + lg)
                d_sc = dev(sc)
                base = {"entry": "subset", "levels": levels, "m": m, "count": count}
                # (a) today's workaround: the full entry on a scalar vector zero-padded to n
                pad = np.zeros((n, 8), np.uint32)
                pad[:m] = sc
                d_pad = dev(pad)
                measure({**base, "form": "padded"}, closed(np.arange(m), sc),
                        lambda: b.compute(pad), lambda: b.compute_device(d_pad),
                        lambda: b.compute_many([pad] * count), lambda: b.compute_many_device([d_pad] * count))
                del pad, d_pad
                # (b) a handle of exactly those m points: the floor
                with M.Bases.from_device(d_pts, m, levels=levels) as own:
                    measure({**base, "form": "own_handle"}, closed(np.arange(m), sc),
                            lambda: own.compute(sc), lambda: own.compute_device(d_sc),
                            lambda: own.compute_many([sc] * count), lambda: own.compute_many_device([d_sc] * count))
                # (c) the range form
                for first in sorted({0, n - m}):
                    measure({**base, "form": "range", "first": first}, closed(first + np.arange(m), sc),
                            lambda: b.compute_subset(sc, first=first),
                            lambda: b.compute_subset_device(d_sc, first=first),
                            lambda: b.compute_subset_many([sc] * count, first=first),
                            lambda: b.compute_subset_many_device([d_sc] * count, first=first))
                # (d) the indexed form
                for order in ("sorted_unique", "random"):
                    if order == "random":
                        idx = rnd.randint(0, n, size=m).astype(np.uint32)
                    else:
                        idx = np.sort(rnd.permutation(n)[:m]).astype(np.uint32)
                    d_idx = dev(idx)
                    measure({**base, "form": "indexed", "order": order}, closed(idx, sc),
                            lambda: b.compute_subset(sc, indices=idx),
                            lambda: b.compute_subset_device(d_sc, indices=d_idx),
                            lambda: b.compute_subset_many([sc] * count, indices=idx),
                            lambda: b.compute_subset_many_device([d_sc] * count, indices=d_idx))
    return 1 if bad else 0


def narrow_pass(a):
    import numpy as np
    import torch

    import msm_amd as M
    from _closed_form import as_xy, closed_form

    n, count, k0, step = a.n, a.count, 3, 5
    bad = []

    def emit(d):
        d = {"n": n, **d}
        if not d.get("correct", True):
            bad.append(d)
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()

    phases = ("recode_count", "coarse_scatter", "fine_sort", "accumulate", "bucket_reduce_1", "bucket_reduce_2",
              "device_total")

    def profile(fn):
        M.set_profiling(1)
        try:
            fn()
            p = M.last_profile()
        finally:
            M.set_profiling(0)
        return {**{k: round(float(p[k]), 4) for k in phases}, "windows": int(p["windows"]), "c": int(p["window_bits"]),
                "run_length": int(p["run_length"])}

    def measure(row, exp, host1, dev1, host_many, dev_many):
        ok = True
        for key, fn, many in (("single_host", host1, False), ("single_device", dev1, False),
                              ("pipelined_host", host_many, True), ("pipelined_device", dev_many, True)):
            ms, runs, res = timed(fn, a.runs)
            if many:
                row[key + "_ms_per_msm"] = round(ms / count, 4)
                ok = ok and [as_xy(r) for r in res] == [exp] * count
            else:
                row[key + "_ms"] = round(ms, 4)
                ok = ok and res == exp
            row[key + "_runs_ms"] = runs
        row["phases_ms"] = profile(dev1)
        row["correct"] = ok
        emit(row)

    pts = M.gen_points(n, k0=k0, step=step)
    d_pts = dev(pts)
    rnd = np.random.RandomState(29)
    # (bits, widths, scalars): the sweep's uniform scalars at the auto and the explicit widths, then
    # --narrow-extra's b:c rows, then --narrow-equal's all-equal bytes
    cases = [(bits, [0] + list(a.narrow_widths), "uniform") for bits in a.narrow_bits]
    cases += [(bits, [c], "uniform") for bits, c in a.narrow_extra]
    cases += [(8, [0], "equal")] if a.narrow_equal else []
    dense_min = os.environ.get("MSM_DENSE_MIN")
    with M.Bases.from_device(d_pts, n, levels=1) as b:
        for bits, widths, kind in cases:
            words = (bits + 31) // 32
            if kind == "equal":
                sc8 = np.zeros((n, 8), np.uint32)
                sc8[:, 7] = 0xA5
            elif bits == 253:
                sc8 = M.gen_scalars(n, seed=700)  # canonical field elements: below 2^253
            else:
                sc8 = np.zeros((n, 8), np.uint32)
                sc8[:, 8 - words:] = rnd.randint(0, 1 << 32, size=(n, words), dtype=np.uint64).astype(np.uint32)
                if bits % 32:
                    sc8[:, 8 - words] &= (1 << (bits % 32)) - 1
            sc = np.ascontiguousarray(sc8[:, 8 - words:])
            exp = closed_form(k0, step, sc8)
            d_sc8, d_sc = dev(sc8), dev(sc)
            base = {"entry": "narrow", "bits": bits, "words": words, "count": count}
            if kind != "uniform":
                base["scalars"] = kind
            base["dense_min"] = dense_min
            if not a.no_extended:
                measure({**base, "form": "extended"}, exp,
                        lambda: b.compute(sc8), lambda: b.compute_device(d_sc8),
                        lambda: b.compute_many([sc8] * count), lambda: b.compute_many_device([d_sc8] * count))
            for c in widths:
                kw = {"window_size": c or None, "scalar_bits": bits}
                # (a library from before the dense accumulation, loaded for an A/B run, has no such plan)
                plan = (M._test_dense_plan(n, 1, False, bits, c) if hasattr(M.load(), "msm_test_dense_plan")
                        else {"dense": 0, "E": 0})
                measure({**base, "form": "narrow", "c": c, "dense": plan["dense"], "E": plan["E"]}, exp,
                        lambda: b.compute(sc, **kw), lambda: b.compute_device(d_sc, **kw),
                        lambda: b.compute_many([sc] * count, **kw),
                        lambda: b.compute_many_device([d_sc] * count, **kw))
    return 1 if bad else 0


def native_pass(a):
    import numpy as np
    import torch

    import msm_amd as M
    from _closed_form import as_xy, scalar_dot
    from oracle import oracle as O

    n, count, k0, step = a.n, a.count, 3, 5
    bad = []

    def emit(d):
        d = {"n": n, **d}
        if not d.get("correct", True):
            bad.append(d)
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()

    phases = ("recode_count", "coarse_scatter", "fine_sort", "accumulate", "bucket_reduce_1", "bucket_reduce_2",
              "device_total")

    def profile(fn):
        M.set_profiling(1)
        try:
            fn()
            p = M.last_profile()
        finally:
            M.set_profiling(0)
        return {**{k: round(float(p[k]), 4) for k in phases}, "windows": int(p["windows"]), "c": int(p["window_bits"]),
                "run_length": int(p["run_length"])}

    def measure(row, exp, host1, dev1, host_many, dev_many):
        ok = True
        for key, fn, many in (("single_host", host1, False), ("single_device", dev1, False),
                              ("pipelined_host", host_many, True), ("pipelined_device", dev_many, True)):
            ms, runs, res = timed(fn, a.runs)
            if many:
                row[key + "_ms_per_msm"] = round(ms / count, 4)
                ok = ok and [as_xy(r) for r in res] == [exp] * count
            else:
                row[key + "_ms"] = round(ms, 4)
                ok = ok and res == exp
            row[key + "_runs_ms"] = runs
        row["phases_ms"] = profile(dev1)
        row["correct"] = ok
        emit(row)

    def to_words(mag, words):
        """Magnitudes (uint64) as [n, words] big-endian u32: the rewrite the narrow call's caller pays."""
        out = np.empty((n, words), np.uint32)
        out[:, words - 1] = mag & np.uint64(0xffffffff)
        if words == 2:
            out[:, 0] = mag >> np.uint64(32)
        return out

    pts = M.gen_points(n, k0=k0, step=step)
    neg_pts = pts.copy()  # every point negated: x -> -x mod p, t -> -t mod p (multi-word, in numpy)
    pw = np.array(O.int_to_be_words(O.P), dtype=np.int64)
    for j in (0, 2):
        d = pw[None, :] - pts[:, 8 * j:8 * j + 8].astype(np.int64)
        for k in range(7, 0, -1):  # borrows
            borrow = d[:, k] < 0
            d[:, k] += borrow.astype(np.int64) << 32
            d[:, k - 1] -= borrow
        zero = ~pts[:, 8 * j:8 * j + 8].any(axis=1)
        d[zero] = 0
        neg_pts[:, 8 * j:8 * j + 8] = d.astype(np.uint32)
    ks = k0 + step * np.arange(n, dtype=np.uint64)
    rnd = np.random.RandomState(31)
    with M.Bases.from_wire(pts, levels=1) as plain:
        for ty in a.native_types:
            _, dt, e = M.SCALAR_TYPES[ty]
            signed = ty[0] == "i"
            if ty == "bit":
                vals = rnd.randint(0, 2, size=n).astype(np.int64)
                arr = np.packbits(vals.astype(np.uint8), bitorder="little")
            else:
                raw = rnd.randint(0, 1 << 32, size=n, dtype=np.uint64) | rnd.randint(0, 1 << 32, size=n, dtype=np.uint64) << np.uint64(32)
                arr = raw.astype(np.uint64).view(np.uint64).astype(dt) if not signed else raw.view(np.int64).astype(dt)
                vals = arr
            t0 = time.perf_counter()
            isneg = (vals < 0) if signed else np.zeros(n, bool)
            mag = np.where(isneg, (0 - vals.astype(np.int64)).astype(np.uint64) if signed else 0,
                           vals.astype(np.uint64)).astype(np.uint64)
            words = (e + 31) // 32
            sc = to_words(mag, words)
            convert_ms = (time.perf_counter() - t0) * 1e3
            sc8p, sc8n = np.zeros((n, 8), np.uint32), np.zeros((n, 8), np.uint32)
            sc8p[~isneg, 8 - words:] = sc[~isneg]
            sc8n[isneg, 8 - words:] = sc[isneg]
            exp = O.scalar_mul(O.G, (scalar_dot(ks, sc8p) - scalar_dot(ks, sc8n)) % O.R_ORDER)
            base = {"entry": "native", "type": ty, "bits": e, "count": count, "vector_bytes": int(arr.nbytes)}
            d_sc, d_arr = torch.from_numpy(sc.view(np.int32)).cuda(), dev(arr)
            kw = {"scalar_bits": e}
            # (a) the narrow call on the magnitudes, over a handle whose points carry the signs
            with M.Bases.from_wire(np.where(isneg[:, None], neg_pts, pts), levels=1) as signed_bases:
                measure({**base, "form": "narrow", "convert_ms": round(convert_ms, 4)}, exp,
                        lambda: signed_bases.compute(sc, **kw), lambda: signed_bases.compute_device(d_sc, **kw),
                        lambda: signed_bases.compute_many([sc] * count, **kw),
                        lambda: signed_bases.compute_many_device([d_sc] * count, **kw))
            # (b) the typed call on the array as it is
            tk = {"scalar_type": ty}
            measure({**base, "form": "typed"}, exp,
                    lambda: plain.compute(arr, **tk), lambda: plain.compute_device(d_arr, **tk),
                    lambda: plain.compute_many([arr] * count, **tk),
                    lambda: plain.compute_many_device([d_arr] * count, **tk))
    return 1 if bad else 0


def wide_pass(a):
    import numpy as np
    import torch

    import msm_amd as M
    from _closed_form import as_xy, scalar_dot
    from oracle import oracle as O

    n, count, k0, step = a.n, a.count, 3, 5
    R = M.FR_MODULUS
    bad = []

    def emit(d):
        d = {"n": n, **d}
        if not d.get("correct", True):
            bad.append(d)
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    phases = ("recode_count", "coarse_scatter", "fine_sort", "accumulate", "bucket_reduce_1", "bucket_reduce_2",
              "device_total")

    def profile(fn):
        M.set_profiling(1)
        try:
            fn()
            p = M.last_profile()
        finally:
            M.set_profiling(0)
        return {**{k: round(float(p[k]), 4) for k in phases}, "windows": int(p["windows"]), "c": int(p["window_bits"]),
                "run_length": int(p["run_length"])}

    def measure(row, exp, host1, dev1, host_many, dev_many):
        ok = True
        for key, fn, many in (("single_host", host1, False), ("single_device", dev1, False),
                              ("pipelined_host", host_many, True), ("pipelined_device", dev_many, True)):
            ms, runs, res = timed(fn, a.runs)
            if many:
                row[key + "_ms_per_msm"] = round(ms / count, 4)
                ok = ok and [as_xy(r) for r in res] == [exp] * count
            else:
                row[key + "_ms"] = round(ms, 4)
                ok = ok and res == exp
            row[key + "_runs_ms"] = runs
        row["phases_ms"] = profile(dev1)
        row["correct"] = ok
        emit(row)

    pts = M.gen_points(n, k0=k0, step=step)
    neg_pts = pts.copy()  # every point negated: x -> -x mod p, t -> -t mod p (multi-word, in numpy)
    pw = np.array(O.int_to_be_words(O.P), dtype=np.int64)
    for j in (0, 2):
        d = pw[None, :] - pts[:, 8 * j:8 * j + 8].astype(np.int64)
        for k in range(7, 0, -1):  # borrows
            borrow = d[:, k] < 0
            d[:, k] += borrow.astype(np.int64) << 32
            d[:, k - 1] -= borrow
        zero = ~pts[:, 8 * j:8 * j + 8].any(axis=1)
        d[zero] = 0
        neg_pts[:, 8 * j:8 * j + 8] = d.astype(np.uint32)
    ks = k0 + step * np.arange(n, dtype=np.uint64)
    rnd = np.random.RandomState(41)

    def be_words(limbs):
        """[n, k] little-endian u64 limbs -> [n, 2 k] big-endian u32 words: the rewrite call (a)'s caller pays."""
        return np.ascontiguousarray(limbs.view(np.uint32)[:, ::-1])

    with M.Bases.from_wire(pts, levels=1) as plain:
        for ty in a.wide_types:
            e = M.WIDE_TYPES[ty][1]
            k = e // 64
            arr = rnd.randint(0, 1 << 32, size=(n, k), dtype=np.uint64) | rnd.randint(0, 1 << 32, size=(n, k), dtype=np.uint64) << np.uint64(32)
            isneg = np.zeros(n, bool)
            if ty == "fr_mont":
                arr[:, 3] %= np.uint64(R >> 192)  # a < r: the top limb below r's
            arr = np.ascontiguousarray(arr)
            t0 = time.perf_counter()
            if ty == "i128":
                isneg = (arr[:, 1] >> np.uint64(63)).astype(bool)
                lo = np.where(isneg, ~arr[:, 0] + np.uint64(1), arr[:, 0])
                hi = np.where(isneg, ~arr[:, 1] + (lo == 0).astype(np.uint64), arr[:, 1])
                sc = be_words(np.ascontiguousarray(np.stack([lo, hi], axis=1)))
            elif ty == "fr_mont":
                rinv = pow(2, -256, R)
                raw = arr.astype("<u8").tobytes()
                sc = np.frombuffer(b"".join((int.from_bytes(raw[32 * i:32 * i + 32], "little") * rinv % R).to_bytes(32, "big")
                                            for i in range(n)), dtype=">u4").astype(np.uint32).reshape(n, 8)
            else:
                sc = be_words(arr)
            convert_ms = (time.perf_counter() - t0) * 1e3
            words = sc.shape[1]
            sc8p, sc8n = np.zeros((n, 8), np.uint32), np.zeros((n, 8), np.uint32)
            sc8p[~isneg, 8 - words:] = sc[~isneg]
            sc8n[isneg, 8 - words:] = sc[isneg]
            exp = O.scalar_mul(O.G, (scalar_dot(ks, sc8p) - scalar_dot(ks, sc8n)) % O.R_ORDER)
            base = {"entry": "wide", "type": ty, "bits": e, "count": count, "vector_bytes": int(arr.nbytes)}
            d_sc = torch.from_numpy(sc.view(np.int32)).cuda()
            d_arr = torch.from_numpy(arr.view(np.int64)).cuda()
            kw = {"scalar_bits": 128} if e == 128 else {}
            tk = {"scalar_type": ty}

            def words_rows(bases, repeat):  # (a) the existing call on the converted words
                measure({**base, "form": "words", "repeat": repeat, "convert_ms": round(convert_ms, 4)}, exp,
                        lambda: bases.compute(sc, **kw), lambda: bases.compute_device(d_sc, **kw),
                        lambda: bases.compute_many([sc] * count, **kw),
                        lambda: bases.compute_many_device([d_sc] * count, **kw))

            # (a) over a handle whose points carry the signs (i128), before and after (b) on the array as it is
            signed_bases = M.Bases.from_wire(np.where(isneg[:, None], neg_pts, pts), levels=1) if isneg.any() else plain
            try:
                words_rows(signed_bases, 0)
                measure({**base, "form": "wide"}, exp,
                        lambda: plain.compute(arr, **tk), lambda: plain.compute_device(d_arr, **tk),
                        lambda: plain.compute_many([arr] * count, **tk),
                        lambda: plain.compute_many_device([d_arr] * count, **tk))
                words_rows(signed_bases, 1)
            finally:
                if signed_bases is not plain:
                    signed_bases.close()
    return 1 if bad else 0


def compressed_pass(a):
    import numpy as np
    import torch

    import msm_amd as M
    from _closed_form import closed_form

    n = a.n

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()

    pts = M.gen_points(n, k0=3, step=5)
    sc = M.gen_scalars(n, seed=500)
    exp = closed_form(3, 5, sc)
    d_pts = dev(pts)
    d_out = torch.zeros((n, 32), dtype=torch.int32, device="cuda")
    xs = {"subgroup": np.ascontiguousarray(pts[:, :8]), "ysign": M.compress_points(pts, "ysign")}
    torch.cuda.synchronize()

    def create(make):
        def run():
            make().close()
        return run

    wire_ms, wire_runs, _ = timed(create(lambda: M.Bases.from_wire(pts, levels=1)), a.runs)
    dwire_ms, dwire_runs, _ = timed(create(lambda: M.Bases.from_device(d_pts, n, levels=1)), a.runs)
    for form, w in xs.items():
        d_xs = dev(w)
        torch.cuda.synchronize()
        with M.Bases.from_x(w, form, levels=1) as b:
            correct = b.compute(sc) == exp
        hx_ms, hx_runs, _ = timed(create(lambda: M.Bases.from_x(w, form, levels=1)), a.runs)
        dx_ms, dx_runs, _ = timed(create(lambda: M.Bases.from_x_device(d_xs, n, form, levels=1)), a.runs)
        k_ms, k_runs, _ = timed(lambda: M.decompress_points_device(d_xs, n, d_out, form), a.runs)
        same = bool(np.array_equal(d_out.cpu().numpy().view(np.uint32), pts))
        d = {"n": n, "entry": "compressed", "form": form, "from_x_ms": round(hx_ms, 4),
             "from_x_device_ms": round(dx_ms, 4), "decompress_device_ms": round(k_ms, 4),
             "decompress_ns_per_point": round(k_ms * 1e6 / n, 2), "from_wire_ms": round(wire_ms, 4),
             "from_device_ms": round(dwire_ms, 4), "runs_ms": {"from_x": hx_runs, "from_x_device": dx_runs,
                                                               "decompress_device": k_runs, "from_wire": wire_runs,
                                                               "from_device": dwire_runs},
             "correct": bool(correct), "records_equal": same}
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")
        if not (correct and same):
            return 1
    return 0


def scale_pass(a):
    """--scale: every size of the sweep in this one process (one context, one torch import)."""
    import numpy as np
    import torch

    import msm_amd as M
    from oracle import oracle as O

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()

    def emit(d):
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    def affine(rec):
        return (O.be_words_to_int(rec[:8]), O.be_words_to_int(rec[8:16]))

    bad = 0
    rng = np.random.default_rng(2024)
    for lg in a.scale_sizes:
        m = 1 << lg
        pts = M.gen_points(m, k0=3, step=5)
        idx = rng.integers(0, m, size=m, dtype=np.uint32)
        d_idx = dev(idx)
        d_out = torch.zeros((m, 32), dtype=torch.int32, device="cuda")
        with M.Bases.from_wire(pts, levels=1) as b:
            for bits in a.scale_bits:
                sw = (bits + 31) // 32
                sc = rng.integers(0, 1 << 32, size=(m, sw), dtype=np.uint64).astype(np.uint32)
                if bits % 32:
                    sc[:, 0] &= (1 << (bits % 32)) - 1
                d_sc = dev(sc)
                kw = {} if bits == 256 else {"scalar_bits": bits}
                torch.cuda.synchronize()
                rows = {}
                rows["device_range"] = timed(lambda: b.scale_device(d_sc, d_out, **kw), a.runs)
                got = d_out.cpu().numpy().view(np.uint32)
                sample = [0, m - 1] + [int(i) for i in rng.integers(0, m, size=4)]
                correct = all(affine(got[i]) == O.c_scalar_mul(affine(pts[i]), O.be_words_to_int(sc[i])) and
                              got[i][31] == 1 for i in sample)
                rows["device_indexed"] = timed(lambda: b.scale_device(d_sc, d_out, indices=d_idx, **kw), a.runs)
                got = d_out.cpu().numpy().view(np.uint32)
                correct = correct and all(
                    affine(got[i]) == O.c_scalar_mul(affine(pts[idx[i]]), O.be_words_to_int(sc[i])) for i in sample)
                rows["host"] = timed(lambda: b.scale(sc, **kw), a.runs)
                correct = correct and bool(np.array_equal(rows["host"][2][sample], b.scale(sc[sample], indices=np.array(
                    sample, np.uint32), **kw)))
                for form, (ms, runs, _) in rows.items():
                    emit({"entry": "scale", "m": m, "bits": bits, "form": form, "ms": round(ms, 4),
                          "ns_per_point": round(ms * 1e6 / m, 2), "runs_ms": runs, "correct": bool(correct)})
                bad += not correct
    # what the library offered before, in the same run: m one-term MSMs, one launch group per point
    for lg in a.scale_msm_sizes:
        m = 1 << lg
        with M.Bases.from_wire(M.gen_points(m, k0=3, step=5), levels=1) as b:
            sc = rng.integers(0, 1 << 32, size=(m, 8), dtype=np.uint64).astype(np.uint32)
            d_sc = dev(sc)
            d_ar = dev(np.arange(m, dtype=np.uint32))
            s_list = [d_sc[i:i + 1] for i in range(m)]
            i_list = [d_ar[i:i + 1] for i in range(m)]
            torch.cuda.synchronize()
            ms, runs, res = timed(lambda: b.compute_subset_many_device(s_list, indices=i_list, m=1), a.runs)
            correct = bool(np.array_equal(res, b.scale(sc)[:, :16]))
            emit({"entry": "scale", "m": m, "bits": 256, "form": "one_term_msms", "ms": round(ms, 4),
                  "ns_per_point": round(ms * 1e6 / m, 2), "runs_ms": runs, "correct": correct})
            bad += not correct
    return 1 if bad else 0


def combine_pass(a):
    """--combine: every size of the sweep in this one process (one context, one torch import)."""
    import numpy as np
    import torch

    import msm_amd as M
    from oracle import oracle as O

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()

    def emit(d):
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    def affine(rec):
        return (O.be_words_to_int(rec[:8]), O.be_words_to_int(rec[8:16]))

    def mul(p, k):
        return p if k is None else O.c_scalar_mul(p, k)

    bad = 0
    rng = np.random.default_rng(2025)
    mmax = 1 << max(a.combine_sizes)
    pts = M.gen_points(2 * mmax, k0=3, step=5)
    with M.Bases.from_wire(pts, levels=1) as h:
        for lg in a.combine_sizes:
            m = 1 << lg
            d_out = torch.zeros((m, 32), dtype=torch.int32, device="cuda")
            d_out2 = torch.zeros((m, 32), dtype=torch.int32, device="cuda")
            sample = [0, m - 1] + [int(i) for i in rng.integers(0, m, size=2)]

            def check(ka, kb):
                got = d_out.cpu().numpy().view(np.uint32)
                return all(affine(got[i]) == O.aff_add(mul(affine(pts[i]), ka(i)), mul(affine(pts[m + i]), kb(i))) and
                           got[i][31] == 1 for i in sample)

            torch.cuda.synchronize()
            ms, runs, _ = timed(lambda: h.combine_device(d_out, b_first=m, m=m), a.runs)
            ok = check(lambda i: None, lambda i: None)
            nbytes = m * (2 * 128 + 2 * 108 + 128)  # two records in, (X : Y : Z) out and in again, a wire record out
            emit({"entry": "combine", "m": m, "bits": 0, "form": "sum", "ms": round(ms, 4),
                  "ns_per_point": round(ms * 1e6 / m, 2), "runs_ms": runs, "spread": round(max(runs) - min(runs), 4),
                  "bytes": nbytes, "gb_per_s": round(nbytes / ms / 1e6, 1), "correct": bool(ok)})
            bad += not ok
            for bits in a.combine_bits:
                sw = (bits + 31) // 32
                sc = rng.integers(0, 1 << 32, size=(2, m, sw), dtype=np.uint64).astype(np.uint32)
                if bits % 32:
                    sc[:, :, 0] &= (1 << (bits % 32)) - 1
                d_sa, d_sb = dev(sc[0]), dev(sc[1])
                d_xa, d_xb = dev(sc[0][:1]), dev(sc[1][:1])
                ia = lambda i: O.be_words_to_int(sc[0][i])  # noqa: E731
                ib = lambda i: O.be_words_to_int(sc[1][i])  # noqa: E731
                kw = {} if bits == 256 else {"scalar_bits": bits}
                torch.cuda.synchronize()

                def twice():
                    h.scale_device(d_sa, d_out, **kw)
                    h.scale_device(d_sb, d_out2, first=m, **kw)

                rows, oks = {}, {}
                rows["scale_once"] = timed(lambda: h.scale_device(d_sb, d_out2, first=m, **kw), a.runs)
                rows["scale_twice"] = timed(twice, a.runs)
                rows["one"] = timed(lambda: h.combine_device(d_out, b=d_sb, b_first=m, **kw), a.runs)
                oks["one"] = check(lambda i: None, ib)
                rows["joint"] = timed(lambda: h.combine_device(d_out, a=d_sa, b=d_sb, b_first=m, **kw), a.runs)
                oks["joint"] = check(ia, ib)
                rows["one_broadcast"] = timed(
                    lambda: h.combine_device(d_out, b=d_xb, b_first=m, m=m, b_broadcast=True, **kw), a.runs)
                oks["one_broadcast"] = check(lambda i: None, lambda i: ib(0))
                rows["joint_broadcast"] = timed(
                    lambda: h.combine_device(d_out, a=d_xa, b=d_xb, b_first=m, m=m, a_broadcast=True, b_broadcast=True,
                                             **kw), a.runs)
                oks["joint_broadcast"] = check(lambda i: ia(0), lambda i: ib(0))
                for form, (ms, runs, _) in rows.items():
                    ref = rows["scale_twice" if form.startswith("joint") else "scale_once"][0]
                    emit({"entry": "combine", "m": m, "bits": bits, "form": form, "ms": round(ms, 4),
                          "ns_per_point": round(ms * 1e6 / m, 2), "runs_ms": runs,
                          "spread": round(max(runs) - min(runs), 4), "ratio": round(ms / ref, 4),
                          "correct": bool(oks.get(form, True))})
                bad += not all(oks.values())
    return 1 if bad else 0


def fr_pass(a):
    """--fr: every size of the Fr vector sweep in this one process (one context, one torch import)."""
    import numpy as np
    import torch

    import msm_amd as M

    R = M.FR_MODULUS

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()

    def emit(d):
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    def synced(fn):
        def run():
            fn()
            torch.cuda.synchronize()
        return run

    def ints(t, idx, form="wire"):
        return M.fr_to_ints(t[idx].cpu().numpy().view(np.uint32), form)

    bad = 0
    rng = np.random.default_rng(2026)
    for lg in a.fr_sizes:
        n = 1 << lg
        h = n // 2
        wa = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
        wb = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
        d_a, d_b = dev(wa), dev(wb)
        va = lambda i: M.wire_to_int(wa[i])  # noqa: E731
        vb = lambda i: M.wire_to_int(wb[i])  # noqa: E731
        mont = wa.copy()  # canonical little-endian words: the top word below r's
        mont[:, 7] &= 0x03ffffff
        d_m = dev(mont)
        x, y = int(rng.integers(1, 1 << 62)) << 180, int(rng.integers(1, 1 << 62)) << 150
        d_x, d_y = dev(M.scalars_to_wire([x])), dev(M.scalars_to_wire([y]))
        o_n = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
        o_h = torch.zeros((h, 8), dtype=torch.int32, device="cuda")
        t_n, t_h = torch.zeros_like(o_n), torch.zeros_like(o_h)
        sample = [0, 63, n - 1] + [int(i) for i in rng.integers(0, n, size=3)]
        sample_h = [i % h for i in sample]
        scratch = d_a.clone()
        r_inv = pow(1 << 256, -1, R)
        dot = {}

        def run_dot():
            dot["v"] = M.fr_dot(d_a[:a.fr_dot_check], d_b[:a.fr_dot_check])
            return M.fr_dot(d_a, d_b)

        # op: (call, bytes moved, torch yardstick and its name, check)
        ops = {
            "fold": (lambda: M.fr_fold(d_a, x, y, out=o_h), 48 * n, synced(lambda: torch.add(d_a[:h], d_a[h:], out=t_h)),
                     "add(lo, hi, out)", lambda: ints(o_h, sample_h) == [(x * va(i) + y * va(i + h)) % R for i in sample_h]),
            "fold_in_place": (lambda: M.fr_fold(scratch, x, y, out=scratch[:h]), 48 * n,
                              synced(lambda: torch.add(d_a[:h], d_a[h:], out=t_h)), "add(lo, hi, out)", lambda: True),
            "hadamard": (lambda: M.fr_mul(d_a, d_b, out=o_n), 96 * n, synced(lambda: torch.add(d_a, d_b, out=t_n)),
                         "add(a, b, out)", lambda: ints(o_n, sample) == [va(i) * vb(i) % R for i in sample]),
            "scale": (lambda: M.fr_mul(d_a, d_x, out=o_n), 64 * n, synced(lambda: torch.add(d_a, 1, out=t_n)), "add(a, 1, out)",
                      lambda: ints(o_n, sample) == [va(i) * x % R for i in sample]),
            "add": (lambda: M.fr_combine(d_a, d_b, out=o_n), 96 * n, synced(lambda: torch.add(d_a, d_b, out=t_n)),
                    "add(a, b, out)", lambda: ints(o_n, sample) == [(va(i) + vb(i)) % R for i in sample]),
            "convert": (lambda: M.fr_convert(d_m, "fr_mont", "wire", out=o_n), 64 * n,
                        synced(lambda: torch.add(d_m, 1, out=t_n)), "add(a, 1, out)",
                        lambda: ints(o_n, sample) == [int.from_bytes(mont[i].astype("<u4").tobytes(), "little") * r_inv % R
                                                      for i in sample]),
            "powers": (lambda: M.fr_powers(x, n, first=y, out=o_n), 32 * n, synced(lambda: t_n.zero_()), "zero_(out)",
                       lambda: ints(o_n, sample) == [y * pow(x, i, R) % R for i in sample]),
            "dot": (run_dot, 64 * n, synced(lambda: torch.add(d_a, d_b, out=t_n)), "add(a, b, out)",
                    lambda: M.fr_to_ints([dot["v"]])[0] == sum(va(i) * vb(i) for i in range(a.fr_dot_check)) % R),
        }
        for op, (call, nbytes, yard, yard_name, check) in ops.items():
            torch.cuda.synchronize()
            ms, runs, _ = timed(call, a.runs)
            ok = bool(check())
            t_ms, _, _ = timed(yard, a.runs)
            emit({"entry": "fr", "op": op, "n": n, "ms": round(ms, 4), "ns_per_elem": round(ms * 1e6 / n, 3), "runs_ms": runs,
                  "bytes": nbytes, "gb_per_s": round(nbytes / ms / 1e6, 1), "torch_op": yard_name, "torch_ms": round(t_ms, 4),
                  "ratio_to_torch": round(ms / t_ms, 3), "correct": ok})
            bad += not ok
        if lg != a.fr_compare:
            continue
        # the two routes of the issue's timing, in this process
        pts = M.gen_points(n, k0=3, step=5)
        with M.Bases.from_wire(pts, levels=1) as g:
            def bases_fold():
                g.fold(x, y).close()
            f_ms, f_runs, _ = timed(bases_fold, a.runs)
            s_ms, s_runs, _ = timed(lambda: M.fr_fold(d_a, x, y, out=o_h), a.runs)
            emit({"entry": "fr", "op": "fold_vs_bases_fold", "n": n, "fr_fold_ms": round(s_ms, 4), "fr_fold_runs_ms": s_runs,
                  "bases_fold_ms": round(f_ms, 4), "bases_fold_runs_ms": f_runs, "ratio": round(s_ms / f_ms, 5)})
            with g.fixed_table(first=0, count=1) as t:
                tau = (x + 12345) % R

                def device_route():
                    t.mul_bases_device(M.fr_powers(tau, n, device=0), n, levels=1).close()

                def host_route():
                    pw = [1] * n
                    for i in range(1, n):
                        pw[i] = pw[i - 1] * tau % R
                    t.mul_bases(M.scalars_to_wire(pw), levels=1).close()

                d_ms, d_runs, _ = timed(device_route, a.runs)
                t0 = time.perf_counter()
                host_route()
                h_ms = (time.perf_counter() - t0) * 1e3
                with t.mul_bases_device(M.fr_powers(tau, n, device=0), n, levels=1) as srs:
                    got = srs.points(first=n - 2, m=2)
                from oracle import oracle as O
                exp = O.affine_to_wire([O.c_scalar_mul(O.c_scalar_mul(O.G, 3), pow(tau, i, R)) for i in (n - 2, n - 1)])
                ok = bool(np.array_equal(got, exp))
                emit({"entry": "fr", "op": "srs", "n": n, "device_route_ms": round(d_ms, 4), "device_route_runs_ms": d_runs,
                      "host_route_ms": round(h_ms, 2), "ratio": round(d_ms / h_ms, 6), "correct": ok})
                bad += not ok
    return 1 if bad else 0


def frscan_pass(a):
    """--frscan: every size of the inverse / scan / tensor sweep in this one process."""
    import numpy as np
    import torch

    import msm_amd as M

    R = M.FR_MODULUS

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()

    def emit(d):
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    def decode(words):
        raw = np.ascontiguousarray(words, dtype=np.uint32).astype(">u4").tobytes()
        return [int.from_bytes(raw[32 * i: 32 * i + 32], "big") for i in range(len(raw) // 32)]

    def encode(vals):
        return np.frombuffer(b"".join(v.to_bytes(32, "big") for v in vals), dtype=">u4").astype(np.uint32).reshape(-1, 8)

    def clock(fn):
        t0 = time.perf_counter()
        res = fn()
        return res, (time.perf_counter() - t0) * 1e3

    def host_inverse(vals):  # Montgomery's trick: one inversion, three products per element
        pre, acc = [], 1
        for v in vals:
            pre.append(acc)
            acc = acc * v % R
        inv = pow(acc, -1, R)
        out = [0] * len(vals)
        for i in range(len(vals) - 1, -1, -1):
            out[i] = inv * pre[i] % R
            inv = inv * vals[i] % R
        return out

    def host_cumprod(vals):
        out, acc = [], 1
        for v in vals:
            acc = acc * v % R
            out.append(acc)
        return out

    def host_cumsum(vals):
        out, acc = [], 0
        for v in vals:
            acc = (acc + v) % R
            out.append(acc)
        return out

    def host_tensor(pairs):
        out = [1]
        for lo, hi in pairs:
            out = [v * lo % R for v in out] + [v * hi % R for v in out]
        return out

    bad = 0
    rng = np.random.default_rng(2027)
    for lg in a.frscan_sizes:
        n = 1 << lg
        wa = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
        wb = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
        d_a, d_b = dev(wa), dev(wb)
        o_n = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
        pairs = [(int.from_bytes(rng.bytes(32), "big"), int.from_bytes(rng.bytes(32), "big")) for _ in range(lg)]
        torch.cuda.synchronize()
        mul_ms, mul_runs, _ = timed(lambda: M.fr_mul(d_a, d_b, out=o_n), a.runs)
        # the route a caller had: down and decode once, encode and up once, shared by the operations
        vals, down_ms = clock(lambda: [v % R for v in decode(d_a.cpu().numpy().view(np.uint32))])
        ops = {
            "inverse": (lambda: M.fr_inverse(d_a, out=o_n), lambda: host_inverse(vals)),
            "cumprod": (lambda: M.fr_cumprod(d_a, out=o_n), lambda: host_cumprod(vals)),
            "cumsum": (lambda: M.fr_cumsum(d_a, out=o_n), lambda: host_cumsum(vals)),
            "tensor": (lambda: M.fr_tensor(pairs, out=o_n), lambda: host_tensor(pairs)),
        }
        up_ms = None
        for op, (call, host) in ops.items():
            torch.cuda.synchronize()
            ms, runs, _ = timed(call, a.runs)
            exp, host_ms = clock(host)
            if up_ms is None:
                _, up_ms = clock(lambda: dev(encode(exp)))
            ok = bool(np.array_equal(o_n.cpu().numpy().view(np.uint32), encode(exp)))
            parts = {"down_decode": round(0.0 if op == "tensor" else down_ms, 2), "python": round(host_ms, 2),
                     "encode_up": round(up_ms, 2)}
            emit({"entry": "frscan", "op": op, "n": n, "ms": round(ms, 4), "ns_per_elem": round(ms * 1e6 / n, 3), "runs_ms": runs,
                  "fr_mul_ms": round(mul_ms, 4), "fr_mul_runs_ms": mul_runs, "ratio_to_fr_mul": round(ms / mul_ms, 3),
                  "host_route_ms": round(sum(parts.values()), 2), "host_parts_ms": parts, "correct": ok})
            bad += not ok
    return 1 if bad else 0


def fixed_pass(a):
    """--fixed: every size of the fixed-base sweep in this one process (one context, one torch import)."""
    import numpy as np
    import torch

    import msm_amd as M
    from oracle import oracle as O

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()

    def emit(d):
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    def affine(rec):
        return (O.be_words_to_int(rec[:8]), O.be_words_to_int(rec[8:16]))

    bad = 0
    rng = np.random.default_rng(2025)
    pts = M.gen_points(2, k0=3, step=5)
    aff = [affine(p) for p in pts]
    mmax = 1 << a.fixed_sizes[-1]
    d_out = torch.zeros((mmax, 32), dtype=torch.int32, device="cuda")
    d_zero = dev(np.zeros(mmax, np.uint32))
    with M.Bases.from_wire(pts, levels=1) as b:
        for bits in a.fixed_bits:
            sw = (bits + 31) // 32
            kw = {} if bits == 256 else {"scalar_bits": bits}
            sc_all = rng.integers(0, 1 << 32, size=(mmax, 2, sw), dtype=np.uint64).astype(np.uint32)
            if bits % 32:
                sc_all[:, :, 0] &= (1 << (bits % 32)) - 1
            # the baseline, same process and same scalars: the ladder on base 0 (an index vector of zeros)
            base_ms = {}
            for lg in a.fixed_sizes:
                m = 1 << lg
                d_sc = dev(sc_all[:m, 0])
                torch.cuda.synchronize()
                ms, runs, _ = timed(lambda: b.scale_device(d_sc, d_out[:m], indices=d_zero[:m], **kw), a.runs)
                base_ms[m] = ms
                emit({"entry": "fixed", "m": m, "bits": bits, "k": 1, "form": "scale_zero_indices", "ms": round(ms, 4),
                      "ns_per_point": round(ms * 1e6 / m, 2), "runs_ms": runs})
            for w in a.fixed_widths:
                for k in a.fixed_bases:
                    ms, runs, t = timed(lambda: b.fixed_table(first=0, count=k, window_bits=w, scalar_bits=bits), a.runs)
                    emit({"entry": "fixed", "bits": bits, "w": w, "k": k, "form": "table_build", "ms": round(ms, 4),
                          "bytes": t.info["bytes"], "runs_ms": runs})
                    with t:
                        for lg in a.fixed_sizes:
                            m = 1 << lg
                            sc = np.ascontiguousarray(sc_all[:m, :k])
                            d_sc = dev(sc)
                            torch.cuda.synchronize()
                            rows = {"device": timed(lambda: t.mul_device(d_sc, d_out[:m], **kw), a.runs)}
                            got = d_out[:m].cpu().numpy().view(np.uint32)
                            sample = [0, m - 1] + [int(i) for i in rng.integers(0, m, size=2)]
                            correct = True
                            for i in sample:
                                acc = (0, 1)
                                for j in range(k):
                                    acc = M.point_add_affine(acc, O.c_scalar_mul(aff[j], O.be_words_to_int(sc[i, j])))
                                correct = correct and affine(got[i]) == acc and got[i][31] == 1
                            rows["host"] = timed(lambda: t.mul(sc, **kw), a.runs)
                            correct = correct and bool(np.array_equal(rows["host"][2], got))
                            for form, (ms, runs, _) in rows.items():
                                d = {"entry": "fixed", "m": m, "bits": bits, "w": w, "k": k, "form": form,
                                     "ms": round(ms, 4), "ns_per_point": round(ms * 1e6 / m, 2), "runs_ms": runs,
                                     "correct": bool(correct)}
                                if form == "device" and k == 1:
                                    d["ratio_to_scale"] = round(base_ms[m] / ms, 2)
                                emit(d)
                            bad += not correct
    return 1 if bad else 0


def vector_pass(a):
    """--vector: the vector-table sweep (msm_fixed_create_vector) in this one process.  For every shape
    (k, m) and width b: today's route on the same scalars -- m subset MSMs of k terms through
    compute_subset_many_device, at b < 256 also in its narrow form, the faster one kept --, then for
    every window width whose table fits a table build and the evaluation (device to device, median of
    `runs` awaited calls) with the plan's G and P; and at --vector-group-w the evaluation at every G."""
    import numpy as np
    import torch

    import msm_amd as M

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).cuda()

    def emit(d):
        print(json.dumps(d), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    bad = 0
    rng = np.random.default_rng(2026)
    kmax = max(k for k, _ in a.vector_shapes)
    pts = M.gen_points(kmax, k0=3, step=5)
    with M.Bases.from_wire(pts, levels=1) as b:
        b.vector_table(first=0, count=9, window_bits=2, scalar_bits=8).close()  # warm-up: the build's kernels
        for k, lg in a.vector_shapes:
            m = 1 << lg
            d_out = torch.zeros((m, 32), dtype=torch.int32, device="cuda")
            for bits in a.vector_bits:
                sw = (bits + 31) // 32
                kw = {} if bits == 256 else {"scalar_bits": bits}
                sc = rng.integers(0, 1 << 32, size=(m, k, sw), dtype=np.uint64).astype(np.uint32)
                if bits % 32:
                    sc[:, :, 0] &= (1 << (bits % 32)) - 1
                wide = np.zeros((m, k, 8), np.uint32)
                wide[:, :, 8 - sw:] = sc
                d_sc, d_wide = dev(sc), dev(wide)
                torch.cuda.synchronize()
                # today's route: one MSM per row, pipelined; raw row pointers, the caller orders the streams
                routes = {"subset_many": ([d_wide.data_ptr() + i * k * 32 for i in range(m)], {})}
                if bits < 256:
                    routes["subset_many_narrow"] = ([d_sc.data_ptr() + i * k * sw * 4 for i in range(m)], kw)
                base = {}
                for form, (ptrs, okw) in routes.items():
                    try:
                        ms, runs, res = timed(lambda: b.compute_subset_many_device(ptrs, first=0, m=k, **okw), a.runs)
                    except M.MsmError as e:
                        emit({"entry": "vector", "k": k, "m": m, "bits": bits, "form": form, "error": e.code})
                        return 1
                    base[form] = (ms, runs, res)
                    emit({"entry": "vector", "k": k, "m": m, "bits": bits, "form": form, "ms": round(ms, 4),
                          "us_per_row": round(ms * 1e3 / m, 3), "runs_ms": runs})
                best_form = min(base, key=lambda f: base[f][0])
                base_ms, base_runs, base_xy = base[best_form]
                if len(base) == 2:
                    bad += not np.array_equal(base["subset_many"][2], base["subset_many_narrow"][2])

                def evaluate(t, w, forced):
                    nonlocal bad
                    M._test_vector_group(forced)
                    plan = M._test_vector_plan(k, w, t.info["scalar_bits"], m, sw)
                    ms, runs, _ = timed(lambda: t.mul_device(d_sc, d_out, **kw), a.runs)
                    M._test_vector_group(0)
                    got = d_out.cpu().numpy().view(np.uint32)
                    correct = bool(np.array_equal(got[:, :16], base_xy)) and bool(np.all(got[:, 31] == 1))
                    bad += not correct
                    emit({"entry": "vector", "k": k, "m": m, "bits": bits, "w": t.info["window_bits"], "auto_w": w == 0,
                          "form": "table", "forced_G": forced,
                          "G": plan["G"], "P": plan["P"], "passes": plan["passes"], "slab_rows": plan["slab_rows"],
                          "ms": round(ms, 4), "us_per_row": round(ms * 1e3 / m, 3), "runs_ms": runs,
                          "baseline": best_form, "baseline_ms": round(base_ms, 4), "ratio_to_baseline": round(base_ms / ms, 2),
                          "table_bytes": t.info["bytes"], "correct": correct})

                auto_w = M._test_vector_plan(k, 0, bits)["window_bits"]
                for w in a.vector_widths:
                    try:
                        M._test_vector_plan(k, w, bits)
                    except M.MsmError:
                        continue  # over 256 MiB
                    t0 = time.perf_counter()
                    t = b.vector_table(first=0, count=k, window_bits=w, scalar_bits=bits)
                    emit({"entry": "vector", "k": k, "bits": bits, "w": w or auto_w, "form": "table_build", "auto_w": auto_w,
                          "ms": round((time.perf_counter() - t0) * 1e3, 3), "bytes": t.info["bytes"]})
                    with t:
                        evaluate(t, w, 0)
                        if w == a.vector_group_w:
                            for g in a.vector_groups:
                                evaluate(t, w, g)
    return 1 if bad else 0


def dense_sweep(a):
    """The children of --dense, one after the other; stops at the first that fails."""
    def child(lg, bits, extra, equal, dense_min, extended):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--n", str(1 << lg),
               "--narrow", "--narrow-bits", bits, "--narrow-widths", "", "--narrow-extra", extra, "--count", str(a.count),
               "--runs", str(a.runs)]
        cmd += (["--narrow-equal"] if equal else []) + ([] if extended else ["--no-extended"])
        cmd += ["--out", a.out] if a.out else []
        env = dict(os.environ)
        env.pop("MSM_DENSE_MIN", None)
        if dense_min:
            env["MSM_DENSE_MIN"] = str(dense_min)
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            print(f"bases_probe: size 2^{lg} (MSM_DENSE_MIN={dense_min}) ended with status {rc}; stopping", file=sys.stderr)
        return rc

    off = 1 << 30
    for lg in (int(x) for x in a.sizes.split(",")):
        for dense_min in (None, off):  # as planned (with the 8-word rows), then the path off
            if rc := child(lg, "1,4,8,12", "16:16", lg == 20, dense_min, dense_min is None):
                return rc
    # the threshold rows, path forced on and off: bytes (256 keys) at 32..256 entries per bucket, 12 bits
    # (4,096 keys) at 32..128, and 13 bits at 2^20 (8,192 keys at 128 per bucket; its two-MSM launches
    # are past DENSE_MAX_KEYS, as any launch of 14 and 15 bits is: the committed rows of those were
    # taken with the cap lifted)
    for lg, bits in ((13, 8), (14, 8), (15, 8), (16, 8), (17, 12), (18, 12), (19, 12), (20, 13)):
        for dense_min in (1, off):
            if rc := child(lg, str(bits), "", False, dense_min, False):
                return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="run this one size in-process")
    ap.add_argument("--sizes", default="16,18,20", help="log2 sizes of the sweep")
    ap.add_argument("--levels", default="1,2,4")
    ap.add_argument("--count", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--c17", action="store_true", help="also time c = 17 (32-bit digit codes)")
    ap.add_argument("--wide", action="store_true", help="the wide-type sweep (MSM_FLAG_SCALAR_FIELD) instead")
    ap.add_argument("--wide-types", default="u128,i128,u256,fr_mont", help="types of the wide sweep")
    ap.add_argument("--out", default="")
    ap.add_argument("--subset", action="store_true", help="the subset sweep (msm_bases_compute_subset*) instead")
    ap.add_argument("--subset-sizes", default="12,16,18,20", help="log2 term counts m of the subset sweep")
    ap.add_argument("--narrow", action="store_true", help="the narrow-scalar sweep (MSM_FLAG_SCALAR_BITS) instead")
    ap.add_argument("--narrow-bits", default="8,16,32,64,128,253", help="scalar widths b of the narrow sweep")
    ap.add_argument("--narrow-widths", default="13,14,15,16,17,19", help="explicit window widths of the narrow sweep")
    ap.add_argument("--narrow-extra", default="", help="more narrow rows at explicit widths, as b:c,b:c")
    ap.add_argument("--narrow-equal", action="store_true", help="a narrow row of all-equal bytes as well")
    ap.add_argument("--no-extended", action="store_true", help="the narrow pass without its 8-word rows")
    ap.add_argument("--dense", action="store_true", help="the dense-bucket sweep (DENSE_MIN, MSM_DENSE_MIN) instead")
    ap.add_argument("--native", action="store_true", help="the native-type sweep (MSM_FLAG_SCALAR_TYPE) instead")
    ap.add_argument("--native-types", default="bit,u8,i8,u16,i16,i32,i64,u64", help="types of the native sweep")
    ap.add_argument("--compressed", action="store_true", help="the compressed-creation sweep (MSM_POINTS_X_*) instead")
    ap.add_argument("--scale", action="store_true", help="the per-point scalar-multiple sweep (msm_bases_scale*) instead")
    ap.add_argument("--scale-sizes", default="12,13,14,15,16,17,18,19,20", help="log2 point counts m of the scale sweep")
    ap.add_argument("--scale-bits", default="64,128,253,256", help="scalar widths b of the scale sweep")
    ap.add_argument("--scale-msm-sizes", default="10,12", help="log2 m at which the one-term-MSM route is timed too")
    ap.add_argument("--scale-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--fixed", action="store_true", help="the fixed-base table sweep (msm_fixed_*) instead")
    ap.add_argument("--fixed-sizes", default="12,13,14,15,16,17,18,19,20", help="log2 row counts m of the fixed sweep")
    ap.add_argument("--fixed-bits", default="64,128,253,256", help="scalar widths b of the fixed sweep")
    ap.add_argument("--fixed-widths", default="6,8,10,12", help="window widths w of the fixed sweep")
    ap.add_argument("--fixed-bases", default="1,2", help="base counts k of the fixed sweep")
    ap.add_argument("--fixed-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--vector", action="store_true", help="the vector-table sweep (msm_fixed_create_vector) instead")
    ap.add_argument("--vector-shapes", default="16:16,64:14,256:12,1024:10,4096:8", help="shapes k:log2(m) of the vector sweep")
    ap.add_argument("--vector-bits", default="256,64", help="scalar widths b of the vector sweep")
    ap.add_argument("--vector-widths", default="2,4,6,8,10,12", help="window widths w of the vector sweep")
    ap.add_argument("--vector-groups", default="1,2,4,8", help="bases per part G timed at --vector-group-w")
    ap.add_argument("--vector-group-w", type=int, default=6, help="the window width at which every G is timed")
    ap.add_argument("--combine", action="store_true", help="the pairwise-combination sweep (msm_bases_combine*) instead")
    ap.add_argument("--combine-sizes", default="12,16,18,20", help="log2 point counts m of the combine sweep")
    ap.add_argument("--combine-bits", default="64,128,256", help="scalar widths b of the combine sweep")
    ap.add_argument("--fr", action="store_true", help="the scalar-field vector sweep (msm_fr_*) instead")
    ap.add_argument("--fr-sizes", default="16,17,18,19,20,21,22", help="log2 element counts n of the Fr sweep")
    ap.add_argument("--fr-compare", type=int, default=20, help="log2 n at which fold and SRS are timed against today's routes (0: skip)")
    ap.add_argument("--fr-dot-check", type=int, default=4096, help="elements of the dot product checked against Python")
    ap.add_argument("--frscan", action="store_true", help="the inverse / scan / tensor sweep (msm_fr_inverse* ..) instead")
    ap.add_argument("--frscan-sizes", default="16,17,18,19,20,21,22", help="log2 element counts n of the --frscan sweep")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds each size may take")
    a = ap.parse_args()
    a.levels = [int(x) for x in str(a.levels).split(",")]
    a.narrow_extra = [tuple(int(v) for v in x.split(":")) for x in str(a.narrow_extra).split(",") if x]
    if a.dense:
        return dense_sweep(a)
    if a.vector:  # one process, as today's route is timed beside the table's rows
        a.vector_shapes = [tuple(int(v) for v in x.split(":")) for x in str(a.vector_shapes).split(",") if x]
        for name in ("vector_bits", "vector_widths", "vector_groups"):
            setattr(a, name, [int(x) for x in str(getattr(a, name)).split(",") if x])
        return vector_pass(a)
    if a.frscan:  # one process, as fr_mul and the host route are timed beside the rows
        a.frscan_sizes = sorted(int(x) for x in str(a.frscan_sizes).split(",") if x)
        return frscan_pass(a)
    if a.fr:  # one process, as the yardsticks are timed beside the rows
        a.fr_sizes = sorted(int(x) for x in str(a.fr_sizes).split(",") if x)
        return fr_pass(a)
    if a.combine:  # one process, as the sweep's references are timed beside its rows
        a.combine_sizes = sorted(int(x) for x in str(a.combine_sizes).split(",") if x)
        a.combine_bits = [int(x) for x in str(a.combine_bits).split(",") if x]
        return combine_pass(a)
    if a.fixed:
        lists = {"--fixed-sizes": "fixed_sizes", "--fixed-bits": "fixed_bits", "--fixed-widths": "fixed_widths",
                 "--fixed-bases": "fixed_bases"}
        for name in lists.values():
            setattr(a, name, sorted(int(x) for x in str(getattr(a, name)).split(",") if x))
        if a.fixed_child:
            return fixed_pass(a)
        cmd = ["timeout", "-k", "10", str(a.step_timeout * 3), sys.executable, os.path.abspath(__file__), "--fixed",
               "--fixed-child", "--runs", str(a.runs)] + (["--out", a.out] if a.out else [])
        for flag, name in lists.items():
            cmd += [flag, ",".join(map(str, getattr(a, name)))]
        return subprocess.run(cmd).returncode
    if a.scale:
        a.scale_bits = [int(x) for x in str(a.scale_bits).split(",") if x]
        a.scale_msm_sizes = [int(x) for x in str(a.scale_msm_sizes).split(",") if x]
        a.scale_sizes = sorted(int(x) for x in str(a.scale_sizes).split(",") if x)
        if a.scale_child:
            return scale_pass(a)
        cmd = ["timeout", "-k", "10", str(a.step_timeout * 3), sys.executable, os.path.abspath(__file__), "--scale",
               "--scale-child", "--scale-sizes", ",".join(map(str, a.scale_sizes)), "--scale-bits",
               ",".join(map(str, a.scale_bits)), "--scale-msm-sizes", ",".join(map(str, a.scale_msm_sizes)),
               "--runs", str(a.runs)] + (["--out", a.out] if a.out else [])
        return subprocess.run(cmd).returncode
    if a.compressed:
        if a.n:
            return compressed_pass(a)
        for lg in (int(x) for x in a.sizes.split(",")):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--n",
                   str(1 << lg), "--compressed", "--runs", str(a.runs)]
            rc = subprocess.run(cmd + (["--out", a.out] if a.out else [])).returncode
            if rc != 0:
                print(f"bases_probe: size 2^{lg} ended with status {rc}; stopping", file=sys.stderr)
                return rc
        return 0
    if a.subset:
        a.subset_sizes = [int(x) for x in str(a.subset_sizes).split(",")]
        if a.n:
            return subset_pass(a)
        lg = int(a.sizes.split(",")[-1])  # one handle: the largest size given (default 2^20)
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--n", str(1 << lg),
               "--subset", "--subset-sizes", ",".join(map(str, a.subset_sizes)), "--count", str(a.count),
               "--runs", str(a.runs)] + (["--out", a.out] if a.out else [])
        return subprocess.run(cmd).returncode
    if a.wide:
        a.wide_types = [x for x in str(a.wide_types).split(",") if x]
        if a.n:
            return wide_pass(a)
        for lg in (int(x) for x in a.sizes.split(",")):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--n",
                   str(1 << lg), "--wide", "--wide-types", ",".join(a.wide_types), "--count", str(a.count),
                   "--runs", str(a.runs)]
            rc = subprocess.run(cmd + (["--out", a.out] if a.out else [])).returncode
            if rc != 0:
                print(f"bases_probe: size 2^{lg} ended with status {rc}; stopping", file=sys.stderr)
                return rc
        return 0
    if a.native:
        a.native_types = [x for x in str(a.native_types).split(",") if x]
        if a.n:
            return native_pass(a)
        for lg in (int(x) for x in a.sizes.split(",")):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--n",
                   str(1 << lg), "--native", "--native-types", ",".join(a.native_types), "--count", str(a.count),
                   "--runs", str(a.runs)]
            rc = subprocess.run(cmd + (["--out", a.out] if a.out else [])).returncode
            if rc != 0:
                print(f"bases_probe: size 2^{lg} ended with status {rc}; stopping", file=sys.stderr)
                return rc
        return 0
    if a.narrow:
        a.narrow_bits = [int(x) for x in str(a.narrow_bits).split(",")]
        a.narrow_widths = [int(x) for x in str(a.narrow_widths).split(",") if x]
        if a.n:
            return narrow_pass(a)
        for lg in (int(x) for x in a.sizes.split(",")):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--n",
                   str(1 << lg), "--narrow", "--narrow-bits", ",".join(map(str, a.narrow_bits)), "--narrow-widths",
                   ",".join(map(str, a.narrow_widths)), "--count", str(a.count), "--runs", str(a.runs)]
            rc = subprocess.run(cmd + (["--out", a.out] if a.out else [])).returncode
            if rc != 0:
                print(f"bases_probe: size 2^{lg} ended with status {rc}; stopping", file=sys.stderr)
                return rc
        return 0
    if a.n:
        return one_size(a)
    for lg in (int(x) for x in a.sizes.split(",")):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--n", str(1 << lg),
               "--levels", ",".join(map(str, a.levels)), "--count", str(a.count), "--runs", str(a.runs)]
        cmd += (["--c17"] if a.c17 else []) + (["--out", a.out] if a.out else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"bases_probe: size 2^{lg} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
