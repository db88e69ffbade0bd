"""Poisoned device buffers (csrc/host_ctx.h g_guard_word, msm_test_guard_fill / _poison / _peek): every
launch path at one or two of its smallest shapes, with every guarded allocation filled with a non-zero
word instead of zero.  Zero is the neutral value of nearly all the integer state the kernels keep -- no
entry, an empty count, a clear flag, key 0, the additive identity of an Fr sum -- so a kernel that reads
a word its launch never wrote is invisible on zero-filled buffers; on poisoned ones it computes a wrong
result or touches a guard band.  The whole module runs once per fill word: as an entry word 1 is record 0
negated and 3 is record 1 negated, as a count or key they differ.

Every case goes through `both`: `checked` releases the workspaces (every buffer allocated fresh, poisoned,
at the call's own size), runs the call, compares bit-exact with the closed form over P_i = (K0 + i STEP) G
and requires an empty guard report; `replayed` overwrites the payloads again (msm_test_guard_poison: no
release, the cached graph is replayed on a workspace that holds nothing of the launch before it) and makes
the same two assertions.  The references are test_gpu_guard.py's.

The `zero` scalar class gives an empty sorted list (M = 0).  What the launch then reads: k_accumulate has
no live run -- it loads the total and stores lead_open[wg] = 0, cross_key stays unwritten --;
k_bucket_reduce_1 finds bucket_start equal over every chunk and stores identities without probing
cross_key; k_red2_groups leaves every (empty) window's red_G unwritten, and k_red2_terms / k_bucket_reduce_2
write identity terms from the windows' emptiness alone, reading neither red_G nor red_U / red_T."""
import functools
import random

import numpy as np
import pytest

import _red_check as RK
import msm_amd as M
import test_gpu_acc_chains as AC
import test_gpu_guard as G
import test_gpu_lifetime as TL
from _closed_form import as_xy
from oracle import oracle as O

pytestmark = pytest.mark.gpu

R = O.R_ORDER
RR = 1 << 256
K0, STEP = G.K0, G.STEP
TA, TB = 11, 7          # the per-point paths' targets: output i is (TA + i TB) G
OFF = 150               # combine's second side: B_i = P_(OFF + i)
NSRC = 300              # the per-point paths' source handle
FILLS = (1, 3)


@pytest.fixture(scope="module", autouse=True, params=FILLS, ids=[f"fill{w}" for w in FILLS])
def poisoned(request):
    L = M.load()
    try:
        L.msm_shutdown()
        M._test_guard(True)
        M._test_guard_fill(request.param)
        yield request.param
    finally:
        M._test_guard_fill(0)
        M._test_vector_slab(0)
        M._test_vector_group(0)
        L.msm_shutdown()
        M._test_guard(False)


# ---- the helpers every case goes through --------------------------------------------------------
def _same(got, exp):
    if isinstance(exp, np.ndarray):
        return isinstance(got, np.ndarray) and got.shape == exp.shape and np.array_equal(got, exp)
    return got == exp


def checked(fn, expected, note=None, release=True):
    """Release (so that every buffer is allocated fresh, poisoned, at this call's own size), run, compare
    bit-exact, and require an empty guard report."""
    if release:
        M._test_guard_release()
    got = fn()
    assert _same(got, expected), note
    G._clean(note)


def replayed(fn, expected, note=None):
    """The same call again on re-poisoned buffers: nothing released, the cached graph replayed."""
    M._test_guard_poison()
    got = fn()
    assert _same(got, expected), ("replayed", note)
    G._clean(("replayed", note))


def both(fn, expected, note=None):
    checked(fn, expected, note)
    replayed(fn, expected, note)


def _raises(code, fn, note):
    with pytest.raises(M.MsmError) as e:
        fn()
    assert e.value.code == code, note
    G._clean(note)


def _k(i):
    return K0 + STEP * i


@functools.lru_cache(maxsize=None)
def _gp(m, k0, step):
    """Wire records of (k0 + i step) G, i < m."""
    pts = M.gen_points(m, k0=k0, step=step)
    pts.setflags(write=False)
    return pts


def _target(m):
    return _gp(m, TA, TB)


def _lift(s, i):
    """s + j r for every third i, below 2^256: the same point from an unreduced scalar."""
    s %= R
    if i % 3 == 2:
        s += (1 + i % 27) * R
    assert s < RR
    return s


def _words(ints):
    return O.ints_to_be_words([int(v) for v in ints])


def _wire_of(ks):
    """Wire records of k G for every k."""
    return O.affine_to_wire([O.c_scalar_mul(O.G, int(k) % R) for k in ks])


def _bytes_dev(a):
    """A host array's bytes on the device: a uint8 tensor [n, bytes per element]."""
    import torch

    raw = np.ascontiguousarray(a).view(np.uint8).reshape(np.asarray(a).shape[0], -1)
    return torch.from_numpy(raw.copy()).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


# ---- self-test: first in the module -------------------------------------------------------------
def test_fill_is_there_and_stays_where_no_kernel_writes(poisoned):
    """g_head is touched only by skewed workgroups (host_launch.h): after one unskewed MSM on fresh buffers,
    and again after msm_test_guard_poison, it holds nothing but the fill word; err, a zero invariant, holds
    zeros whatever the word."""
    name = "unskewed_k1"  # the accumulation catalogue's shape without a skewed workgroup, by its model
    s, inp, lay, res, exp = AC._case(name)
    assert not res.skewed and not res.second_pass
    dp, ds = AC._dpts(s.n), AC._dev(inp["scalars"])
    run = lambda: M.compute_msm_device(dp, ds, s.n, window_size=s.c, run_length=s.K)
    checked(run, exp, "self-test MSM")
    assert M._test_acc_state([], [])["skewed"] == []
    words = lay.nruns * 36  # every live run's staging record
    head = M._test_guard_peek("g_head", 0, words)
    assert head.dtype == np.uint32 and head.tolist() == [poisoned] * words
    assert M._test_guard_peek("err", 0, 4).tolist() == [0] * 4
    assert M._test_guard_peek("skew_list", 0, 1).tolist() == [0]
    tail = M._test_guard_peek("h_out", 0, 8)       # the first window term's X: written by the launch
    M._test_guard_poison()
    assert M._test_guard_peek("g_head", 0, words).tolist() == [poisoned] * words
    assert M._test_guard_peek("h_out", 0, 8).tolist() == [poisoned] * 8 != tail.tolist()
    assert M._test_guard_peek("sorted_entry", 0, 4).tolist() == [poisoned] * 4
    assert M._test_guard_peek("skew_list", 1, 1).tolist() == [poisoned]
    assert M._test_guard_peek("err", 0, 4).tolist() == [0] * 4            # left out of the pass
    assert M._test_guard_peek("skew_list", 0, 1).tolist() == [0]
    assert M._test_guard_peek("colsum", 0, 2).tolist() == [0, 0]
    G._clean("after the poison pass")
    with pytest.raises(M.MsmError) as e:                                   # a range past the payload
        M._test_guard_peek("err", 3, 2)
    assert e.value.code == -1
    with pytest.raises(M.MsmError):                                        # a buffer this plan did not allocate
        M._test_guard_peek("partials", 0, 1)
    with pytest.raises(M.MsmError):                                        # a handle's records: not a slot's
        M._test_guard_peek("bases_rec", 0, 1)
    assert M._test_guard_fill(poisoned) == poisoned
    replayed(run, exp, "self-test MSM")
    assert M._test_guard_peek("g_head", 0, words).tolist() == [poisoned] * words


# ---- per-call entries ---------------------------------------------------------------------------
KINDS = ("mod_p", "ones", "equal", "zero")


@pytest.mark.parametrize("k", [0, 1], ids=["kauto", "k1"])
@pytest.mark.parametrize("c", [0, 4, 17], ids=["cauto", "c4", "c17"])
@pytest.mark.parametrize("n", [1, 65, 257, 4097])
def test_per_call_host_and_device(n, c, k):
    pts, dp = G._pts(n), G._dpts(n)
    kw = dict(window_size=c or None, run_length=k or None)
    for kind in KINDS:
        sc, exp = G._scalars(kind, n), G._expected(kind, n)
        both(lambda: M.compute_msm_wire(pts, sc, **kw), exp, ("host", kind, n, c, k))
        ds = G._dev(sc)
        both(lambda: M.compute_msm_device(dp, ds, n, **kw), exp, ("device", kind, n, c, k))


@pytest.mark.parametrize("count", [2, 5])
def test_many_device(count):
    n = 257
    kinds = [KINDS[j % len(KINDS)] for j in range(count)]
    dss = [G._dev(G._scalars(kd, n, j)) for j, kd in enumerate(kinds)]
    exp = [G._expected(kd, n, j) for j, kd in enumerate(kinds)]
    both(lambda: G._rows(M.compute_msm_many_device([G._dpts(n)] * count, dss, n)), exp, ("many_device", count))


def test_shared_device():
    n, count = 257, 3
    dss = [G._dev(G._scalars("mod_p", n, j)) for j in range(count)]
    exp = [G._expected("mod_p", n, j) for j in range(count)]
    both(lambda: G._rows(M.compute_msm_shared_device(G._dpts(n), dss, n)), exp, "shared_device")
    both(lambda: G._rows(M.compute_msm_shared(G._pts(n), [G._scalars("mod_p", n, j) for j in range(count)])), exp,
         "shared")


@pytest.mark.parametrize("ranges", [((0, 5), (5, 12), (12, None)), ((0, 11, 2), (11, None, 2))], ids=["whole", "half"])
def test_partial_window_ranges(ranges):
    """One partition into whole-window ranges and one into half-window ranges at (n = 1000, c = 10): the
    partials join to the MSM."""
    n, c = 1000, 10
    wm = M.window_count(c)
    rs = [(r[0], (wm * (2 if len(r) > 2 else 1)) if r[1] is None else r[1]) + tuple(r[2:]) for r in ranges]
    sc = G._scalars("mod_p", n)
    ds = G._dev(sc)
    for entry in (lambda r: M.compute_msm_partial(G._pts(n), sc, window_size=c, windows=r),
                  lambda r: M.compute_msm_device_partial(G._dpts(n), ds, n, window_size=c, windows=r)):
        for again in (False, True):
            parts = []
            for r in rs:
                if again:
                    M._test_guard_poison()
                else:
                    M._test_guard_release()
                parts.append(entry(r))
                G._clean(("partial", r, again))
            assert M.combine_partials(np.stack(parts)) == G._expected("mod_p", n), (ranges, again)


def test_split_host_upload():
    """65,537 points: two upload pieces, the second of one point."""
    n = 65537
    sc = G._scalars("mod_p", n)
    both(lambda: M.compute_msm_wire(G._pts(n), sc), G._expected("mod_p", n), ("host", n))


# ---- handles ------------------------------------------------------------------------------------
def _open(n, levels, c=0):
    """A handle from device points, allocated over poison; its records are read whole by every MSM on it."""
    M._test_guard_release()
    h = M.Bases.from_device(G._dpts(n), n, levels=levels, window_size=c or None)
    G._clean(("from_device", n, levels, c))
    return h


@pytest.fixture(scope="module")
def handles(poisoned):
    hs = {(lv, n): _open(n, lv) for lv in (1, 2, 3) for n in (1, 257, 4097)}
    yield hs
    for h in hs.values():
        h.close()


def _native_vals(ty, n):
    rnd = random.Random(n + sum(map(ord, ty)))
    if ty == "bit":
        return [1] * n if n < 8 else [rnd.getrandbits(1) for _ in range(n)]
    e = M.SCALAR_TYPES[ty][2]
    lo, hi = (-(1 << (e - 1)), (1 << (e - 1)) - 1) if ty[0] == "i" else (0, (1 << e) - 1)
    vals = [rnd.randint(lo, hi) for _ in range(n)]
    vals[0], vals[-1] = (lo if lo < 0 else hi), hi
    return vals


def _wide_vals(ty, n):
    rnd = random.Random(7 * n + sum(map(ord, ty)))
    lo, hi = (-(1 << 127), (1 << 127) - 1) if ty == "i128" else (0, R - 1)
    vals = [rnd.randint(lo, hi) for _ in range(n)]
    vals[0], vals[-1] = lo if lo < 0 else hi, hi
    return vals


@pytest.mark.parametrize("n", [1, 257, 4097])
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_handles_full_width_and_subsets(handles, levels, n):
    h = handles[levels, n]
    sc = G._scalars("mod_p", n)
    both(lambda: h.compute(sc), G._expected("mod_p", n), ("compute", levels, n))
    d = G._dev(G._scalars("ones", n))
    both(lambda: h.compute_device(d), G._expected("ones", n), ("compute_device", levels, n))
    kinds = ("equal", "mod_p", "zero")
    both(lambda: G._rows(h.compute_many([G._scalars(kd, n) for kd in kinds])), [G._expected(kd, n) for kd in kinds],
         ("compute_many", levels, n))
    # subsets: a range, an index list, and index lists through the pipelined device entry
    first = n // 2
    m = n - first
    s = G._scalars("mod_p", m, 9)
    ds = G._dev(s)
    rng_exp = G._expect(s, np.arange(first, first + m))
    both(lambda: h.compute_subset(s, first=first), rng_exp, ("range", levels, n))
    both(lambda: h.compute_subset_device(ds, first=first), rng_exp, ("range device", levels, n))
    idx = np.random.default_rng(n + levels).integers(0, n, size=max(m, 2)).astype(np.uint32)
    idx[0], idx[-1] = n - 1, 0
    si = G._scalars("mod_p", len(idx), 11)
    dsi, di = G._dev(si), G._dev(idx)
    both(lambda: h.compute_subset(si, indices=idx), G._expect(si, idx), ("indexed", levels, n))
    both(lambda: h.compute_subset_device(dsi, indices=di), G._expect(si, idx), ("indexed device", levels, n))
    rev = np.ascontiguousarray(idx[::-1])
    both(lambda: G._rows(h.compute_subset_many_device([dsi, dsi, dsi], indices=[di, G._dev(rev), di])),
         [G._expect(si, idx), G._expect(si, rev), G._expect(si, idx)], ("indexed many device", levels, n))


@pytest.mark.parametrize("n", [1, 257, 4097])
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_handles_narrow_native_wide(handles, levels, n):
    h = handles[levels, n]
    for b in (1, 8, 33, 64, 253):
        vals = G._narrow_vals(b, n, False)
        vals[-1] = (1 << b) - 1
        w = M.scalars_to_wire(vals, scalar_bits=b)
        exp = G._expect_ints(vals)
        both(lambda: h.compute(w, scalar_bits=b), exp, ("narrow", levels, n, b))
        d = G._dev(w)
        both(lambda: h.compute_device(d, scalar_bits=b), exp, ("narrow device", levels, n, b))
    for ty in ("bit", "i8", "u64"):
        vals = _native_vals(ty, n)
        a = M.scalars_to_native(vals, ty)
        exp = G._expect_ints(vals)
        both(lambda: h.compute_subset(a, m=n, scalar_type=ty), exp, ("native", levels, n, ty))
        d = G._ndev(a, max(M.SCALAR_TYPES[ty][2] // 8, 4))
        both(lambda: h.compute_subset_device(d, m=n, scalar_type=ty), exp, ("native device", levels, n, ty))
    for ty in ("fr_mont", "i128"):
        vals = _wide_vals(ty, n)
        a = M.scalars_to_wide(vals, ty)
        exp = G._expect_ints(vals)
        both(lambda: h.compute(a, scalar_type=ty), exp, ("wide", levels, n, ty))
        d = _bytes_dev(a)
        both(lambda: h.compute_device(d, scalar_type=ty), exp, ("wide device", levels, n, ty))


@pytest.mark.parametrize("b,n,c", [(8, 4097, 4), (1, 1024, 0)])
def test_dense(handles, b, n, c):
    G._dense_plan(n, b, c)
    h = handles[1, 4097]
    rnd = random.Random(b * n)
    for vals in ([rnd.getrandbits(b) for _ in range(n)], [(0xA5 & ((1 << b) - 1)) or 1] * n):
        w = G._bits_wire(vals, b)
        exp = G._expect_ints(vals)
        both(lambda: h.compute_subset(w, window_size=c or None, scalar_bits=b), exp, ("dense", b, n, c))
        d = G._dev(w)
        both(lambda: h.compute_subset_device(d, window_size=c or None, scalar_bits=b), exp, ("dense device", b, n, c))


# ---- compressed creation and decompression ------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 257])
def test_compressed(n):
    pts = G._pts(n)
    xs = np.ascontiguousarray(pts[:, :8])
    both(lambda: M.decompress_points(xs, "subgroup"), np.array(pts), ("decompress", n))
    sc = G._scalars("mod_p", n)
    for levels in (1, 2):
        def created():
            with M.Bases.from_x(xs, levels=levels) as b:
                G._clean(("from_x", n, levels))
                return b.points(), b.compute(sc)
        M._test_guard_release()
        got_pts, got = created()
        assert np.array_equal(got_pts, pts) and got == G._expected("mod_p", n), (n, levels)
        G._clean(("from_x use", n, levels))
        M._test_guard_poison()
        got_pts, got = created()
        assert np.array_equal(got_pts, pts) and got == G._expected("mod_p", n), ("replayed", n, levels)
        G._clean(("from_x use, replayed", n, levels))


# ---- per-point paths ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def src(poisoned):
    M._test_guard_release()
    h = M.Bases.from_wire(G._pts(NSRC), levels=1)
    G._clean("per-point source")
    yield h
    h.close()


def _made(make):
    """A creating call's new handle, allocated over poison, read back whole."""
    def fn():
        with make() as nb:
            G._clean("a created handle")
            return nb.points()
    return fn


@functools.lru_cache(maxsize=None)
def _scale_scalars(m):
    """s_i with s_i P_i = (TA + i TB) G."""
    return _words([_lift((TA + i * TB) * pow(_k(i), -1, R), i) for i in range(m)])


@pytest.mark.parametrize("m", [1, 63, 65, 130])
def test_scale(src, m):
    sc, exp = _scale_scalars(m), np.array(_target(m))
    both(lambda: src.scale(sc), exp, ("scale", m))
    for levels in (1, 2):
        both(_made(lambda: src.scaled(sc, levels=levels)), exp, ("scaled", m, levels))
    idx = np.arange(m, dtype=np.uint32)[::-1].copy()
    rsc = np.ascontiguousarray(sc[::-1])
    both(lambda: src.scale(rsc, indices=idx), np.ascontiguousarray(exp[::-1]), ("scale indexed", m))
    d_out = G._dev(np.zeros((m, 32), np.uint32))

    def device():
        d_out.zero_()
        src.scale_device(G._dev(sc), d_out)
        return _host(d_out)
    both(device, exp, ("scale_device", m))


@functools.lru_cache(maxsize=None)
def _combine_scalars(m):
    """(b_i with A_i + b_i B_i = T_i G; a_i random and b'_i with a_i A_i + b'_i B_i = T_i G)."""
    rnd = random.Random(1001 + m)
    one = [_lift((TA + i * TB - _k(i)) * pow(_k(OFF + i), -1, R), i) for i in range(m)]
    as_ = [rnd.getrandbits(256) for _ in range(m)]
    bs = [_lift((TA + i * TB - a * _k(i)) * pow(_k(OFF + i), -1, R), i) for i, a in enumerate(as_)]
    return _words(one), _words(as_), _words(bs)


@pytest.mark.parametrize("m", [1, 63, 65, 130])
def test_combine_and_fold(src, m):
    one, as_, bs = _combine_scalars(m)
    exp = np.array(_target(m))
    forms = [("sum", dict(b_first=OFF, m=m), np.array(_gp(m, 2 * K0 + OFF * STEP, 2 * STEP))),
             ("one-sided", dict(b=one, b_first=OFF), exp),
             ("joint", dict(a=as_, b=bs, b_first=OFF), exp)]
    for what, kw, want in forms:
        both(lambda: src.combine(**kw), want, ("combine", what, m))
        both(_made(lambda: src.combined(levels=2, **kw)), want, ("combined", what, m))
    # one folding step of the first 2 m points: x_inv P_i + x P_(i + m)
    x = 0x1234567890ABCDEF << 100
    xi = pow(x, -1, R)
    M._test_guard_release()
    with M.Bases.from_wire(G._pts(2 * m), levels=1) as h2:
        both(_made(lambda: h2.fold(x, x_inv=xi, levels=1)), _wire_of(xi * _k(i) + x * _k(i + m) for i in range(m)),
             ("fold", m))


@functools.lru_cache(maxsize=None)
def _table_rows(k, m):
    """[m, k, 8] wire scalars with sum_j s_ij (K0 + j STEP) = TA + i TB mod r."""
    rnd = random.Random(1000 * k + m)
    ks = [_k(j) for j in range(k)]
    inv_last = pow(ks[-1], -1, R)
    out = []
    for i in range(m):
        row = [rnd.getrandbits(256) for _ in range(k - 1)]
        out += row + [_lift((TA + i * TB - sum(s * kj for s, kj in zip(row, ks))) * inv_last, i)]
    sc = _words(out).reshape(m, k, 8)
    sc.setflags(write=False)
    return sc


@pytest.mark.parametrize("k", [1, 8])
def test_fixed_tables(src, k):
    M._test_guard_release()
    with src.fixed_table(first=0, count=k, window_bits=8) as t:
        G._clean(("fixed_table", k))
        for m in (1, 65, 130):
            sc, exp = _table_rows(k, m), np.array(_target(m))
            both(lambda: t.mul(sc), exp, ("fixed mul", k, m))
            both(_made(lambda: t.mul_bases(sc, levels=2)), exp, ("fixed mul_bases", k, m))


@pytest.mark.parametrize("k", [9, 20])
def test_vector_tables(src, k):
    w = 5
    M._test_guard_release()
    with src.vector_table(first=0, count=k, window_bits=w) as t:
        G._clean(("vector_table", k))
        for m in (1, 65, 130):
            sc, exp = _table_rows(k, m), np.array(_target(m))
            both(lambda: t.mul(sc), exp, ("vector mul", k, m))
            both(_made(lambda: t.mul_bases(sc, levels=2)), exp, ("vector mul_bases", k, m))
        m = 130
        sc, exp = _table_rows(k, m), np.array(_target(m))
        try:
            M._test_vector_slab(1)  # the least partial buffer: the call is cut into several slabs
            assert M._test_vector_plan(k, w, 256, m, 8)["slab_rows"] < m
            both(lambda: t.mul(sc), exp, ("vector slabs", k))
        finally:
            M._test_vector_slab(0)
        try:
            M._test_vector_group(8)  # parts of 8 bases, the last one ragged
            plan = M._test_vector_plan(k, w, 256, m, 8)
            assert plan["G"] == 8 and plan["P"] >= 2
            both(lambda: t.mul(sc), exp, ("vector group", k))
        finally:
            M._test_vector_group(0)


# ---- Fr vectors ---------------------------------------------------------------------------------
FORMS = ("wire", "fr_mont")


def _enc(vals, form):
    """Residues as the 8-word elements of `form`: big-endian words of v, or little-endian words of v R."""
    if form == "wire":
        return _words(vals)
    buf = b"".join((int(v) * RR % R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u4").astype(np.uint32).reshape(-1, 8)


def _fr_dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def _fr_vec(m, seed):
    rnd = random.Random(100003 * seed + m)
    vals = [rnd.randrange(R) for _ in range(m)]
    vals[0], vals[-1] = R - 1, vals[-1] if m > 1 else R - 1
    return tuple(vals)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m", [1, 65, 257])
def test_fr_combine(m, form):
    a, b = _fr_vec(m, 1), _fr_vec(m, 2)
    x, y = 12345, _fr_vec(m, 3)
    exp = _enc([(x * u + w * v) % R for u, v, w in zip(a, b, y)], form)
    ea, eb, ey = _enc(a, form), _enc(b, form), _enc(y, form)
    both(lambda: M.fr_combine(ea, eb, x=x, y=ey, form=form), exp, ("fr_combine host", m, form))
    da, db, dy = _fr_dev(ea), _fr_dev(eb), _fr_dev(ey)
    both(lambda: _host(M.fr_combine(da, db, x=x, y=dy, form=form)).reshape(-1, 8), exp, ("fr_combine device", m, form))


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_fr_powers(n):
    g = 0x0123456789ABCDEF0123456789ABCDEF % R
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * g % R
    for form in FORMS:
        exp = _enc(pw, form)
        both(lambda: M.fr_powers(g, n, out_form=form), exp, ("fr_powers host", n, form))
        both(lambda: _host(M.fr_powers(g, n, out_form=form, device=0)).reshape(-1, 8), exp, ("fr_powers device", n, form))


def _dot_sizes():
    c = M._test_fr_constants()
    T, cap = c["threads"], c["dot_cap"]
    return [1, 65, T + 1, cap * T + 65]


@functools.lru_cache(maxsize=None)
def _dot_operands():
    """Two vectors of residues for the longest case (the shorter cases take their tails), as ints and as
    wire words."""
    n = _dot_sizes()[-1]
    out = []
    for seed in (5, 6):
        words = np.random.default_rng(seed).integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
        words[:, 0] &= 0x03FFFFFF  # below 2^250 < r: the big-endian words are the residues themselves
        raw = words.astype(">u4").tobytes()
        ints = [int.from_bytes(raw[32 * i:32 * i + 32], "big") for i in range(n)]
        words.setflags(write=False)
        out.append((tuple(ints), words))
    return out


@pytest.mark.parametrize("k", range(4))
def test_fr_dot(k):
    """With a zero fill k_fr_dot_final reading fr_part past the partials k_fr_dot_partial wrote could not be
    seen at all: the sum's identity is zero."""
    n = _dot_sizes()[k]
    (ai, aw), (bi, bw) = _dot_operands()
    ai, aw, bi, bw = ai[-n:], aw[-n:], bi[-n:], bw[-n:]
    s_ab, s_a = sum(u * v for u, v in zip(ai, bi)) % R, sum(ai) % R
    da, db = _fr_dev(aw), _fr_dev(bw)
    for fout in FORMS:
        both(lambda: M.fr_dot(da, db, out_form=fout), _enc([s_ab], fout)[0], ("fr_dot", n, fout))
        both(lambda: M.fr_dot(da, out_form=fout), _enc([s_a], fout)[0], ("fr_dot sum", n, fout))
    if n <= 4096:
        both(lambda: M.fr_dot(aw, bw), _enc([s_ab], "wire")[0], ("fr_dot host", n))


# ---- error paths, then a good call on the same poisoned state -----------------------------------
def test_error_paths_then_a_good_call(handles):
    n = 257
    good, exp = G._scalars("mod_p", n), G._expected("mod_p", n)
    dgood = G._dev(good)
    h = handles[1, n]

    def after(note):
        checked(lambda: M.compute_msm_device(G._dpts(n), dgood, n), exp, ("after", note), release=False)
        replayed(lambda: h.compute_device(dgood), exp, ("after, on the handle", note))

    bad_z = G._pts(n).copy()
    bad_z[n - 1, 24:32] = 0                                   # z = 0: a bad point at creation
    dbad = G._dev(bad_z)
    for levels in (1, 2):
        M._test_guard_release()
        _raises(-4, lambda: M.Bases.from_device(dbad, n, levels=levels), ("bad point at creation", levels))
        after(("bad point at creation", levels))
    M._test_guard_poison()
    _raises(-4, lambda: M.compute_msm_device(dbad, dgood, n), "bad point in a launch")
    after("bad point in a launch")

    vals = _wide_vals("fr_mont", n)                            # a device fr_mont >= r
    a = M.scalars_to_wide(vals, "fr_mont")
    bad = a.copy()
    bad[n // 2] = np.frombuffer(R.to_bytes(32, "little"), dtype="<u8")
    M._test_guard_release()
    _raises(-1, lambda: h.compute_device(_bytes_dev(bad), scalar_type="fr_mont"), "fr_mont >= r")
    checked(lambda: h.compute_device(_bytes_dev(a), scalar_type="fr_mont"), G._expect_ints(vals), "after fr_mont >= r",
            release=False)
    after("fr_mont >= r")
    frbad = _fr_dev(np.frombuffer((R - 1).to_bytes(32, "little") * 64 + R.to_bytes(32, "little"), dtype="<u4").reshape(-1, 8))
    M._test_guard_poison()
    _raises(-1, lambda: M.fr_dot(frbad, form="fr_mont"), "fr_dot of an fr_mont >= r")
    (ai, aw), _ = _dot_operands()
    replayed(lambda: M.fr_dot(_fr_dev(aw[:65])), _enc([sum(ai[:65]) % R], "wire")[0], "after fr_dot of an fr_mont >= r")

    b = 20                                                     # a native magnitude out of range
    rnd = random.Random(b)
    nvals = [rnd.randint(-(1 << b) + 1, (1 << b) - 1) for _ in range(n)]
    na = M.scalars_to_native(nvals, "i32")
    nbad = na.copy()
    nbad[n - 1] = 1 << b
    M._test_guard_release()
    _raises(-1, lambda: h.compute_device(G._ndev(nbad, 4), scalar_bits=b, scalar_type="i32"), "native out of range")
    checked(lambda: h.compute_device(G._ndev(na, 4), scalar_bits=b, scalar_type="i32"), G._expect_ints(nvals),
            "after native out of range", release=False)
    after("native out of range")


# ---- production growth order --------------------------------------------------------------------
def test_growth_order_small_large_small():
    """No release between the calls, the payloads poisoned again before each: a buffer sized by the large
    call serves the small one after it, and holds nothing the small call could mistake for its own."""
    M._test_guard_release()
    for n in (257, 4097, 257, 1, 65):
        for kind in ("mod_p", "ones", "zero"):
            sc = G._scalars(kind, n)
            replayed(lambda: M.compute_msm_wire(G._pts(n), sc), G._expected(kind, n), ("growth host", n, kind))
            ds = G._dev(sc)
            replayed(lambda: M.compute_msm_device(G._dpts(n), ds, n), G._expected(kind, n), ("growth device", n, kind))


# ---- state read-backs under poison --------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges_k1", "unskewed_k1"])
def test_accumulation_state(name):
    """cross_key, lead_open, the skew list and the bucket points against the model: the words a stale read
    would corrupt."""
    keys = AC._every_key(name)[:16]
    M._test_guard_release()
    AC._run_device(name)
    G._clean(name)
    AC._check_state(name, keys)
    M._test_guard_poison()
    AC._run_device(name)
    G._clean((name, "replayed"))
    AC._check_state(name, keys)


def test_reduction_state():
    name = "c13_groups"
    M._test_guard_release()
    RK.run_device(name)
    G._clean(name)
    RK.check_state(name)
    M._test_guard_poison()
    RK.run_device(name)
    G._clean((name, "replayed"))
    RK.check_state(name)


# ---- the lifetime sweep on poisoned buffers -----------------------------------------------------
def test_lifetime_sequence():
    """test_sequence_guarded's seed, with every payload overwritten between the steps: a step finds nothing
    of the step before it in the workspaces."""
    seed = TL.SEEDS[0]
    hits = []

    def after_step(i, rec):
        found = M._test_guard_check()
        if found and not hits:
            hits.append((i, found))
        M._test_guard_poison()

    M._test_guard_release()
    failure = TL.run_sequence(seed, TL.STEPS, after_step)
    assert failure is None, TL._message(seed, TL.STEPS, failure)
    assert not hits, TL._message(seed, TL.STEPS, (hits[0][0], f"guard bands written: {hits[0][1]}"))
    G._clean("lifetime sequence")
