"""Guard-banded device buffers (csrc/host_ctx.h g_guard, csrc/host_guard.h): every launch path at the
smallest shapes that reach it, with every workspace buffer allocated at exactly its plan's size between
a 4 KiB and a 64 KiB band of a known byte.  After each call the result is compared bit-exact with the
closed form over P_i = (K0 + i STEP) G, then the bands are read back: a kernel that wrote past a
buffer, or relied on the slack a grown-and-never-shrunk buffer has in production, shows as a touched
band with the buffer's name, side and offset; a launch that left a word in one of the five buffers
the kernels keep all-zero between MSMs shows as a "zero" finding.  The module switches the mode on
for itself only (after msm_shutdown, and back off the same way), so the rest of the suite runs the
production allocator."""
import functools
import random

import numpy as np
import pytest

import msm_amd as M
from _closed_form import as_xy, scalar_dot
from oracle import oracle as O

pytestmark = pytest.mark.gpu

K0, STEP = 3, 5
NMAX = 32769
ALL_ONES = (1 << 256) - 1


@pytest.fixture(scope="module", autouse=True)
def guarded():
    L = M.load()
    try:
        L.msm_shutdown()
        M._test_guard(True)
        yield
    finally:
        L.msm_shutdown()
        M._test_guard(False)


# ---- inputs and expected values -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _all_points(n=NMAX):
    pts = M.gen_points(n, k0=K0, step=STEP)
    pts.setflags(write=False)
    return pts


def _pts(n):
    return _all_points()[:n] if n <= NMAX else _all_points(n)


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def _dpts(n):
    return _dev(_pts(n))


def _ks(idx):
    return K0 + STEP * np.asarray(idx, dtype=np.uint64)


def _expect(sc8, idx=None):
    """sum_i s_i P_idx[i] by the closed form ((sum s_i k_i) mod r) G; idx = 0 .. n-1 by default."""
    sc8 = np.asarray(sc8).reshape(-1, 8)
    ks = _ks(np.arange(sc8.shape[0]) if idx is None else idx)
    return O.scalar_mul(O.G, scalar_dot(ks, sc8) % O.R_ORDER)


def _expect_ints(vals, idx=None):
    ks = _ks(np.arange(len(vals)) if idx is None else idx)
    return O.scalar_mul(O.G, sum(int(k) * int(v) for k, v in zip(ks, vals)) % O.R_ORDER)


def _extend(w):
    full = np.zeros((w.shape[0], 8), np.uint32)
    full[:, 8 - w.shape[1]:] = w
    return full


CLASSES = ("mod_p", "full", "ones", "equal", "zero")


@functools.lru_cache(maxsize=None)
def _scalars(kind, n, seed=0):
    """[n, 8] wire scalars of one class: xorshift mod p; random 256-bit (entries in the overflow
    window); every scalar 2^256 - 1 (every window non-zero, one bucket: the most entries and skew); all
    equal (the chain, lead and cross joins); all zero (an empty sorted list)."""
    if kind == "mod_p":
        w = M.gen_scalars(n, seed=1000 + n + seed)
    elif kind == "full":
        w = np.random.default_rng(n + seed).integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    elif kind == "ones":
        w = np.full((n, 8), 0xFFFFFFFF, np.uint32)
    elif kind == "equal":
        w = np.tile(M.gen_scalars(1, seed=77 + seed), (n, 1))
    else:
        w = np.zeros((n, 8), np.uint32)
    w = np.ascontiguousarray(w)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _expected(kind, n, seed=0):
    return _expect(_scalars(kind, n, seed))


# ---- the helper every case goes through ---------------------------------------------------------
def _clean(note=None):
    hits = M._test_guard_check()
    assert not hits, "; ".join(
        f"{h['buffer']} (slot {h['slot']}) {h['side']}: {h['count']} touched, offsets {h['first']}..{h['last']}"
        for h in hits) + f" after {note!r}"


def checked(fn, expected, note=None, release=True):
    """Release the workspaces (so every buffer is allocated at this call's own size), run fn, compare
    with the expected value, and require an empty guard report."""
    if release:
        M._test_guard_release()
    got = fn()
    assert got == expected, note
    _clean(note)


def _rows(res):
    return [as_xy(r) for r in res]


# ---- self-test: first in the module -------------------------------------------------------------
def test_planted_bytes_are_reported_once():
    n = 257
    sc = _scalars("mod_p", n)
    checked(lambda: M.compute_msm_wire(_pts(n), sc), _expected("mod_p", n), "self-test MSM")
    assert "sorted_entry" in M._test_guard_names() and "h_out" in M._test_guard_names()
    with pytest.raises(M.MsmError) as e:  # the layouts never mix: no switching while buffers are held
        M._test_guard(False)
    assert e.value.code == -1
    assert M._test_guard(True) is True
    plants = [("sorted_entry", 0, dict(side="back", first=0, last=0, count=1)),
              ("buckets", 1, dict(side="back", first=65535, last=65535, count=1)),
              ("lead_flag", 2, dict(side="front", first=-1, last=-1, count=1)),
              ("colsum", 3, dict(side="zero", first=4, last=4, count=1))]
    for buf, where, want in plants:
        M._test_guard_plant(buf, where, slot=0)
        want = dict(want, buffer=buf, slot=0, device=M.device_ordinals()[0])
        assert M._test_guard_check() == [want], (buf, where)
        assert M._test_guard_check() == [], (buf, where)
    # several at once, two of them in one band
    M._test_guard_plant("err", 0)
    M._test_guard_plant("err", 1)
    M._test_guard_plant("digits", 2)
    got = {(h["buffer"], h["side"]): (h["first"], h["last"], h["count"]) for h in M._test_guard_check()}
    assert got == {("err", "back"): (0, 65535, 2), ("digits", "front"): (-1, -1, 1)}
    assert M._test_guard_check() == []
    # the repaired slot computes on
    checked(lambda: M.compute_msm_wire(_pts(n), sc), _expected("mod_p", n), "after the plants", release=False)
    with pytest.raises(M.MsmError):  # a buffer this plan did not allocate has no guard to plant in
        M._test_guard_plant("partials", 0)


# ---- per-call entries, 8-word scalars -----------------------------------------------------------
# (n, window_size, run_length); 0 = auto.  Every n and every width at least twice; run_length = 1 with
# the largest n of each width (the most runs: lead_*, g_head, g_hkey, g_tkey, skew_list at their largest).
COMBOS = [
    (1, 0, 0), (2, 0, 0), (63, 0, 0), (64, 0, 4), (65, 0, 0), (255, 0, 1), (256, 0, 0), (257, 0, 0), (1023, 0, 4),
    (4097, 0, 0), (16383, 0, 0), (16384, 0, 0), (16385, 0, 4), (32769, 0, 0), (32769, 0, 1),
    (1, 4, 0), (2, 4, 0), (65, 4, 4), (255, 4, 0), (257, 4, 1),
    (63, 8, 0), (256, 8, 4), (1023, 8, 0), (4097, 8, 1),
    (255, 12, 0), (4097, 12, 4), (16384, 12, 1),
    (64, 13, 0), (16383, 13, 0), (16385, 13, 1),
    (1, 16, 0), (1023, 16, 4), (16384, 16, 0), (32769, 16, 1),
    (2, 17, 0), (257, 17, 0), (16385, 17, 1),
    (65, 20, 0), (4097, 20, 0), (16383, 20, 1),
]


def test_combos_cover_the_list():
    ns = [n for n, _, _ in COMBOS]
    cs = [c for _, c, _ in COMBOS]
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 4097, 16383, 16384, 16385, 32769):
        assert ns.count(n) >= 2, n
    for c in (0, 4, 8, 12, 13, 16, 17, 20):
        assert cs.count(c) >= 2, c
        assert (max(n for n, cc, _ in COMBOS if cc == c), c, 1) in COMBOS, c
    assert all(n <= 600 for n, c, _ in COMBOS if c == 4)


@pytest.mark.parametrize("n,c,k", COMBOS)
def test_per_call_host_and_device(n, c, k):
    pts, dp = _pts(n), _dpts(n)
    for kind in CLASSES:
        sc, exp = _scalars(kind, n), _expected(kind, n)
        checked(lambda: M.compute_msm_wire(pts, sc, window_size=c or None, run_length=k or None), exp,
                ("host", kind, n, c, k))
        ds = _dev(sc)
        checked(lambda: M.compute_msm_device(dp, ds, n, window_size=c or None, run_length=k or None), exp,
                ("device", kind, n, c, k))


@pytest.mark.parametrize("n", [257, 4097])
@pytest.mark.parametrize("count", [1, 2, 3, 5, 9])
def test_many_device(n, count):
    """4 and 8 MSMs per launch, the last launch padded."""
    kinds = [CLASSES[j % len(CLASSES)] for j in range(count)]
    dss = [_dev(_scalars(kd, n, j)) for j, kd in enumerate(kinds)]
    exp = [_expected(kd, n, j) for j, kd in enumerate(kinds)]
    checked(lambda: _rows(M.compute_msm_many_device([_dpts(n)] * count, dss, n)), exp, ("many_device", n, count))


@pytest.mark.parametrize("n,count", [(257, 3), (4097, 5)])
def test_shared_device(n, count):
    dss = [_dev(_scalars("mod_p", n, j)) for j in range(count)]
    exp = [_expected("mod_p", n, j) for j in range(count)]
    checked(lambda: _rows(M.compute_msm_shared_device(_dpts(n), dss, n)), exp, ("shared_device", n, count))
    checked(lambda: _rows(M.compute_msm_shared(_pts(n), [_scalars("mod_p", n, j) for j in range(count)])), exp,
            ("shared", n, count))


@pytest.mark.parametrize("ranges", [((0, 5), (5, 12), (12, None)), ((0, 11, 2), (11, None, 2))])
@pytest.mark.parametrize("kind", ["mod_p", "full"])
def test_partial_window_ranges(ranges, kind):
    """Whole- and half-window ranges at (n = 1000, c = 10): the partials of a partition join to the MSM."""
    n, c = 1000, 10
    wm = M.window_count(c)
    rs = [(r[0], (wm * (2 if len(r) > 2 else 1)) if r[1] is None else r[1]) + tuple(r[2:]) for r in ranges]
    sc = _scalars(kind, n)
    parts = []
    for r in rs:
        M._test_guard_release()
        parts.append(M.compute_msm_partial(_pts(n), sc, window_size=c, windows=r))
        _clean(("partial", r))
    assert M.combine_partials(np.stack(parts)) == _expected(kind, n)
    ds = _dev(sc)
    parts = []
    for r in rs:
        M._test_guard_release()
        parts.append(M.compute_msm_device_partial(_dpts(n), ds, n, window_size=c, windows=r))
        _clean(("device partial", r))
    assert M.combine_partials(np.stack(parts)) == _expected(kind, n)


@pytest.mark.parametrize("n", [65537, 3 * (1 << 17) + 2])
def test_large_host_uploads(n):
    """65,537: two upload pieces, the second of one point.  3 * 2^17 + 2: the split path with a short
    padded last slice (host_sc, host_pts)."""
    sc = _scalars("mod_p", n)
    checked(lambda: M.compute_msm_wire(_pts(n), sc), _expected("mod_p", n), ("host", n))


# ---- handles ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _index_lists(n):
    lists = {"one": np.array([n - 1], np.uint32), "reversed": np.arange(n, dtype=np.uint32)[::-1].copy(),
             "same": np.full(max(n, 2), n // 2, np.uint32)}
    if n == 257:
        lists["longer"] = np.random.default_rng(5).integers(0, n, size=1000).astype(np.uint32)
    return lists


def _handle_cases(h, n, c):
    kw = dict(window_size=c or None)
    sc = _scalars("full", n)
    checked(lambda: h.compute(sc, **kw), _expected("full", n), ("compute", n, c))
    d = _dev(_scalars("mod_p", n))
    checked(lambda: h.compute_device(d, **kw), _expected("mod_p", n), ("compute_device", n, c))
    kinds = ("ones", "mod_p", "equal")
    checked(lambda: _rows(h.compute_many([_scalars(kd, n) for kd in kinds], **kw)), [_expected(kd, n) for kd in kinds],
            ("compute_many", n, c))
    if n > 1:
        first = n // 2
        for m in sorted({1, n - first}):
            s = _scalars("full", m, 9)
            checked(lambda: h.compute_subset(s, first=first, **kw), _expect(s, np.arange(first, first + m)),
                    ("range", n, c, first, m))
            ds = _dev(s)
            checked(lambda: h.compute_subset_device(ds, first=first, **kw), _expect(s, np.arange(first, first + m)),
                    ("range device", n, c, first, m))
    for name, idx in _index_lists(n).items():
        s = _scalars("full" if name != "same" else "mod_p", len(idx), 11)
        checked(lambda: h.compute_subset(s, indices=idx, **kw), _expect(s, idx), ("indexed", name, n, c))
        ds, di = _dev(s), _dev(idx)
        checked(lambda: h.compute_subset_device(ds, indices=di, **kw), _expect(s, idx), ("indexed device", name, n, c))


def _open(n, levels, c=0):
    """A handle from device points, its records and the preparation's error word checked at once."""
    M._test_guard_release()
    h = M.Bases.from_device(_dpts(n), n, levels=levels, window_size=c or None)
    _clean(("from_device", n, levels, c))
    return h


@pytest.mark.parametrize("n", [1, 2, 257, 4097])
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_handles(levels, n):
    with _open(n, levels) as h:
        _handle_cases(h, n, 0)


@pytest.mark.parametrize("levels,n,c", [(1, 257, 17), (2, 4097, 17), (3, 257, 17), (1, 4097, 20), (2, 257, 20)])
def test_handles_32_bit_digit_codes(levels, n, c):
    """Widths 17 and 20 take the 32-bit digit codes (a levels > 1 handle is made for its width)."""
    with _open(n, levels, c if levels > 1 else 0) as h:
        _handle_cases(h, n, c)


def test_handle_from_host_points():
    n = 257
    M._test_guard_release()
    with M.Bases.from_wire(_pts(n), levels=2) as h:
        _clean("from_wire")
        sc = _scalars("mod_p", n)
        checked(lambda: h.compute(sc), _expected("mod_p", n), "from_wire compute")


# ---- narrow scalars -----------------------------------------------------------------------------
def _narrow_vals(b, n, top):
    if top:
        return [(1 << b) - 1] * n
    rnd = random.Random(100 * b + n)
    return [rnd.getrandbits(b) for _ in range(n)]


def _narrow_cases(h, b, n):
    for top in (False, True):
        vals = _narrow_vals(b, n, top)
        w = M.scalars_to_wire(vals, scalar_bits=b)
        exp = _expect_ints(vals)
        checked(lambda: h.compute(w, scalar_bits=b), exp, ("narrow", b, n, top))
        d = _dev(w)
        checked(lambda: h.compute_device(d, scalar_bits=b), exp, ("narrow device", b, n, top))


@pytest.fixture(scope="module")
def handles(guarded):
    hs = {(lv, n): _open(n, lv) for lv, n in ((1, 1), (1, 257), (1, 4097), (2, 1), (2, 257), (2, 4097), (1, NMAX))}
    yield hs
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("n", [1, 257, 4097])
@pytest.mark.parametrize("b", [1, 2, 3, 8, 12, 16, 31, 32, 33, 64, 65, 128, 253])
def test_narrow(handles, b, n):
    _narrow_cases(handles[1, n], b, n)


@pytest.mark.parametrize("n", [1, 257, 4097])
@pytest.mark.parametrize("b", [8, 64, 253])
def test_narrow_on_a_folded_handle(handles, b, n):
    _narrow_cases(handles[2, n], b, n)


# ---- the dense-bucket accumulation --------------------------------------------------------------
def _dense_plan(n, b, c=0, nm=1, pipelined=False):
    p = M._test_dense_plan(n, nm, pipelined, b, c)
    assert p["dense"] == 1, (n, b, c, nm, p)
    return p


def _bits_wire(vals, b):
    return M.scalars_to_wire([int(v) for v in vals], scalar_bits=b)


# (b = 8, n = 4097) is dense at width 4 (three 3-bit windows, ~1,000 entries per bucket), not at the
# auto width: the case runs where the plan confirms the dense path.
@pytest.mark.parametrize("b,n,c", [(1, 1024, 0), (3, 1025, 0), (8, 4097, 4), (8, 32769, 9)])
def test_dense(handles, b, n, c):
    _dense_plan(n, b, c)
    h = handles[1, NMAX]
    rnd = random.Random(b * n)
    for vals in ([rnd.getrandbits(b) for _ in range(n)], [(0xA5 & ((1 << b) - 1)) or 1] * n):
        w = _bits_wire(vals, b)
        exp = _expect_ints(vals)
        checked(lambda: h.compute_subset(w, window_size=c or None, scalar_bits=b), exp, ("dense", b, n, c))
        d = _dev(w)
        checked(lambda: h.compute_subset_device(d, window_size=c or None, scalar_bits=b), exp, ("dense device", b, n, c))


def test_dense_one_bucket_of_more_partials_than_fold_lanes(handles):
    """All-equal bytes at n = 32,769, width 9: one bucket per window, 128 unit partials each."""
    n, b, c = NMAX, 8, 9
    p = _dense_plan(n, b, c)
    assert n // (64 * p["E"]) > 64
    w = np.full((n, 1), 0xA5, np.uint32)
    checked(lambda: handles[1, NMAX].compute(w, window_size=c, scalar_bits=b), _expect_ints([0xA5] * n), "all-equal bytes")


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_dense_bucket_of_one_segment(handles, delta):
    """A bucket of exactly 64 E - 1, 64 E and 64 E + 1 entries (b = 1: the ones are one bucket)."""
    n = 1024
    k = 64 * _dense_plan(n, 1)["E"] + delta
    vals = [1] * k + [0] * (n - k)
    random.Random(k).shuffle(vals)
    w = _bits_wire(vals, 1)
    checked(lambda: handles[1, 4097].compute_subset(w, scalar_bits=1), _expect_ints(vals), ("segment", k))
    d = _dev(w)
    checked(lambda: handles[1, 4097].compute_subset_device(d, scalar_bits=1), _expect_ints(vals), ("segment device", k))


def test_dense_many_and_indexed(handles):
    n = 4097
    _dense_plan(n, 1, 0, 4, True)
    rnd = random.Random(8)
    vecs = [[rnd.getrandbits(1) for _ in range(n)] for _ in range(5)]
    vecs[2] = [0] * n
    ws = [_bits_wire(v, 1) for v in vecs]
    checked(lambda: _rows(handles[1, n].compute_many(ws, scalar_bits=1)), [_expect_ints(v) for v in vecs], "dense many")
    m = 2048
    _dense_plan(m, 1)
    idx = np.random.default_rng(9).integers(0, n, size=m).astype(np.uint32)
    idx[2:12] = 7
    w = ws[0][:m]
    checked(lambda: handles[1, n].compute_subset(w, indices=idx, scalar_bits=1), _expect_ints(vecs[0][:m], idx),
            "dense indexed")
    dw, di = _dev(w), _dev(idx)
    checked(lambda: handles[1, n].compute_subset_device(dw, indices=di, scalar_bits=1),
            _expect_ints(vecs[0][:m], idx), "dense indexed device")


# ---- native scalar types ------------------------------------------------------------------------
def _ndev(a, lead):
    """A host array's bytes on the device, `lead` bytes past a 16-byte boundary."""
    import torch

    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.zeros(raw.size + 16 + lead, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[16 + lead:] = torch.from_numpy(raw.copy())
    return buf[16 + lead:]


@pytest.mark.parametrize("m", [1, 7, 8, 9, 1025])
def test_native_bitmap(handles, m):
    rnd = random.Random(m)
    bits = [1] * m if m < 8 else [rnd.getrandbits(1) for _ in range(m)]
    a = M.scalars_to_native(bits, "bit")
    h = handles[1, 4097]
    checked(lambda: h.compute_subset(a, m=m, scalar_type="bit"), _expect_ints(bits), ("bitmap", m))
    d = _ndev(a, 4)
    checked(lambda: h.compute_subset_device(d, m=m, scalar_type="bit"), _expect_ints(bits), ("bitmap device", m))


@pytest.mark.parametrize("ty", ["u8", "i8", "u16", "i16", "u32", "i32", "u64", "i64"])
def test_native_types(handles, ty):
    """m odd, the type's extremes among the values; the device vector starts one element past a 16-byte
    boundary -- or 4 bytes past it for the types of fewer, the least offset the entry takes (it reads
    whole words)."""
    e = M.SCALAR_TYPES[ty][2]
    m = 1025
    lo, hi = (-(1 << (e - 1)), (1 << (e - 1)) - 1) if ty[0] == "i" else (0, (1 << e) - 1)
    rnd = random.Random(e + (ty[0] == "i"))
    vals = [rnd.randint(lo, hi) for _ in range(m)]
    vals[:6] = [lo, hi, 0, 1, hi, lo]
    vals[-1] = lo if lo < 0 else hi
    a = M.scalars_to_native(vals, ty)
    h = handles[1, 4097]
    checked(lambda: h.compute_subset(a, scalar_type=ty), _expect_ints(vals), ("native", ty))
    d = _ndev(a, max(e // 8, 4))
    checked(lambda: h.compute_subset_device(d, m=m, scalar_type=ty), _expect_ints(vals), ("native device", ty))


# ---- error paths: the slot is left clean --------------------------------------------------------
def _raises(code, fn, note):
    with pytest.raises(M.MsmError) as e:
        fn()
    assert e.value.code == code, note
    _clean(note)


def test_error_paths_leave_guards_and_invariants_clean(handles):
    n = 257
    good, exp = _scalars("mod_p", n), _expected("mod_p", n)
    dgood = _dev(good)

    def after(note):
        checked(lambda: M.compute_msm_device(_dpts(n), dgood, n), exp, ("after", note), release=False)

    bad_coord = _pts(n).copy()
    bad_coord[100, 0:8] = O.int_to_be_words(O.P)           # x = p
    bad_z = _pts(n).copy()
    bad_z[n - 1, 24:32] = 0                                  # z = 0
    for name, pts, code in (("coordinate >= p", bad_coord, -3), ("z = 0", bad_z, -4)):
        M._test_guard_release()
        _raises(code, lambda: M.compute_msm_wire(pts, good), name)
        after(name)
        dp = _dev(pts)
        _raises(code, lambda: M.compute_msm_device(dp, dgood, n), name + " (device)")
        after(name + " (device)")
        # a bad member in a pipelined call
        _raises(code, lambda: M.compute_msm_many_device([_dpts(n), dp, _dpts(n)], [dgood] * 3, n), name + " (pipelined)")
        after(name + " (pipelined)")
        assert _rows(M.compute_msm_many_device([_dpts(n)] * 3, [dgood] * 3, n)) == [exp] * 3
        _clean(name + " (pipelined, next call)")
        _raises(code, lambda: M.Bases.from_device(dp, n, levels=2), name + " (handle)")

    h = handles[1, n]
    idx = np.arange(n, dtype=np.uint32)
    idx[n // 2] = n                                          # one past the handle's last base
    di = _dev(idx)
    M._test_guard_release()
    _raises(-1, lambda: h.compute_subset_device(dgood, indices=di), "bad device index")
    checked(lambda: h.compute_device(dgood), exp, "after a bad device index", release=False)
    _raises(-1, lambda: h.compute_subset_many_device([dgood, dgood], indices=[_dev(np.arange(n, dtype=np.uint32)), di]),
            "bad device index (pipelined)")
    checked(lambda: h.compute_device(dgood), exp, "after a bad device index (pipelined)", release=False)

    b = 12
    vals = _narrow_vals(b, n, False)
    w = M.scalars_to_wire(vals, scalar_bits=b)
    bad = w.copy()
    bad[n - 1, 0] |= 1 << b                                  # a bit at scalar_bits
    dbad, dw = _dev(bad), _dev(w)
    M._test_guard_release()
    _raises(-1, lambda: h.compute_device(dbad, scalar_bits=b), "narrow excess bit")
    checked(lambda: h.compute_device(dw, scalar_bits=b), _expect_ints(vals), "after a narrow excess bit", release=False)
    _raises(-1, lambda: h.compute_many_device([dw, dbad, dw], scalar_bits=b), "narrow excess bit (pipelined)")
    checked(lambda: _rows(h.compute_many_device([dw] * 3, scalar_bits=b)), [_expect_ints(vals)] * 3,
            "after a narrow excess bit (pipelined)", release=False)


# ---- production growth order --------------------------------------------------------------------
def test_growth_order_small_large_small(handles):
    """No release between the calls: a buffer sized by the large call serves the small one after it, the
    state the rest of the suite runs in (grown on demand, never shrunk)."""
    M._test_guard_release()
    for n in (257, NMAX, 257, 1, 4097):
        for kind in ("mod_p", "ones", "zero"):
            sc = _scalars(kind, n)
            checked(lambda: M.compute_msm_wire(_pts(n), sc), _expected(kind, n), ("growth host", n, kind), release=False)
            ds = _dev(sc)
            checked(lambda: M.compute_msm_device(_dpts(n), ds, n), _expected(kind, n), ("growth device", n, kind),
                    release=False)
    h = handles[1, 4097]
    M._test_guard_release()
    for m in (1, 4097, 1, 257):
        s = _scalars("full", m, 21)
        idx = np.random.default_rng(m).integers(0, 4097, size=m).astype(np.uint32)
        checked(lambda: h.compute_subset(s, indices=idx), _expect(s, idx), ("growth indexed", m), release=False)
        first = 4097 - m
        checked(lambda: h.compute_subset(s, first=first), _expect(s, np.arange(first, 4097)), ("growth range", m),
                release=False)
    hb = handles[1, NMAX]
    M._test_guard_release()
    for b, n, c in ((1, 1024, 0), (8, NMAX, 9), (1, 1024, 0), (3, 1025, 0)):
        _dense_plan(n, b, c)
        rnd = random.Random(n + b)
        vals = [rnd.getrandbits(b) for _ in range(n)]
        w = _bits_wire(vals, b)
        checked(lambda: hb.compute_subset(w, window_size=c or None, scalar_bits=b), _expect_ints(vals),
                ("growth dense", b, n, c), release=False)
