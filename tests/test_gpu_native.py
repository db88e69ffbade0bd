"""GPU tests of native integer scalars on a resident-bases handle (include/msm.h MSM_FLAG_SCALAR_TYPE,
msm_amd.Bases.compute*(scalar_type=...)): the caller's own int8 .. uint64 arrays and bitmaps, negative
values included, bit-exact against the C oracle on the magnitudes zero-extended to 8 words over points
negated by hand where the value is negative -- never against another entry of the library."""
import ctypes
import functools
import random

import numpy as np
import pytest

import msm_amd as M
from _closed_form import as_xy
from _narrow_model import auto_width, edge_scalars
from oracle import oracle as O
from test_gpu_subset import _dev, _points

pytestmark = pytest.mark.gpu

TYPES = {"bit": 1, "u8": 8, "i8": 8, "u16": 16, "i16": 16, "u32": 32, "i32": 32, "u64": 64, "i64": 64}
N = 4097  # one past the recode workgroup's span: two workgroups, the second with one scalar; odd
# two workgroups and even (paired 4-B code stores), the second of 38 scalars: a ragged last lane of two for u8 /
# i8 and of six after one full lane for bit, full lanes for the two-per-lane types
N_EVEN = 4134
SIZES = (1, 2, 31, 33, 4095, N, N_EVEN)
WIDTHS = (None, 4, 13, 17)  # 17 takes the 32-bit digit codes


def _signed(ty):
    return ty[0] == "i"


def _limits(ty, b=None):
    """The least and greatest value of the type, or of magnitudes below 2^b."""
    e = TYPES[ty]
    lo, hi = (-(1 << (e - 1)), (1 << (e - 1)) - 1) if _signed(ty) else (0, (1 << e) - 1)
    if b is not None and b < e:
        lo, hi = max(lo, -((1 << b) - 1)), min(hi, (1 << b) - 1)
    return lo, hi


@functools.lru_cache(maxsize=None)
def _negated(n):
    """_points(n) with every point negated: x -> -x mod p, t -> -t mod p."""
    pts = _points(n).copy()
    for i in range(n):
        for j in (0, 2):
            v = O.be_words_to_int(pts[i, 8 * j: 8 * j + 8])
            pts[i, 8 * j: 8 * j + 8] = O.int_to_be_words((O.P - v) % O.P)
    pts.setflags(write=False)
    return pts


def _oracle(vals, pts, neg_pts):
    """sum v_i P_i by the oracle: |v_i| as 8-word scalars on the points, negated where v_i < 0."""
    neg = np.array([v < 0 for v in vals], dtype=bool)
    p = np.ascontiguousarray(np.where(neg[:, None], neg_pts, pts))
    return O.msm(p, O.ints_to_be_words([abs(v) for v in vals]), window=10, threads=8)


def _pack(vals, ty):
    """The array a typed call takes; a bitmap's pad bits are set, to show that they are ignored."""
    a = M.scalars_to_native(vals, ty)
    if ty == "bit" and len(vals) % 8:
        a[-1] |= (0xff << (len(vals) % 8)) & 0xff
    a.setflags(write=False)
    return a


def _ndev(a, lead=0):
    """A host array's bytes on the device (a uint8 tensor), `lead` bytes past a 512-byte boundary."""
    import torch

    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.zeros(raw.size + lead, dtype=torch.uint8, device="cuda")
    buf[lead:] = torch.from_numpy(raw.copy())
    return buf[lead:]


@functools.lru_cache(maxsize=None)
def _values(ty, m=N, seed=0, b=None):
    """m values of the type (magnitudes below 2^b): random ones, then (from m = 16) 0, +-1, the least
    and greatest value and the carry edges of every window of every width the tests run, under both
    signs; a single value is the least one (-2^(e-1) for a signed type)."""
    e = TYPES[ty]
    bb = e if b is None else b
    lo, hi = _limits(ty, b)
    rnd = random.Random(7000 + 131 * e + 17 * m + seed + (1000 if _signed(ty) else 0) + 7 * bb)
    vals = [rnd.randint(lo, hi) for _ in range(m)]
    if m >= 16:
        edges = {0, 1, lo, hi}
        for c in WIDTHS:
            for v in edge_scalars(bb, c or auto_width(m, bb, M.get_best_window_size(m))):
                edges.update(x for x in (v, -v) if lo <= x <= hi)
        if lo < 0:
            edges.add(-1)
        for i, v in enumerate(sorted(edges, key=lambda x: (abs(x), x))[:m - 10]):
            vals[10 + i] = v
    elif m == 1:
        vals[0] = lo if lo < 0 else hi
    return tuple(vals)


@functools.lru_cache(maxsize=None)
def _expected(ty, n=N, seed=0, b=None):
    return _oracle(_values(ty, n, seed, b), _points(n), _negated(n))


# ---- parity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
def test_parity_with_oracle(ty):
    for n in SIZES:
        vals, exp = _values(ty, n), _expected(ty, n)
        a = _pack(vals, ty)
        assert a.nbytes == -(-n * TYPES[ty] // 8)
        d = _ndev(a)
        with M.Bases.from_wire(_points(n), levels=1) as h:
            for c in WIDTHS:
                assert h.compute(a, window_size=c, scalar_type=ty) == exp, (ty, n, c)
                assert h.compute_device(d, window_size=c, scalar_type=ty) == exp, (ty, n, c)


def test_values_cover_the_extremes():
    for ty, e in TYPES.items():
        vals = set(_values(ty))
        lo, hi = _limits(ty)
        assert {0, 1, lo, hi} <= vals
        if _signed(ty):
            assert {-1, -(1 << (e - 1))} <= vals and min(_values(ty, 1)) == -(1 << (e - 1))


# ---- the width bound: signs through the dense units ----------------------------------------------------
def test_width_bound_and_dense_buckets():
    import torch

    n = 4096
    assert M._test_dense_plan(n, 1, False, 4, 0)["dense"] == 1
    pts = _points(n)
    with M.Bases.from_wire(pts, levels=1) as h:
        for ty, b in (("i32", 20), ("i8", 4)):
            vals, exp = _values(ty, n, 0, b), _expected(ty, n, 0, b)
            assert max(abs(v) for v in vals) == (1 << b) - 1 and min(vals) < 0
            a = _pack(vals, ty)
            for c in WIDTHS:
                assert h.compute(a, window_size=c, scalar_bits=b, scalar_type=ty) == exp, (ty, c)
                assert h.compute_device(_ndev(a), window_size=c, scalar_bits=b, scalar_type=ty) == exp, (ty, c)
        # a boolean mask as it is: "native" makes it u8 with scalar_bits = 1
        bits = [random.Random(3).getrandbits(1) for _ in range(n)]
        mask = torch.tensor(bits, dtype=torch.bool)
        exp = _oracle(bits, pts, _negated(n))
        assert h.compute(mask, scalar_type="native") == exp
        assert h.compute(mask.numpy(), scalar_type="native") == exp
        assert h.compute_device(mask.cuda(), scalar_type="native") == exp
        assert h.compute_device(torch.tensor(_values("i16", n), dtype=torch.int16).cuda(),
                                scalar_type="native") == _expected("i16", n)


# ---- every entry ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _entry_case(ty):
    """Five vectors (a short last launch), a range, an index list with repeats, and the oracle's
    results for each."""
    pts, neg = _points(N), _negated(N)
    vecs = [_values(ty, N, seed) for seed in range(5)]
    full = [_expected(ty, N, seed) for seed in range(5)]
    first, m = 255, 1001
    sub = [_values(ty, m, seed) for seed in range(5)]
    rng = [_oracle(s, pts[first:first + m], neg[first:first + m]) for s in sub]
    idx = np.random.RandomState(TYPES[ty]).randint(0, N, size=m).astype(np.uint32)
    idx[m // 2] = idx[0]
    idx[1] = N - 1
    idx[2:12] = np.arange(10)
    idx.setflags(write=False)
    ind = [_oracle(s, pts[idx], neg[idx]) for s in sub]
    return [_pack(v, ty) for v in vecs], full, first, m, [_pack(s, ty) for s in sub], rng, idx, ind


@pytest.mark.parametrize("flags", [0, M.MSM_FLAG_SERIAL])
@pytest.mark.parametrize("ty", ["i8", "u16", "i64"])
def test_every_entry(ty, flags):
    scs, full, first, m, sub, rng, idx, ind = _entry_case(ty)
    d_scs, d_sub, d_idx = [_ndev(s) for s in scs], [_ndev(s) for s in sub], _dev(idx)
    kw = dict(scalar_type=ty)
    with M.Bases.from_wire(_points(N), levels=1) as h:
        assert [as_xy(r) for r in h.compute_many(scs, flags=flags, **kw)] == full
        assert [as_xy(r) for r in h.compute_many_device(d_scs, flags=flags, **kw)] == full
        assert h.compute_subset(sub[0], first=first, **kw) == rng[0]
        assert h.compute_subset_device(d_sub[1], first=first, m=m, **kw) == rng[1]
        assert h.compute_subset(sub[2], indices=idx, **kw) == ind[2]
        assert h.compute_subset_device(d_sub[3], indices=d_idx, m=m, **kw) == ind[3]
        assert [as_xy(r) for r in h.compute_subset_many(sub, first=first, flags=flags, **kw)] == rng
        assert [as_xy(r) for r in h.compute_subset_many_device(d_sub, first=first, m=m, flags=flags, **kw)] == rng
        assert [as_xy(r) for r in h.compute_subset_many(sub, indices=idx, flags=flags, **kw)] == ind
        assert [as_xy(r) for r in h.compute_subset_many_device(d_sub, indices=d_idx, m=m, flags=flags,
                                                               **kw)] == ind


def test_bit_vectors_on_subsets():
    """A bitmap's length is not its byte count: m is given (or is the index list's)."""
    pts, neg = _points(N), _negated(N)
    first, m = 255, 1001
    bits = _values("bit", m)
    a = _pack(bits, "bit")
    idx = _entry_case("i8")[6]
    with M.Bases.from_wire(pts, levels=1) as h:
        exp = _oracle(bits, pts[first:first + m], neg[first:first + m])
        assert h.compute_subset(a, first=first, m=m, scalar_type="bit") == exp
        assert h.compute_subset_device(_ndev(a), first=first, m=m, scalar_type="bit") == exp
        assert h.compute_subset(a, indices=idx, scalar_type="bit") == _oracle(bits, pts[idx], neg[idx])
        assert as_xy(h.compute_subset_many([a, a], first=first, m=m, scalar_type="bit")[1]) == exp


# ---- cancellation, one bucket -----------------------------------------------------------------------
def test_a_value_and_its_negation_on_one_base_cancel():
    m = 1000
    vals = []
    for v in _values("i16", m // 2, 3):
        v = v if v != -(1 << 15) else 5  # (-2^15 has no counterpart)
        vals += [v, -v]
    idx = np.repeat(np.random.RandomState(9).randint(0, N, size=m // 2), 2).astype(np.uint32)
    with M.Bases.from_wire(_points(N), levels=1) as h:
        a = _pack(vals, "i16")
        for c in WIDTHS:
            assert h.compute_subset(a, indices=idx, window_size=c, scalar_type="i16") == (0, 1), c
        assert h.compute_subset_device(_ndev(a), indices=_dev(idx), m=m, scalar_type="i16") == (0, 1)


def test_all_scalars_in_one_bucket():
    pts, neg = _points(N), _negated(N)
    with M.Bases.from_wire(pts, levels=1) as h:
        for ty, v in (("i8", -128), ("i64", -(1 << 63))):
            exp = _oracle([v] * N, pts, neg)
            a = _pack([v] * N, ty)
            for c in WIDTHS:
                assert h.compute(a, window_size=c, scalar_type=ty) == exp, (ty, c)
                assert h.compute_device(_ndev(a), window_size=c, scalar_type=ty) == exp, (ty, c)


# ---- the plan key and the replayed graph's inputs ---------------------------------------------------
def test_successive_calls_with_other_types_on_one_handle():
    pts, neg = _points(N), _negated(N)
    full = M.gen_scalars(N, seed=77)
    exp_full = O.msm(pts, full, window=10, threads=8)
    i8 = _pack(_values("i8"), "i8")
    as_u8 = [int(x) for x in i8.view(np.uint8)]  # the same bytes read unsigned: other results
    assert _oracle(as_u8, pts, neg) != _expected("i8")
    n64 = M.scalars_to_wire([abs(v) for v in _values("i64")], scalar_bits=64)
    keep = []

    def dev(a):
        keep.append(_ndev(a))  # kept alive: the next tensor gets a new address
        return keep[-1]

    with M.Bases.from_wire(pts, levels=1) as h:
        for _ in range(2):
            assert h.compute_device(dev(i8), scalar_type="i8") == _expected("i8")
            assert h.compute_device(dev(i8), scalar_type="u8") == _oracle(as_u8, pts, neg)
            assert h.compute_device(dev(_pack(_values("bit"), "bit")), scalar_type="bit") == _expected("bit")
            assert h.compute_device(dev(_pack(_values("i64"), "i64")), scalar_type="i64") == _expected("i64")
            keep.append(_dev(n64))
            assert h.compute_device(keep[-1], scalar_bits=64) == O.msm(
                pts, O.ints_to_be_words([abs(v) for v in _values("i64")]), window=10, threads=8)
            keep.append(_dev(full))
            assert h.compute_device(keep[-1]) == exp_full
            assert h.compute(i8, scalar_type="i8") == _expected("i8")
            assert h.compute(i8.view(np.uint8), scalar_type="u8") == _oracle(as_u8, pts, neg)
            assert h.compute(full) == exp_full
        # another vector of the same type at a new address: the replayed graph reads the new one
        assert h.compute_device(dev(_pack(_values("i8", N, 1), "i8")), scalar_type="i8") == _expected("i8", N, 1)
        assert h.compute_device(dev(_pack(_values("i8", N, 2), "i8")), scalar_type="i8") == _expected("i8", N, 2)


# ---- alignment --------------------------------------------------------------------------------------
def _invalid(call):
    with pytest.raises(M.MsmError) as e:
        call()
    assert e.value.code == -1


def test_device_vectors_that_are_only_word_aligned_and_less():
    with M.Bases.from_wire(_points(N), levels=1) as h:
        for ty in ("u8", "i64"):
            a = _pack(_values(ty), ty)
            d4 = _ndev(a, lead=4)
            assert d4.data_ptr() % 16 == 4
            assert h.compute_device(d4, scalar_type=ty) == _expected(ty), ty
            d1 = _ndev(a, lead=1)
            assert d1.data_ptr() % 4 == 1
            _invalid(lambda: h.compute_device(d1, scalar_type=ty))
            _invalid(lambda: h.compute_many_device([_ndev(a), d1], scalar_type=ty))
            assert h.compute_device(_ndev(a), scalar_type=ty) == _expected(ty), ty  # the next call is exact


def test_host_vectors_need_their_elements_alignment():
    a = _pack(_values("i64"), "i64")
    raw = np.zeros(a.nbytes + 8, np.uint8)
    off = (4 - raw.ctypes.data % 8) % 8  # 4 bytes past an 8-byte boundary
    raw[off:off + a.nbytes] = a.view(np.uint8)
    skew = raw[off:off + a.nbytes].view(np.int64)
    assert skew.ctypes.data % 8 == 4
    with M.Bases.from_wire(_points(N), levels=1) as h:
        _invalid(lambda: h.compute(skew, scalar_type="i64"))
        assert h.compute(a, scalar_type="i64") == _expected("i64")


# ---- errors -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("badv", [9, -9, 8, -8, -128])
def test_magnitudes_out_of_range(badv):
    ty, b, count = "i8", 3, 5
    vecs = [_values(ty, N, seed, b) for seed in range(count)]
    scs = [_pack(v, ty) for v in vecs]
    exp = [_expected(ty, N, seed, b) for seed in range(count)]
    bad_last = _pack(vecs[-1][:-1] + (badv,), ty)
    bad_first = _pack((badv,) + vecs[0][1:], ty)
    d_scs = [_ndev(s) for s in scs]
    kw = dict(scalar_bits=b, scalar_type=ty)
    with M.Bases.from_wire(_points(N), levels=1) as h:
        # the host entries refuse before anything is uploaded
        _invalid(lambda: h.compute_many(scs[:-1] + [bad_last], **kw))
        assert [as_xy(r) for r in h.compute_many(scs, **kw)] == exp  # the very next call is exact
        _invalid(lambda: h.compute(bad_first, **kw))
        _invalid(lambda: h.compute_subset(bad_first[:10], first=3, **kw))
        # on the device the recode masks the magnitude: an error, and the slot left clean
        _invalid(lambda: h.compute_many_device(d_scs[:-1] + [_ndev(bad_last)], **kw))
        assert [as_xy(r) for r in h.compute_many_device(d_scs, **kw)] == exp
        _invalid(lambda: h.compute_many_device([_ndev(bad_first)] + d_scs[1:], **kw))
        assert [as_xy(r) for r in h.compute_many_device(d_scs, **kw)] == exp
        _invalid(lambda: h.compute_device(_ndev(bad_last), **kw))
        assert h.compute_device(d_scs[0], **kw) == exp[0]
        assert h.compute(scs[1], **kw) == exp[1]


def test_type_and_width_arguments():
    a = _pack(_values("i8"), "i8")
    with M.Bases.from_wire(_points(N), levels=1) as h:
        for ty, b in ((0, None), (10, None), (77, 4), ("i8", 0), ("i8", 9), ("bit", 2), ("u64", 65), ("i32", 256)):
            o = M._opts(None, scalar_bits=b, scalar_type=ty)
            out = np.zeros(16, np.uint32)
            rc = M.load().msm_bases_compute(h._h, a.ctypes.data, o, out.ctypes.data_as(ctypes.POINTER(
                ctypes.c_uint32)))
            assert rc == -1, (ty, b)
            d = _ndev(a)
            rc = M.load().msm_bases_compute_device(h._h, d.data_ptr(), o, None, out.ctypes.data_as(
                ctypes.POINTER(ctypes.c_uint32)))
            assert rc == -1, (ty, b)
        assert h.compute(a, scalar_type="i8", scalar_bits=8) == _expected("i8")
        assert h.compute(_pack(_values("bit"), "bit"), scalar_type="bit", scalar_bits=1) == _expected("bit")


# ---- folded handles run typed calls unfolded --------------------------------------------------------
def test_typed_calls_on_a_folded_handle():
    full = M.gen_scalars(N, seed=78)
    exp_full = O.msm(_points(N), full, window=10, threads=8)
    with M.Bases.from_wire(_points(N), levels=2, window_size=15) as h:
        assert h.info["levels"] == 2
        for ty in ("bit", "i8", "i64"):
            a = _pack(_values(ty), ty)
            for c in (None, 4, 13, 15, 17):  # any width: the level-0 records do not depend on it
                assert h.compute(a, window_size=c, scalar_type=ty) == _expected(ty), (ty, c)
            assert h.compute_device(_ndev(a), scalar_type=ty) == _expected(ty), ty
        assert h.compute(full) == exp_full  # folded, as before
        assert h.compute_device(_dev(full)) == exp_full


# ---- profile ----------------------------------------------------------------------------------------
def test_profile_reports_the_launchs_windows():
    with M.Bases.from_wire(_points(N), levels=1) as h:
        M.set_profiling(True)
        try:
            for ty, b, c in (("i64", None, 16), ("i64", None, None), ("i8", None, 4), ("i32", 20, 13), ("bit", None, 17)):
                bb = b or TYPES[ty]
                assert h.compute(_pack(_values(ty, N, 0, b), ty), window_size=c, scalar_bits=b,
                                 scalar_type=ty) == _expected(ty, N, 0, b)
                plan = M._test_native_plan(N, ty, bb, c or 0)
                assert plan["windows"] == M._test_narrow_plan(N, bb, c or 0)["windows"]
                prof = M.last_profile()
                assert prof["windows"] == plan["windows"], (ty, c)
                assert prof["window_bits"] == plan["c"], (ty, c)
        finally:
            M.set_profiling(False)
