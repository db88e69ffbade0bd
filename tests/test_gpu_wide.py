"""GPU tests of wide native scalars on a resident-bases handle (include/msm.h MSM_FLAG_SCALAR_FIELD,
msm_amd.Bases.compute*(scalar_type="u128" | "i128" | "u256" | "fr_mont")): little-endian 128- and 256-bit
integers and Montgomery-form Fr as they lie in a prover's memory, bit-exact against the C oracle on the
magnitudes as 8-word scalars over points negated by hand where the value is negative -- never against
another entry of the library.  Values are integers throughout; "fr_mont" vectors hold their Montgomery
encodings a = v 2^256 mod r."""
import ctypes
import functools
import random

import numpy as np
import pytest

import msm_amd as M
from _closed_form import as_xy
from _narrow_model import auto_width, edge_scalars
from oracle import oracle as O
from test_gpu_native import _negated, _oracle
from test_gpu_subset import _dev, _points

pytestmark = pytest.mark.gpu

TYPES = {"u128": 128, "i128": 128, "u256": 256, "fr_mont": 256}
R = M.FR_MODULUS
N = 4097  # one past the recode workgroup's span: two workgroups, the second with one scalar; odd (no paired stores)
N_EVEN = 4134  # two workgroups and even: paired 4-B code stores in every lane, the second workgroup's full lanes too
SIZES = (1, 2, 3, 4095, N, N_EVEN)
WIDTHS = (None, 4, 13, 17)  # 17 takes the 32-bit digit codes


def _width(ty, b=None):
    """The magnitude bits of a call: scalar_bits, else the element's (251 for fr_mont)."""
    return b if b is not None else 251 if ty == "fr_mont" else TYPES[ty]


def _limits(ty, b=None):
    """The least and greatest value of the type, or of magnitudes below 2^b."""
    lo, hi = {"i128": (-(1 << 127), (1 << 127) - 1), "fr_mont": (0, R - 1)}.get(ty, (0, (1 << TYPES[ty]) - 1))
    if b is not None and b < TYPES[ty]:
        lo, hi = max(lo, -((1 << b) - 1)), min(hi, (1 << b) - 1)
    return lo, hi


@functools.lru_cache(maxsize=None)
def _values(ty, m=N, seed=0, b=None):
    """m values of the type (magnitudes below 2^b): random ones, then (from m = 16) 0, 1, the least and
    greatest value, -1, r - 1, the value whose Montgomery encoding is 1, and the carry edges of every window
    of every width the tests run (under both signs for i128); the first of fewer values is the least one of
    a signed type, else the greatest, and the second the greatest."""
    bb = _width(ty, b)
    lo, hi = _limits(ty, b)
    rnd = random.Random(9000 + 131 * TYPES[ty] + 17 * m + seed + 7 * bb + sum(map(ord, ty)))
    vals = [rnd.randint(lo, hi) for _ in range(m)]
    if m >= 16:
        edges = {0, 1, lo, hi, -1, R - 1, pow(2, -256, R), 1 << (bb - 1)}
        for c in WIDTHS:
            gb = min(bb, 253)  # (a 256-bit integer of 254 bits and more: the edges of the 253-bit windows)
            for v in edge_scalars(gb, c or auto_width(m, gb, M.get_best_window_size(m))):
                edges.update((v, -v))
        edges = sorted((x for x in edges if lo <= x <= hi), key=lambda x: (abs(x), x))
        assert len(edges) <= m - 10
        vals[10:10 + len(edges)] = edges
    else:
        vals[0] = lo if lo < 0 else hi
        if m > 1:
            vals[1] = hi
    return tuple(vals)


@functools.lru_cache(maxsize=None)
def _expected(ty, n=N, seed=0, b=None):
    return _oracle(_values(ty, n, seed, b), _points(n), _negated(n))


@functools.lru_cache(maxsize=None)
def _pack(ty, n=N, seed=0, b=None):
    a = M.scalars_to_wide(_values(ty, n, seed, b), ty)
    a.setflags(write=False)
    return a


def _ndev(a, lead=0):
    """A host array's bytes on the device, `lead` bytes past a 512-byte boundary: a uint8 tensor
    [n, e / 8] of exactly the vector's bytes."""
    import torch

    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.zeros(raw.size + lead, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 512 == 0
    buf[lead:] = torch.from_numpy(raw.copy())
    return buf[lead:].view(a.shape[0], -1)


def _with_row(a, i, value):
    """A copy of the vector with element i replaced by the raw little-endian integer `value`."""
    bad = a.copy()
    k = a.shape[1]
    bad[i] = np.frombuffer((value & ((1 << 64 * k) - 1)).to_bytes(8 * k, "little"), dtype="<u8")
    return bad


def _invalid(call):
    with pytest.raises(M.MsmError) as e:
        call()
    assert e.value.code == -1


# ---- 1. parity --------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
def test_parity_with_oracle(ty):
    import torch

    for n in SIZES:
        a, exp = _pack(ty, n), _expected(ty, n)
        assert a.nbytes == n * TYPES[ty] // 8
        d = _ndev(a)
        with M.Bases.from_wire(_points(n), levels=1) as h:
            for c in (WIDTHS if n == N else (None,)):
                assert h.compute(a, window_size=c, scalar_type=ty) == exp, (ty, n, c)
                assert h.compute_device(d, window_size=c, scalar_type=ty) == exp, (ty, n, c)
            if n == N:  # the other array forms: words and bytes on the host, int64 limbs on the device
                assert h.compute(a.view(np.uint32), scalar_type=ty) == exp
                assert h.compute(a.view(np.uint8), scalar_type=ty) == exp
                assert h.compute_device(torch.from_numpy(a.view(np.int64).copy()).cuda(), scalar_type=ty) == exp


def test_values_cover_the_extremes():
    for ty, e in TYPES.items():
        vals = set(_values(ty))
        lo, hi = _limits(ty)
        assert {0, 1, lo, hi} <= vals, ty
        assert hi == {"u128": (1 << 128) - 1, "i128": (1 << 127) - 1, "u256": (1 << 256) - 1, "fr_mont": R - 1}[ty]
        if ty == "i128":
            assert {-1, -(1 << 127)} <= vals and _values(ty, 1)[0] == -(1 << 127)
        if e == 256:
            assert R - 1 in vals
        for c in WIDTHS:
            gb = min(_width(ty), 253)
            edges = edge_scalars(gb, c or auto_width(N, gb, M.get_best_window_size(N)))
            assert {v for v in edges if v <= hi} <= vals, (ty, c)
            if ty == "i128":
                assert {-v for v in edges if -v >= lo} <= vals, c
    # fr_mont: the encodings are what the vector holds, the encoding of 1 (2^256 mod r) and 1 itself among them
    enc = {int.from_bytes(row.astype("<u8").tobytes(), "little") for row in _pack("fr_mont")}
    assert {(1 << 256) % R, 1, 0, (R - 1 << 256) % R} <= enc and max(enc) < R


# ---- 2. u256 at every kind of width -------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 8, 64, 251, 253, 254, 256])
def test_u256_widths(b):
    a, exp = _pack("u256", N, 0, b), _expected("u256", N, 0, b)
    assert max(_values("u256", N, 0, b)) == (1 << b) - 1
    with M.Bases.from_wire(_points(N), levels=1) as h:
        assert h.compute(a, scalar_bits=b, scalar_type="u256") == exp
        assert h.compute_device(_ndev(a), scalar_bits=b, scalar_type="u256") == exp
        assert h.compute_device(_ndev(a), window_size=17, scalar_bits=b, scalar_type="u256") == exp


def test_u256_bytes_take_the_dense_buckets():
    n, b, c = 4096, 8, 4
    assert M._test_dense_plan(n, 1, False, b, c)["dense"] == 1
    assert M._test_wide_plan(n, "u256", b, c)["windows"] == M._test_narrow_plan(n, b, c)["windows"]
    a, exp = _pack("u256", n, 0, b), _expected("u256", n, 0, b)
    with M.Bases.from_wire(_points(n), levels=1) as h:
        assert h.compute(a, window_size=c, scalar_bits=b, scalar_type="u256") == exp
        assert h.compute_device(_ndev(a), window_size=c, scalar_bits=b, scalar_type="u256") == exp


# ---- 3. alignment -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
def test_device_vectors_that_are_only_word_aligned_and_less(ty):
    a, exp = _pack(ty), _expected(ty)
    with M.Bases.from_wire(_points(N), levels=1) as h:
        for lead in (4, 8, 12):
            d = _ndev(a, lead)
            assert d.data_ptr() % 16 == lead
            assert h.compute_device(d, scalar_type=ty) == exp, (ty, lead)
        d2 = _ndev(a, 2)
        assert d2.data_ptr() % 4 == 2
        _invalid(lambda: h.compute_device(d2, scalar_type=ty))
        _invalid(lambda: h.compute_many_device([_ndev(a), d2], scalar_type=ty))
        assert h.compute_device(_ndev(a), scalar_type=ty) == exp  # the next call is exact


def test_u256_of_256_bits_word_aligned():
    """The full-width little-endian recode reads a 4-byte-aligned vector word by word too."""
    a, exp = _pack("u256"), _expected("u256")
    with M.Bases.from_wire(_points(N), levels=1) as h:
        for c in (None, 17):
            assert h.compute_device(_ndev(a, 4), window_size=c, scalar_type="u256") == exp, c


def test_host_vectors_need_8_byte_alignment():
    a = _pack("i128")
    raw = np.zeros(a.nbytes + 16, np.uint8)
    off = (4 - raw.ctypes.data % 8) % 8  # 4 bytes past an 8-byte boundary
    raw[off:off + a.nbytes] = a.view(np.uint8).reshape(-1)
    skew = raw[off:off + a.nbytes]
    assert skew.ctypes.data % 8 == 4
    out = np.zeros(16, np.uint32)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    with M.Bases.from_wire(_points(N), levels=1) as h:
        assert M.load().msm_bases_compute(h._h, skew.ctypes.data, M._opts(None, scalar_type="i128"), op) == -1
        assert h.compute(skew.reshape(-1, 16), scalar_type="i128") == _expected("i128")  # (the binding copies)


# ---- 4. range errors --------------------------------------------------------------------------------
RANGE_CASES = {
    "fr_mont-r": ("fr_mont", None, R),
    "fr_mont-ones": ("fr_mont", None, (1 << 256) - 1),
    "u256-bit200": ("u256", 200, 1 << 200),
    "u256-top": ("u256", 200, 1 << 255),
    "i128-bit100": ("i128", 100, 1 << 100),
    "i128-neg": ("i128", 100, -(1 << 100)),
    "i128-least": ("i128", 127, -(1 << 127)),
}


@pytest.mark.parametrize("at", [0, N - 1])
@pytest.mark.parametrize("case", RANGE_CASES)
def test_values_out_of_range(case, at):
    ty, b, badv = RANGE_CASES[case]
    good, good2 = _pack(ty, N, 0, b), _pack(ty, N, 1, b)
    exp, exp2 = _expected(ty, N, 0, b), _expected(ty, N, 1, b)
    bad = _with_row(good, at, badv)
    kw = dict(scalar_bits=b, scalar_type=ty)
    with M.Bases.from_wire(_points(N), levels=1) as h:
        # the host entries refuse before anything is uploaded
        _invalid(lambda: h.compute(bad, **kw))
        assert h.compute(good, **kw) == exp  # the very next call is exact
        _invalid(lambda: h.compute_many([good, good2, bad], **kw))
        assert [as_xy(r) for r in h.compute_many([good, good2], **kw)] == [exp, exp2]
        # on the device the recode masks the value: an error after the launch, and the slot left clean
        d_good, d_good2 = _ndev(good), _ndev(good2)
        _invalid(lambda: h.compute_device(_ndev(bad), **kw))
        assert h.compute_device(d_good, **kw) == exp
        _invalid(lambda: h.compute_many_device([d_good, _ndev(bad), d_good2], **kw))
        assert [as_xy(r) for r in h.compute_many_device([d_good, d_good2], **kw)] == [exp, exp2]


def test_field_and_width_arguments():
    a = _pack("u256")
    d = _ndev(a)
    out = np.zeros(16, np.uint32)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))

    def typed(flags, scalar_type=0, scalar_field=0, scalar_bits=0):
        o = M.MsmOptsTyped(0, 0, -1, flags)
        o.scalar_type, o.scalar_field, o.scalar_bits = scalar_type, scalar_field, scalar_bits
        return o

    F, T, B = M.MSM_FLAG_SCALAR_FIELD, M.MSM_FLAG_SCALAR_TYPE, M.MSM_FLAG_SCALAR_BITS
    with M.Bases.from_wire(_points(N), levels=1) as h:
        for o in (typed(F, 0, 0), typed(F, 0, 5), typed(F, 5, 0), typed(F | T, 5, 3), typed(F | T, 0, 3),
                  typed(F | B, 0, 3, 0), typed(F | B, 0, 3, 257), typed(F | B, 0, 1, 129), typed(F | B, 0, 2, 129),
                  typed(F | B, 0, 4, 250), typed(F | B, 0, 4, 252), typed(F | B, 0, 4, 256), typed(T, 0x103, 0)):
            L = M.load()
            assert L.msm_bases_compute(h._h, a.ctypes.data, ctypes.byref(o), op) == -1
            assert L.msm_bases_compute_device(h._h, d.data_ptr(), ctypes.byref(o), None, op) == -1
        # scalar_field is read only when its flag is set: garbage there leaves a typed and a plain call alone
        o = typed(0, 77, 99)
        assert M.load().msm_bases_compute(h._h, _pack_be(a).ctypes.data, ctypes.byref(o), op) == 0
        assert as_xy(out) == _expected("u256")
        assert h.compute(a, scalar_type="u256", scalar_bits=256) == _expected("u256")
        assert h.compute(_pack("fr_mont"), scalar_type="fr_mont", scalar_bits=251) == _expected("fr_mont")
        with pytest.raises(TypeError):
            h.compute(a.view(np.int64), scalar_type="u256")
        with pytest.raises(TypeError):
            h.compute_device(a, scalar_type="u256")  # a host array at a device entry


def _pack_be(a):
    """The 8-word wire scalars of a u256 vector (the call the wide one replaces)."""
    vals = [int.from_bytes(row.astype("<u8").tobytes(), "little") for row in a]
    return np.ascontiguousarray(O.ints_to_be_words(vals))


# ---- 5. composition ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _entry_case(ty):
    """Two vectors (given as three, one repeated), a range, an index list with repeats, and the oracle's
    results for each."""
    pts, neg = _points(N), _negated(N)
    first, m = 1999, 1001
    sub = [_values(ty, m, seed) for seed in range(2)]
    rng = [_oracle(s, pts[first:first + m], neg[first:first + m]) for s in sub]
    idx = np.random.RandomState(TYPES[ty]).randint(0, N, size=m).astype(np.uint32)
    idx[m // 2] = idx[0]
    idx[1] = N - 1
    idx[2:12] = np.arange(10)
    idx[12:16] = 7
    idx.setflags(write=False)
    ind = [_oracle(s, pts[idx], neg[idx]) for s in sub]
    return first, m, [_pack(ty, m, seed) for seed in range(2)], rng, idx, ind


@pytest.mark.parametrize("flags", [0, M.MSM_FLAG_SERIAL])
@pytest.mark.parametrize("ty", ["fr_mont", "i128"])
def test_every_entry(ty, flags):
    first, m, sub, rng, idx, ind = _entry_case(ty)
    scs = [_pack(ty, N, 0), _pack(ty, N, 1), _pack(ty, N, 1)]
    full = [_expected(ty, N, 0), _expected(ty, N, 1), _expected(ty, N, 1)]
    d0, d1 = _ndev(scs[0]), _ndev(scs[1])
    d_scs = [d0, d1, d1]
    s3, r3, i3 = [sub[0], sub[1], sub[1]], [rng[0], rng[1], rng[1]], [ind[0], ind[1], ind[1]]
    ds0, ds1 = _ndev(sub[0]), _ndev(sub[1])
    d_sub, d_idx = [ds0, ds1, ds1], _dev(idx)
    kw = dict(scalar_type=ty)
    with M.Bases.from_wire(_points(N), levels=1) as h:
        assert [as_xy(r) for r in h.compute_many(scs, flags=flags, **kw)] == full
        assert [as_xy(r) for r in h.compute_many_device(d_scs, flags=flags, **kw)] == full
        assert h.compute_subset(sub[0], first=first, **kw) == rng[0]
        assert h.compute_subset_device(ds1, first=first, **kw) == rng[1]
        assert h.compute_subset(sub[1], indices=idx, **kw) == ind[1]
        assert h.compute_subset_device(ds0, indices=d_idx, **kw) == ind[0]
        assert [as_xy(r) for r in h.compute_subset_many(s3, first=first, flags=flags, **kw)] == r3
        assert [as_xy(r) for r in h.compute_subset_many_device(d_sub, first=first, flags=flags, **kw)] == r3
        assert [as_xy(r) for r in h.compute_subset_many(s3, indices=idx, flags=flags, **kw)] == i3
        assert [as_xy(r) for r in h.compute_subset_many_device(d_sub, indices=d_idx, flags=flags, **kw)] == i3
        assert h.compute_device(d0, run_length=20, **kw) == full[0]


# ---- 6. folded handles run wide calls unfolded --------------------------------------------------------
def test_wide_calls_on_a_folded_handle():
    full = M.gen_scalars(N, seed=78)
    exp_full = O.msm(_points(N), full, window=10, threads=8)
    with M.Bases.from_wire(_points(N), levels=2, window_size=15) as h:
        assert h.info["levels"] == 2
        for ty in ("fr_mont", "u256"):  # u256 of 256 bits: the full-width launch, unfolded all the same
            a = _pack(ty)
            for c in (None, 4, 15, 17):  # any width: the level-0 records do not depend on it
                assert h.compute(a, window_size=c, scalar_type=ty) == _expected(ty), (ty, c)
            assert h.compute_device(_ndev(a), scalar_type=ty) == _expected(ty), ty
        assert h.compute(_pack("u256"), scalar_bits=256, scalar_type="u256") == _expected("u256")
        assert h.compute(full) == exp_full  # folded, as before
        assert h.compute_device(_dev(full)) == exp_full


# ---- the plan key and the replayed graph's inputs ---------------------------------------------------
def test_successive_calls_with_other_types_on_one_handle():
    pts = _points(N)
    u256 = _pack("u256", N, 0, 251)
    assert max(_values("u256", N, 0, 251)) >= R  # the same bytes read as Montgomery forms: not canonical
    keep = []

    def dev(a):
        keep.append(_ndev(a))  # kept alive: the next tensor gets a new address
        return keep[-1]

    with M.Bases.from_wire(pts, levels=1) as h:
        for _ in range(2):
            assert h.compute_device(dev(u256), scalar_bits=251, scalar_type="u256") == _expected("u256", N, 0, 251)
            assert h.compute_device(dev(_pack("fr_mont")), scalar_type="fr_mont") == _expected("fr_mont")
            assert h.compute_device(dev(_pack("u128")), scalar_type="u128") == _expected("u128")
            assert h.compute_device(dev(_pack("i128")), scalar_type="i128") == _expected("i128")
            assert h.compute_device(dev(_pack("u256")), scalar_type="u256") == _expected("u256")
            keep.append(_dev(_pack_be(_pack("u256"))))
            assert h.compute_device(keep[-1]) == _expected("u256")
        # another vector of the same type at a new address: the replayed graph reads the new one
        assert h.compute_device(dev(_pack("fr_mont", N, 1)), scalar_type="fr_mont") == _expected("fr_mont", N, 1)
        assert h.compute_device(dev(_pack("fr_mont", N, 2)), scalar_type="fr_mont") == _expected("fr_mont", N, 2)
        _invalid(lambda: h.compute_device(dev(u256), scalar_type="fr_mont"))
        assert h.compute_device(dev(_pack("fr_mont")), scalar_type="fr_mont") == _expected("fr_mont")


# ---- 7. guard bands ---------------------------------------------------------------------------------
def test_guard_bands_stay_clean():
    """Every workspace buffer at exactly its plan's size between guard bands (csrc/host_guard.h), and the
    caller's device vectors of exactly n e / 8 bytes: exact results and an empty report."""
    L = M.load()
    L.msm_shutdown()
    M._test_guard(True)
    try:
        for ty in TYPES:
            for n in (1, 3, N):
                a, exp = _pack(ty, n), _expected(ty, n)
                d = _ndev(a)
                assert d.numel() == n * TYPES[ty] // 8
                M._test_guard_release()
                with M.Bases.from_wire(_points(n), levels=1) as h:
                    assert h.compute_device(d, scalar_type=ty) == exp, (ty, n)
                    assert h.compute(a, scalar_type=ty) == exp, (ty, n)
                    assert M._test_guard_check() == [], (ty, n)
    finally:
        L.msm_shutdown()
        M._test_guard(False)
