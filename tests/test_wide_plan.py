"""Wide native scalars on a resident-bases handle, the host-only part (include/msm.h MSM_FLAG_SCALAR_FIELD):
the header and the bindings agree, the plan of a wide launch is the narrow plan of its magnitude bits
(msm_test_wide_plan), the argument rules, the entries that refuse the flag, the Montgomery decoding of
csrc/fr.cuh run on the host (msm_test_fr_from_mont) against Python's integers, and the Python side's
packing.  No GPU needed."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import msm_amd as M
from oracle import oracle as O

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "msm.h")
TYPES = {"u128": 128, "i128": 128, "u256": 256, "fr_mont": 256}
SIZES = (1, 7, 8, 9, 4097, 1 << 20)
WIDTHS = (0, 4, 13, 16, 17, 20)
SHARED = ("c", "windows", "q", "nhi", "words", "packed")
R = M.FR_MODULUS


# ---- header and bindings ------------------------------------------------------------------------------
def test_the_field_table_matches_the_header():
    src = open(HEADER).read()
    vals = {k.lower(): int(v) for k, v in re.findall(r"#define MSM_FIELD_([A-Z0-9_]+) (\d+)u", src)}
    assert vals == {k: v[0] for k, v in M.WIDE_TYPES.items()} == {"u128": 1, "i128": 2, "u256": 3, "fr_mont": 4}
    assert {k: v[1] for k, v in M.WIDE_TYPES.items()} == TYPES
    assert int(re.search(r"#define MSM_FLAG_SCALAR_FIELD (\d+)u", src).group(1)) == M.MSM_FLAG_SCALAR_FIELD == 64
    assert M.FR_MODULUS == O.R_ORDER and R.bit_length() == 251
    assert hex(R)[2:].rjust(64, "0") in src.lower()


def test_scalar_field_fills_the_tail_padding():
    assert ctypes.sizeof(M.MsmOpts) == 40
    assert M.MsmOptsTyped.scalar_type.offset == 40
    assert M.MsmOptsTyped.scalar_field.offset == 44 and ctypes.sizeof(M.MsmOptsTyped) == 48
    o = M._opts(16, scalar_bits=100, scalar_type="i128")._obj
    assert isinstance(o, M.MsmOptsTyped) and o.scalar_field == 2 and o.scalar_type == 0
    assert o.flags == M.MSM_FLAG_SCALAR_FIELD | M.MSM_FLAG_SCALAR_BITS and o.scalar_bits == 100
    o = M._opts(None, scalar_type="fr_mont")._obj
    assert o.flags == M.MSM_FLAG_SCALAR_FIELD and o.scalar_field == 4
    o = M._opts(None, scalar_type="i64")._obj  # the native types keep their flag and field
    assert o.flags == M.MSM_FLAG_SCALAR_TYPE and o.scalar_field == 0


# ---- plans ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", ["u128", "i128", "u256"])
def test_plan_is_the_narrow_plan_of_the_magnitude_bits(ty):
    e = TYPES[ty]
    for n in SIZES:
        for b in range(1, min(e, 253) + 1):
            for c in WIDTHS:
                p = M._test_wide_plan(n, ty, b, c)
                assert {k: p[k] for k in SHARED} == M._test_narrow_plan(n, b, c), (ty, n, b, c)
                assert p["vector_bytes"] == n * e // 8 == p["region_bytes"], (ty, n)


def test_fr_mont_plan_is_the_narrow_plan_of_251_bits():
    for n in SIZES:
        for c in WIDTHS:
            p = M._test_wide_plan(n, "fr_mont", 251, c)
            assert {k: p[k] for k in SHARED} == M._test_narrow_plan(n, 251, c), (n, c)
            assert p["vector_bytes"] == 32 * n
    # at c = 16: sixteen balanced windows over T = 252 bits (twelve of 16 bits, four of 15), no overflow window
    p = M._test_wide_plan(1 << 20, "fr_mont", 251, 16)
    assert (p["windows"], p["q"], p["nhi"], p["c"]) == (16, 15, 12, 16)


def test_u256_of_254_bits_and_more_is_the_full_width_plan():
    for n in SIZES:
        for b in (254, 255, 256):
            for c in WIDTHS:
                p = M._test_wide_plan(n, "u256", b, c)
                assert {k: p[k] for k in SHARED} == M._test_narrow_plan(n, b, c), (n, b, c)
                assert p["words"] == 8 and p["vector_bytes"] == 32 * n
                if c:  # main windows plus the overflow window
                    assert p["windows"] == M.window_count(c), (n, b, c)


def test_plan_argument_errors():
    def invalid(*a):
        with pytest.raises(M.MsmError) as err:
            M._test_wide_plan(4097, *a)
        assert err.value.code == -1, a

    for field in (0, 5, 255, 0x101, 1 << 31):
        invalid(field, 1, 16)
    for ty, e in TYPES.items():
        invalid(ty, 0, 16)
        invalid(ty, e + 1, 16)
        invalid(ty, 257, 16)
    for b in (1, 250, 252, 253, 255, 256):
        invalid("fr_mont", b, 16)
    for c in (3, 21):
        with pytest.raises(M.MsmError) as err:
            M._test_wide_plan(4097, "u256", 200, c)
        assert err.value.code == -2, c


def test_other_entries_refuse_the_flag_before_any_device_work():
    L = M.load()
    n = 4
    pts = np.ascontiguousarray(M.gen_points(n))
    sc = np.ascontiguousarray(M.gen_scalars(n))
    out = np.zeros(16, np.uint32)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    pp = (ctypes.c_void_p * 1)(pts.ctypes.data)
    ss = (ctypes.c_void_p * 1)(sc.ctypes.data)
    for bits, ty in ((None, "u256"), (251, "fr_mont"), (8, "i128")):
        o = M._opts(None, scalar_bits=bits, scalar_type=ty)
        assert L.msm_compute(pts.ctypes.data, sc.ctypes.data, n, o, op) == -1
        # (host addresses: the flag is refused before either pointer is looked at)
        assert L.msm_compute_device(pts.ctypes.data, sc.ctypes.data, n, o, None, op) == -1
        assert L.msm_compute_batch_device(pts.ctypes.data, sc.ctypes.data, n, 1, o, None, op) == -1
        assert L.msm_compute_many_device(ctypes.cast(pp, ctypes.c_void_p), ctypes.cast(ss, ctypes.c_void_p), n, 1, o,
                                         None, op) == -1
        assert L.msm_compute_shared_device(pts.ctypes.data, ctypes.cast(ss, ctypes.c_void_p), n, 1, o, None, op) == -1
        assert L.msm_compute_shared(pts.ctypes.data, ctypes.cast(ss, ctypes.c_void_p), n, 1, o, op) == -1
        assert L.msm_compute_many(ctypes.cast(pp, ctypes.c_void_p), ctypes.cast(ss, ctypes.c_void_p), n, 1, o,
                                  op) == -1
        assert L.msm_compute_cocompute(pts.ctypes.data, sc.ctypes.data, n, o, 0.5, 1, op) == -1
        h = ctypes.c_void_p()
        assert L.msm_bases_create(pts.ctypes.data, n, o, 1, ctypes.byref(h)) == -1
        assert not h.value
        assert L.msm_bases_create_device(pts.ctypes.data, n, o, 1, None, ctypes.byref(h)) == -1
        part = np.zeros(32, np.uint32)
        pp32 = part.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        assert L.msm_compute_partial(pts.ctypes.data, sc.ctypes.data, n, o, pp32) == -1
        assert L.msm_compute_device_partial(pts.ctypes.data, sc.ctypes.data, n, o, None, pp32) == -1
        assert L.msm_compute_many_device_partial(ctypes.cast(pp, ctypes.c_void_p), ctypes.cast(ss, ctypes.c_void_p),
                                                 n, 1, o, None, pp32) == -1


# ---- REDC -----------------------------------------------------------------------------------------------
def _decode(a):
    return a * pow(2, -256, R) % R


def test_fr_from_mont_on_random_values():
    rnd = random.Random(251)
    vals = [rnd.randrange(R) for _ in range(4096)]
    got, ok = M._test_fr_from_mont(vals)
    assert all(ok)
    assert got == [_decode(a) for a in vals]


def test_fr_from_mont_on_the_edges():
    ones = 0xffffffff
    edge = [0, 1, (1 << 256) % R, R - 1]
    # every a < r with one 32-bit limb all-ones and the others 0 or all-ones
    for k in range(8):
        others = [j for j in range(8) if j != k]
        for mask in range(1 << 7):
            a = ones << (32 * k)
            for bit, j in enumerate(others):
                if mask >> bit & 1:
                    a |= ones << (32 * j)
            if a < R:
                edge.append(a)
    assert len(edge) == 4 + 7 * 64  # (limb 7 all-ones is past r: the patterns of the other seven limbs remain)
    got, ok = M._test_fr_from_mont(edge)
    assert all(ok)
    assert got == [_decode(a) for a in edge]
    assert got[2] == 1 and got[0] == 0
    # not canonical; the decoding is still the reduced one, as the recode kernel relies on
    bad = [R, R + 1, (1 << 256) - 1, 1 << 255, R | (1 << 255)]
    got, ok = M._test_fr_from_mont(bad)
    assert ok == [False] * len(bad)
    assert got == [_decode(a) for a in bad] and all(v < R for v in got)


# ---- packing --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
def test_scalars_to_wide_round_trips_and_refuses_values_that_do_not_fit(ty):
    e = TYPES[ty]
    lo, hi = {"i128": (-(1 << 127), (1 << 127) - 1), "fr_mont": (0, R - 1)}.get(ty, (0, (1 << e) - 1))
    vals = [0, 1, hi, lo, 12345678901234567890123456789 % (hi + 1), hi - 1]
    a = M.scalars_to_wide(vals, ty)
    assert a.dtype == np.uint64 and a.shape == (len(vals), e // 64) and a.flags["C_CONTIGUOUS"]
    raw = a.astype("<u8").tobytes()
    back = [int.from_bytes(raw[i * e // 8:(i + 1) * e // 8], "little") for i in range(len(vals))]
    if ty == "i128":
        back = [v - (1 << 128) if v >> 127 else v for v in back]
    if ty == "fr_mont":
        assert all(v < R for v in back)
        assert back[1] == (1 << 256) % R
        back = [_decode(v) for v in back]
    assert back == vals
    assert M.scalars_to_wide([], ty).shape == (0, e // 64)
    for bad in (hi + 1, lo - 1):
        with pytest.raises(ValueError):
            M.scalars_to_wide([1, bad], ty)
    with pytest.raises(ValueError):
        M.scalars_to_wide([1], "u64")


def test_the_arrays_a_wide_type_takes():
    import torch

    a = M.scalars_to_wide([1, 2, 3], "u256")
    for view in (a, a.view(np.uint32), a.view(np.uint8)):
        assert M._native_type(view, "u256", None) == ("u256", None)
        assert M._native_host(view, "u256").ctypes.data == view.ctypes.data  # uncopied
        assert M._native_host(view, "u256").shape[0] == 3
    assert M._native_host(torch.from_numpy(a.view(np.int64)), "fr_mont").shape == (3, 4)
    assert M._native_host([5, 6], "u128").tolist() == [[5, 0], [6, 0]]
    for bad in (a.reshape(-1), a.view(np.uint16), a.astype(np.float64), a[:, :2], a.view(np.int64),
                np.asfortranarray(a), a[::2], torch.zeros(3, 4, dtype=torch.int32)):
        with pytest.raises(TypeError):
            M._native_type(bad, "u256", None)
    with pytest.raises(TypeError):
        M._native_type(a, "u128", None)  # [3, 4] uint64 is three 256-bit elements, not 128-bit ones
    # "native" never infers a wide type: a [n, 4] uint64 array is ambiguous
    with pytest.raises(TypeError):
        M._native_type(np.zeros((3, 4), np.float32), "native", None)
    assert M._native_type(np.zeros((3, 4), np.uint64), "native", None) == ("u64", None)
    # the device forms take device tensors or raw pointers only
    with pytest.raises(TypeError):
        M._wide_device(a, "u256")
    with pytest.raises(TypeError):
        M._wide_device(torch.from_numpy(a.view(np.int64)), "u256")
    M._wide_device(0x7f0000000000, "u256")
    M._wide_device(a, "i64")  # not a wide type: nothing to check


def test_a_host_vector_off_its_alignment_is_copied():
    a = M.scalars_to_wide(list(range(1, 6)), "u128")
    raw = np.zeros(a.nbytes + 16, np.uint8)
    off = (4 - raw.ctypes.data % 8) % 8  # 4 bytes past an 8-byte boundary
    raw[off:off + a.nbytes] = a.view(np.uint8).reshape(-1)
    skew = raw[off:off + a.nbytes].reshape(-1, 16)
    assert skew.ctypes.data % 8 == 4
    got = M._native_host(skew, "u128")
    assert got.ctypes.data % 8 == 0 and got.tobytes() == a.tobytes()


# ---- build ----------------------------------------------------------------------------------------------
def test_the_built_library_holds_the_wide_recode_kernels():
    """build() cross-compiled them for gfx950: every instantiation's symbol is in the library's code object."""
    blob = open(M.lib_path(), "rb").read()
    for sym in (b"k_recode_wideItLj4ELj0E", b"k_recode_wideItLj4ELj1E", b"k_recode_wideItLj8ELj0E",
                b"k_recode_wideItLj8ELj2E", b"k_recode_wideIjLj4ELj0E", b"k_recode_wideIjLj4ELj1E",
                b"k_recode_wideIjLj8ELj0E", b"k_recode_wideIjLj8ELj2E", b"k_recode_hist_leItE", b"k_recode_hist_leIjE"):
        assert sym in blob, sym
