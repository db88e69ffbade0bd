"""Native integer scalars on a resident-bases handle, the host-only part (include/msm.h
MSM_FLAG_SCALAR_TYPE): the plan of a typed launch is the narrow plan of its magnitude bits and the
upload is counted in bytes (msm_test_native_plan), the argument rules, the entries that refuse the
flag, and the Python side's packing and dtype inference.  No GPU needed."""
import ctypes
import re
import os

import numpy as np
import pytest

import msm_amd as M

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "msm.h")
TYPES = {"bit": 1, "u8": 8, "i8": 8, "u16": 16, "i16": 16, "u32": 32, "i32": 32, "u64": 64, "i64": 64}
SIZES = (1, 7, 8, 9, 4097)


def test_the_type_table_matches_the_header():
    src = open(HEADER).read()
    vals = {k.lower(): int(v) for k, v in re.findall(r"#define MSM_SCALAR_([A-Z0-9]+) (\d+)u", src)}
    assert vals == {k: v[0] for k, v in M.SCALAR_TYPES.items()}
    assert len(set(vals.values())) == len(vals) and 0 not in vals.values()
    assert {k: v[2] for k, v in M.SCALAR_TYPES.items()} == TYPES
    assert int(re.search(r"#define MSM_FLAG_SCALAR_TYPE (\d+)u", src).group(1)) == M.MSM_FLAG_SCALAR_TYPE == 32


def test_typed_opts_append_the_field_and_leave_the_short_struct_alone():
    assert ctypes.sizeof(M.MsmOpts) == 40
    assert M.MsmOptsTyped.scalar_type.offset == 40 and ctypes.sizeof(M.MsmOptsTyped) == 48
    assert M.MsmOptsTyped.window_hi.offset == M.MsmOpts.window_hi.offset
    o = M._opts(16, scalar_bits=5, scalar_type="i8")._obj
    assert isinstance(o, M.MsmOptsTyped) and o.scalar_type == M.SCALAR_TYPES["i8"][0]
    assert o.flags == M.MSM_FLAG_SCALAR_TYPE | M.MSM_FLAG_SCALAR_BITS and o.scalar_bits == 5
    o = M._opts(None, scalar_type="u64")._obj
    assert o.flags == M.MSM_FLAG_SCALAR_TYPE
    o = M._opts(16, scalar_bits=5)._obj
    assert type(o) is M.MsmOpts and not o.flags & M.MSM_FLAG_SCALAR_TYPE


@pytest.mark.parametrize("ty", TYPES)
def test_plan_is_the_narrow_plan_of_the_magnitude_bits(ty):
    e = TYPES[ty]
    shared = ("c", "windows", "q", "nhi", "words", "packed")
    for n in SIZES + (1 << 20,):
        for b in range(1, e + 1):
            for c in (0, 4, 13, 16, 17, 20):
                p = M._test_native_plan(n, ty, b, c)
                q = M._test_narrow_plan(n, b, c)
                assert {k: p[k] for k in shared} == q, (ty, n, b, c)
                assert p["vector_bytes"] == -(-n * e // 8), (ty, n)
                assert p["region_bytes"] == -(-p["vector_bytes"] // 16) * 16, (ty, n)


def test_u8_and_i8_share_the_plan():
    for b in (1, 4, 8):
        assert M._test_native_plan(4097, "u8", b) == M._test_native_plan(4097, "i8", b)


def test_plan_argument_errors():
    def invalid(*a):
        with pytest.raises(M.MsmError) as err:
            M._test_native_plan(4097, *a)
        assert err.value.code == -1, a

    for ty in (0, 10, 255, 1 << 31):
        invalid(ty, 1, 16)
    for ty, e in TYPES.items():
        invalid(ty, 0, 16)
        invalid(ty, e + 1, 16)
        invalid(ty, 257, 16)
    invalid("bit", 2, 16)
    for c in (3, 21):
        with pytest.raises(M.MsmError) as err:
            M._test_native_plan(4097, "i64", 64, c)
        assert err.value.code == -2, c


# ---- the flag belongs to msm_bases_compute* ---------------------------------------------------------
def test_other_entries_refuse_the_flag_before_any_device_work():
    L = M.load()
    n = 4
    pts = np.ascontiguousarray(M.gen_points(n))
    sc = np.ascontiguousarray(M.gen_scalars(n))
    out = np.zeros(16, np.uint32)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    pp = (ctypes.c_void_p * 1)(pts.ctypes.data)
    ss = (ctypes.c_void_p * 1)(sc.ctypes.data)
    for bits in (None, 8):
        o = M._opts(None, scalar_bits=bits, scalar_type="i8")
        assert L.msm_compute(pts.ctypes.data, sc.ctypes.data, n, o, op) == -1
        # (host addresses: the flag is refused before either pointer is looked at)
        assert L.msm_compute_device(pts.ctypes.data, sc.ctypes.data, n, o, None, op) == -1
        assert L.msm_compute_shared(pts.ctypes.data, ctypes.cast(ss, ctypes.c_void_p), n, 1, o, op) == -1
        assert L.msm_compute_many(ctypes.cast(pp, ctypes.c_void_p), ctypes.cast(ss, ctypes.c_void_p), n, 1, o,
                                  op) == -1
        assert L.msm_compute_cocompute(pts.ctypes.data, sc.ctypes.data, n, o, 0.5, 1, op) == -1
        h = ctypes.c_void_p()
        assert L.msm_bases_create(pts.ctypes.data, n, o, 1, ctypes.byref(h)) == -1
        assert not h.value
        assert L.msm_bases_create_device(pts.ctypes.data, n, o, 1, None, ctypes.byref(h)) == -1
        part = np.zeros(32, np.uint32)
        assert L.msm_compute_partial(pts.ctypes.data, sc.ctypes.data, n, o,
                                     part.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) == -1


# ---- packing ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYPES)
def test_scalars_to_native_round_trips_and_refuses_values_that_do_not_fit(ty):
    e = TYPES[ty]
    signed = ty[0] == "i"
    lo, hi = (-(1 << (e - 1)), (1 << (e - 1)) - 1) if signed else (0, (1 << e) - 1)
    vals = [0, 1, hi, lo, 1, 0, hi, hi, lo, 1, 1][:11]
    a = M.scalars_to_native(vals, ty)
    if ty == "bit":
        assert a.dtype == np.uint8 and a.shape == (2,)
        assert np.unpackbits(a, bitorder="little")[:len(vals)].tolist() == vals
        assert (a == np.packbits(np.array(vals, np.uint8), bitorder="little")).all()
    else:
        assert a.dtype == M.SCALAR_TYPES[ty][1] and a.shape == (len(vals),)
        assert [int(v) for v in a] == vals
    assert M.scalars_to_native([], ty).shape == (0,)
    for bad in (hi + 1, lo - 1):
        with pytest.raises(ValueError):
            M.scalars_to_native([1, bad], ty)
    with pytest.raises(ValueError):
        M.scalars_to_native([1], "u128")


def test_native_infers_the_type_from_the_dtype():
    for ty, (_, dt, _) in M.SCALAR_TYPES.items():
        if ty != "bit":
            assert M._native_type(np.zeros(3, dt), "native", None) == (ty, None)
            assert M._native_type(np.zeros(3, dt), "native", 5) == (ty, 5)
    assert M._native_type(np.zeros(3, np.bool_), "native", None) == ("u8", 1)
    assert M._native_type(np.zeros(3, np.bool_), "native", 8) == ("u8", 8)
    for dt in (np.float32, np.float64, np.complex64):
        with pytest.raises(TypeError):
            M._native_type(np.zeros(3, dt), "native", None)
    with pytest.raises(TypeError):
        M._native_type([1, 2, 3], "native", None)
    assert M._native_type(np.zeros(3, np.uint32), None, 7) == (None, 7)
    assert M._native_type([1, 2], "i16", None) == ("i16", None)
    with pytest.raises(ValueError):
        M._native_type(np.zeros(3, np.int8), "i128", None)


def test_native_infers_the_type_from_a_torch_dtype():
    import torch

    for dt, ty in ((torch.int8, "i8"), (torch.uint8, "u8"), (torch.int16, "i16"), (torch.int32, "i32"),
                   (torch.int64, "i64")):
        assert M._native_type(torch.zeros(3, dtype=dt), "native", None) == (ty, None)
    assert M._native_type(torch.zeros(3, dtype=torch.bool), "native", None) == ("u8", 1)
    with pytest.raises(TypeError):
        M._native_type(torch.zeros(3, dtype=torch.float16), "native", None)


def test_typed_host_arrays_pass_through_uncopied():
    a = np.arange(-5, 5, dtype=np.int16)
    assert M._native_host(a, "i16").ctypes.data == a.ctypes.data
    m = np.array([True, False, True])
    assert M._native_host(m, "u8").ctypes.data == m.ctypes.data
    assert M._native_host(a[::2], "i16").tolist() == a[::2].tolist()  # not contiguous: copied
    assert M._native_host([-1, 2], "i8").tolist() == [-1, 2]
    with pytest.raises(TypeError):
        M._native_host(a, "u16")
    with pytest.raises(ValueError):
        M._native_len(np.zeros(2, np.uint8), "bit", None)
    with pytest.raises(ValueError):
        M._native_len(np.zeros(2, np.uint8), "bit", 17)
    assert M._native_len(np.zeros(2, np.uint8), "bit", 16) == 16
