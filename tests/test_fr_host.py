"""csrc/fr.cuh's arithmetic mod r on the host (msm_test_fr_op runs the functions the Fr vector kernels run) against
Python integers, the bound in fr_mont_mul's comment at its extremes, the constants, and the argument rules of
the msm_fr_* entries that return before any device work.  No GPU needed."""
import ctypes
import itertools
import random

import numpy as np
import pytest

import msm_amd as M

R = M.FR_MODULUS
RR = 1 << 256
R_INV = pow(RR, -1, R)
R2 = RR * RR % R
EDGES = [0, 1, 2, R - 1, R, R + 1, 1 << 251, 1 << 255, RR - 1, RR % R, R2]


def _pairs():
    rnd = random.Random(20240521)
    rand = []
    for i in range(2000):
        a = rnd.getrandbits(256)
        b = rnd.getrandbits(256) if i % 2 else rnd.randrange(R)
        rand.append((a, b))
    return list(itertools.product(EDGES, EDGES)) + rand


PAIRS = _pairs()


def test_constants_match_python():
    c = M._test_fr_constants()
    assert c["r_powers"] == [pow(RR, k, R) for k in range(4)]
    assert c["r_powers"][2] == R2 < R  # fr_to_mont's factor, canonical as fr_mont_mul's second operand must be
    assert c["threads"] == 256 and c["dot_cap"] * c["threads"] <= 1 << 19 and c["pow_steps"] >= 1


def test_mont_mul():
    # the precondition: any a < 2^256, b < r
    pairs = [(a, b) for a, b in PAIRS if b < R] + [(a, b % R) for a, b in PAIRS if b >= R]
    got = M._test_fr_op("mont_mul", [a for a, _ in pairs], [b for _, b in pairs])
    assert got == [a * b * R_INV % R for a, b in pairs]
    assert all(v < R for v in got)


def test_mont_mul_bound_at_its_extremes():
    """(a b + m r) / 2^256 < b + r < 2 r < 2^252 for every m < 2^256: the largest operands the function takes
    stay inside the one conditional subtract, and the result is exact."""
    a, b = RR - 1, R - 1
    assert (a * b + (RR - 1) * R) // RR < b + R < 2 * R < 1 << 252
    assert M._test_fr_op("mont_mul", [a, a, RR - 1], [b, 0, 1]) == [a * b * R_INV % R, 0, (RR - 1) * R_INV % R]


def test_mont_mul_refuses_a_second_operand_at_or_above_r():
    with pytest.raises(M.MsmError) as e:
        M._test_fr_op("mont_mul", [1], [R])
    assert e.value.code == -1


@pytest.mark.parametrize("name", ["add", "sub"])
def test_add_sub(name):
    pairs = [(a % R, b % R) for a, b in PAIRS] + [(a, b) for a, b in PAIRS if a < R and b < R]
    got = M._test_fr_op(name, [a for a, _ in pairs], [b for _, b in pairs])
    sign = 1 if name == "add" else -1
    assert got == [(a + sign * b) % R for a, b in pairs]
    for bad in ([R], [0]), ([0], [R]):
        with pytest.raises(M.MsmError):
            M._test_fr_op(name, *bad)


def test_to_mont_and_round_trip():
    vals = EDGES + [a for a, _ in PAIRS[len(EDGES) ** 2:]] + [b for _, b in PAIRS[len(EDGES) ** 2:]]
    mont = M._test_fr_op("to_mont", vals)
    assert mont == [v * RR % R for v in vals]
    assert M._test_fr_op("round_trip", vals) == [v % R for v in vals]
    # and through the function the wide scalar types already use
    back, ok = M._test_fr_from_mont(mont)
    assert back == [v % R for v in vals] and all(ok)


# ---- the entries' argument rules that need no device ------------------------------------------------
def _u32(vals):
    return np.ascontiguousarray(M.scalars_to_wire(vals))


def _combine(a, m, b=None, x=None, y=None, flags=0, in_form=0, out_form=0, reserved=0, opts=None, out=True):
    keep = [None if v is None else np.ascontiguousarray(v, dtype=np.uint32) for v in (a, b, x, y)]
    cb = M.FrCombine(*[None if v is None else v.ctypes.data for v in keep], flags, in_form, out_form, reserved)
    res = np.zeros((max(m, 1), 8), np.uint32)
    return M.load().msm_fr_combine(ctypes.byref(cb), m, opts, res.ctypes.data if out else None)


A2 = _u32([3, 4])
SCALAR_FLAGS = [M.MSM_FLAG_SCALAR_BITS, M.MSM_FLAG_SCALAR_TYPE, M.MSM_FLAG_SCALAR_FIELD, M.MSM_FLAG_DEVICES,
                M.MSM_FLAG_WINDOWS]


def test_entries_are_exported():
    L = M.load()
    for name in ("msm_fr_combine", "msm_fr_combine_device", "msm_fr_powers", "msm_fr_powers_device", "msm_fr_dot",
                 "msm_fr_dot_device", "msm_test_fr_op"):
        assert isinstance(getattr(L, name), ctypes._CFuncPtr)


@pytest.mark.parametrize("kw", [
    dict(in_form=2), dict(out_form=2), dict(in_form=0xffffffff), dict(reserved=1), dict(flags=8),
    dict(flags=M.MSM_FR_X_BROADCAST), dict(flags=M.MSM_FR_Y_BROADCAST, b=A2), dict(flags=M.MSM_FR_SUB),
    dict(y=A2), dict(out=False),
])
def test_combine_refuses_before_device_work(kw):
    assert _combine(A2, 2, **kw) == -1


def test_combine_refuses_a_null_first_operand_and_a_null_descriptor():
    cb = M.FrCombine(None, None, None, None, 0, 0, 0, 0)
    res = np.zeros((2, 8), np.uint32)
    assert M.load().msm_fr_combine(ctypes.byref(cb), 2, None, res.ctypes.data) == -1
    assert M.load().msm_fr_combine(None, 2, None, res.ctypes.data) == -1
    assert M.load().msm_fr_combine_device(None, 2, None, None, res.ctypes.data) == -1


@pytest.mark.parametrize("flag", SCALAR_FLAGS)
def test_scalar_and_list_flags_are_refused(flag):
    L = M.load()
    o = M.MsmOpts(0, 0, -1, flag)
    o.scalar_bits = 64
    assert _combine(A2, 2, opts=ctypes.byref(o)) == -1
    res = np.zeros((2, 8), np.uint32)
    g = _u32([5])
    assert L.msm_fr_powers(g.ctypes.data, None, 2, 0, ctypes.byref(o), res.ctypes.data) == -1
    assert L.msm_fr_powers_device(g.ctypes.data, None, 2, 0, ctypes.byref(o), None, res.ctypes.data) == -1
    out = (ctypes.c_uint32 * 8)()
    assert L.msm_fr_dot(A2.ctypes.data, None, 2, 0, 0, ctypes.byref(o), out) == -1
    assert L.msm_fr_dot_device(A2.ctypes.data, None, 2, 0, 0, ctypes.byref(o), None, out) == -1


def test_host_mont_inputs_at_or_above_r_are_refused_before_any_upload():
    good = M.scalars_to_wide([5, R - 1], "fr_mont").view(np.uint32).reshape(-1, 8)
    for bad_value in (R, R + 1, RR - 1):
        bad = good.copy()
        bad[1] = np.frombuffer(bad_value.to_bytes(32, "little"), dtype="<u4")
        one = bad[1:2]
        assert _combine(bad, 2, in_form=1) == -1
        assert _combine(good, 2, b=bad, in_form=1) == -1
        assert _combine(good, 2, x=bad, in_form=1) == -1
        assert _combine(good, 2, x=one, flags=M.MSM_FR_X_BROADCAST, in_form=1) == -1
        assert _combine(good, 2, b=good, y=one, flags=M.MSM_FR_Y_BROADCAST, in_form=1) == -1
        out = (ctypes.c_uint32 * 8)()
        assert M.load().msm_fr_dot(bad.ctypes.data, None, 2, 1, 0, None, out) == -1
        assert M.load().msm_fr_dot(good.ctypes.data, bad.ctypes.data, 2, 1, 0, None, out) == -1


def test_powers_and_dot_refuse_before_device_work():
    L = M.load()
    res = np.zeros((2, 8), np.uint32)
    g = _u32([5])
    out = (ctypes.c_uint32 * 8)()
    assert L.msm_fr_powers(None, None, 2, 0, None, res.ctypes.data) == -1
    assert L.msm_fr_powers(g.ctypes.data, None, 2, 2, None, res.ctypes.data) == -1
    assert L.msm_fr_powers(g.ctypes.data, None, 2, 0, None, None) == -1
    assert L.msm_fr_powers_device(g.ctypes.data, None, 2, 0, None, None, res.ctypes.data + 4) == -1  # misaligned
    assert L.msm_fr_dot(A2.ctypes.data, None, 2, 2, 0, None, out) == -1
    assert L.msm_fr_dot(A2.ctypes.data, None, 2, 0, 2, None, out) == -1
    assert L.msm_fr_dot(None, None, 2, 0, 0, None, out) == -1
    assert L.msm_fr_dot(A2.ctypes.data, None, 2, 0, 0, None, None) == -1
    assert L.msm_fr_dot_device(A2.ctypes.data + 4, None, 2, 0, 0, None, None, out) == -1  # misaligned


def test_device_pointer_rules_are_decided_from_the_values():
    """Alignment and overlap of a device call's pointers are refused before anything is enqueued, whatever
    the addresses hold: out may be exactly a or exactly b, nothing else may overlap it."""
    L = M.load()
    base = 1 << 20

    def call(a, out, m=4, b=None, x=None, flags=0):
        cb = M.FrCombine(a, b, x, None, flags, 0, 0, 0)
        return L.msm_fr_combine_device(ctypes.byref(cb), m, None, None, out)

    assert call(base + 4, base + 4096) == -1           # a misaligned
    assert call(base, base + 4096 + 8) == -1           # out misaligned
    assert call(base, base + 32) == -1                 # out one element into a
    assert call(base, base - 32) == -1                 # out ending inside a
    assert call(base, base + 8192, b=base + 8192 + 96) == -1  # b's last element is out's first
    assert call(base, base + 8192, x=base + 8192) == -1       # a multiplier may not be the output
    assert call(base, base + 8192, x=base + 8192 + 96, flags=M.MSM_FR_X_BROADCAST) == -1


def test_zero_length_calls_touch_nothing():
    L = M.load()
    g = _u32([5])
    out = (ctypes.c_uint32 * 8)(*([7] * 8))
    assert _combine(A2, 0) == 0
    assert L.msm_fr_powers(g.ctypes.data, None, 0, 0, None, None) == 0
    assert L.msm_fr_dot(None, None, 0, 0, 0, None, out) == 0 and list(out) == [7] * 8
    assert M.fr_combine(np.zeros((0, 8), np.uint32)).shape == (0, 8)
    assert M.fr_powers(3, 0).shape == (0, 8)


def test_python_forms_and_helpers():
    vals = [0, 1, R - 1, 12345]
    mont = M.scalars_to_wide(vals, "fr_mont")
    assert M.fr_to_ints(mont, "fr_mont") == vals
    assert M.fr_to_ints(M.scalars_to_wire([R, R + 5, RR - 1])) == [0, 5, (RR - 1) % R]
    with pytest.raises(ValueError):
        M.fr_combine([1], form="mont")
    with pytest.raises(ValueError):
        M.fr_fold([1, 2, 3], 5)
    with pytest.raises(ValueError):
        M.fr_combine([1, 2], b=[1, 2, 3])
