"""CPU tests of the pairwise combinations (include/msm.h msm_bases_combine*): the exported symbols, the
joint ladder's digit function run on the host (msm_test_combine_digits calls the kernel's own
combine_digit), and the argument rules that return before any device work."""
import ctypes
import random
import subprocess

import numpy as np
import pytest

import msm_amd as M

ENTRIES = ["msm_bases_combine", "msm_bases_combine_device", "msm_bases_combine_create",
           "msm_bases_combine_create_device"]
BITS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 251, 253, 254, 255, 256]


def test_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", M.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ENTRIES + ["msm_test_combine_digits"]:
        assert name in exported, name
        assert hasattr(M.load(), name)


@pytest.mark.parametrize("b", BITS)
def test_digits_are_the_bit_pairs(b):
    rnd = random.Random(2000 + b)
    full = (1 << b) - 1
    pairs = [(0, 0), (full, 0), (0, full), (full, full), (1, 1 << (b - 1)), (1 << (b - 1), 1)]
    pairs += [(1 << k, 0) for k in range(b)] + [(0, 1 << k) for k in range(b)]
    pairs += [(rnd.getrandbits(b), rnd.getrandbits(b)) for _ in range(40)]
    for a, v in pairs:
        d = M._test_combine_digits(a, v, b)
        # the trip count depends on b alone (wave-uniform): one digit per bit
        assert len(d) == b, (b, a, v)
        for j, dj in enumerate(d):
            assert dj == ((a >> j) & 1) + 2 * ((v >> j) & 1), (b, j, hex(a), hex(v))


@pytest.mark.parametrize("b", [x for x in BITS if x % 32])
def test_a_bit_above_the_width_reaches_no_digit(b):
    """The top word's bits at or above b (the kernel flags them) are read by no digit."""
    L = M.load()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    sw = (b + 31) // 32
    rnd = random.Random(3000 + b)
    a, v = rnd.getrandbits(b), rnd.getrandbits(b)
    sa, sb = M.scalars_to_wire([a], b).copy(), M.scalars_to_wire([v], b).copy()
    clean = M._test_combine_digits(a, v, b)
    cnt = ctypes.c_uint32()
    for stray in range(b % 32, 32):
        for arr in (sa, sb):
            dirty = arr.copy()
            dirty[0, 0] |= np.uint32(1 << stray)
            pa, pb = (dirty, sb) if arr is sa else (sa, dirty)
            dg = np.zeros(256, np.uint32)
            assert L.msm_test_combine_digits(pa.ctypes.data_as(ctypes.c_void_p), pb.ctypes.data_as(ctypes.c_void_p), sw, b,
                                             dg.ctypes.data_as(u32p), ctypes.byref(cnt)) == 0
            assert cnt.value == b and [int(x) for x in dg[:b]] == clean and not dg[b:].any()


def test_digits_hook_argument_rules():
    L = M.load()
    sc = np.zeros(8, np.uint32)
    dg = np.zeros(256, np.uint32)
    cnt = ctypes.c_uint32()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    u32p = ctypes.POINTER(ctypes.c_uint32)
    assert L.msm_test_combine_digits(p(sc), p(sc), 8, 256, dg.ctypes.data_as(u32p), ctypes.byref(cnt)) == 0
    assert cnt.value == 256
    for sw, b in ((8, 0), (8, 257), (7, 256), (2, 33 + 32)):
        assert L.msm_test_combine_digits(p(sc), p(sc), sw, b, dg.ctypes.data_as(u32p), ctypes.byref(cnt)) == -1
    assert L.msm_test_combine_digits(None, p(sc), 8, 256, dg.ctypes.data_as(u32p), ctypes.byref(cnt)) == -1
    assert L.msm_test_combine_digits(p(sc), None, 8, 256, dg.ctypes.data_as(u32p), ctypes.byref(cnt)) == -1
    assert L.msm_test_combine_digits(p(sc), p(sc), 8, 256, None, ctypes.byref(cnt)) == -1
    assert L.msm_test_combine_digits(p(sc), p(sc), 8, 256, dg.ctypes.data_as(u32p), None) == -1


def _combine(m_a=4, m_b=4, flags=0, reserved=0, a=True, b=True):
    """A msm_combine_t with valid-looking host arguments, and the arrays it points at."""
    sa, sb = np.zeros((4, 8), np.uint32), np.zeros((4, 8), np.uint32)
    vp = ctypes.c_void_p
    cb = M.Combine(None, M.Subset(0, m_a, None), M.Subset(0, m_b, None), sa.ctypes.data_as(vp) if a else None,
                   sb.ctypes.data_as(vp) if b else None, flags, reserved)
    return cb, (sa, sb)


def _calls(handle, cb, opts, out_ref):
    """The four entries on `handle`: their return codes."""
    L = M.load()
    vp = ctypes.c_void_p
    pts = np.zeros((4, 32), np.uint32)
    ref = ctypes.byref(cb) if cb is not None else None
    return [
        L.msm_bases_combine(handle, ref, opts, pts.ctypes.data_as(vp)),
        L.msm_bases_combine_device(handle, ref, opts, None, pts.ctypes.data_as(vp)),
        L.msm_bases_combine_create(handle, ref, opts, 1, out_ref),
        L.msm_bases_combine_create_device(handle, ref, opts, 1, None, out_ref),
    ]


HANDLES = [None, ctypes.c_void_p(0x7FFFFFF0), ctypes.c_void_p(1)]


@pytest.mark.parametrize("handle", HANDLES, ids=["null", "unknown", "one"])
def test_argument_rules_return_before_device_work(handle):
    def refused(cb, opts=None):
        h = ctypes.c_void_p(0xDEAD)
        assert _calls(handle, cb, opts, ctypes.byref(h)) == [-1] * 4
        assert h.value is None  # the create entries clear *out

    cb, keep = _combine()
    refused(cb)                                   # the handle itself: null, or a token no creation handed out
    refused(None)                                 # a null combine struct
    refused(_combine(m_a=4, m_b=3)[0])            # a.m != b.m
    for flags in (8, 1 << 31, 0xFFFFFFF8):
        refused(_combine(flags=flags)[0])         # an unknown flag bit
    refused(_combine(reserved=1)[0])
    refused(_combine(flags=M.MSM_COMBINE_A_BROADCAST, a=False)[0])   # a broadcast flag without its scalars
    refused(_combine(flags=M.MSM_COMBINE_B_BROADCAST, b=False)[0])
    # the flags the entries do not take, and a width outside 1..256
    for opts in (M._opts(None, scalar_type="u32"), M._opts(None, scalar_type="u256"), M._opts(None, devices=[0]),
                 M._opts(13, windows=(0, 2)), M._opts(13, windows=(0, 2, 2)), M._opts(None, scalar_bits=0),
                 M._opts(None, scalar_bits=257)):
        refused(cb, opts)
    # a null `out`
    assert _calls(handle, cb, None, None)[2:] == [-1, -1]
