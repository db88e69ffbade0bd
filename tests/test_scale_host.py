"""CPU tests of the per-point scalar multiples (include/msm.h msm_bases_scale*): the exported symbols,
the ladder's digit function run on the host (msm_test_scale_digits calls the kernel's own scale_digit),
and the argument rules that return before any device work."""
import ctypes
import random
import subprocess

import numpy as np
import pytest

import msm_amd as M

ENTRIES = ["msm_bases_scale", "msm_bases_scale_device", "msm_bases_scale_create", "msm_bases_scale_create_device"]
BITS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 251, 253, 254, 255, 256]


def test_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", M.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ENTRIES + ["msm_test_scale_digits"]:
        assert name in exported, name
        assert hasattr(M.load(), name)


def _window_bits():
    """The ladder's window width w, from its trip count at 256 bits."""
    count = len(M._test_scale_digits(0, 256))
    assert 256 % count == 0
    return 256 // count


@pytest.mark.parametrize("b", BITS)
def test_digits_are_the_windows_of_the_integer(b):
    w = _window_bits()
    rnd = random.Random(1000 + b)
    values = [0, 1, (1 << b) - 1] + [1 << k for k in range(b)] + [rnd.getrandbits(b) for _ in range(40)]
    values += [rnd.getrandbits(b) | 1 << (b - 1) for _ in range(8)]
    for v in values:
        d = M._test_scale_digits(v, b)
        # the trip count depends on b alone (wave-uniform): the windows that b bits reach
        assert len(d) == -(-b // w), (b, v)
        assert sum(dj << (w * j) for j, dj in enumerate(d)) == v, (b, hex(v))
        for j, dj in enumerate(d):
            assert 0 <= dj < 1 << min(w, b - w * j), (b, j, hex(v))  # the top window may be partly filled


def test_digits_hook_argument_rules():
    L = M.load()
    sc = np.zeros(8, np.uint32)
    dg = np.zeros(256, np.uint32)
    cnt = ctypes.c_uint32()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    u32p = ctypes.POINTER(ctypes.c_uint32)
    assert L.msm_test_scale_digits(p(sc), 8, 256, dg.ctypes.data_as(u32p), ctypes.byref(cnt)) == 0
    for sw, b in ((8, 0), (8, 257), (7, 256), (2, 33 + 32)):
        assert L.msm_test_scale_digits(p(sc), sw, b, dg.ctypes.data_as(u32p), ctypes.byref(cnt)) == -1
    assert L.msm_test_scale_digits(None, 8, 256, dg.ctypes.data_as(u32p), ctypes.byref(cnt)) == -1


def _calls(handle, opts, out_ref):
    """The four entries on `handle` with valid-looking host arguments: their return codes."""
    L = M.load()
    vp = ctypes.c_void_p
    sc = np.zeros((4, 8), np.uint32)
    pts = np.zeros((4, 32), np.uint32)
    sub = M.Subset(0, 4, None)
    return [
        L.msm_bases_scale(handle, ctypes.byref(sub), sc.ctypes.data_as(vp), opts, pts.ctypes.data_as(vp)),
        L.msm_bases_scale_device(handle, ctypes.byref(sub), sc.ctypes.data_as(vp), opts, None, pts.ctypes.data_as(vp)),
        L.msm_bases_scale_create(handle, ctypes.byref(sub), sc.ctypes.data_as(vp), opts, 1, out_ref),
        L.msm_bases_scale_create_device(handle, ctypes.byref(sub), sc.ctypes.data_as(vp), opts, 1, None, out_ref),
    ]


def test_argument_rules_return_before_device_work():
    h = ctypes.c_void_p(0xDEAD)
    # a null handle, and a token no creation handed out
    for handle in (None, ctypes.c_void_p(0x7FFFFFF0)):
        assert _calls(handle, None, ctypes.byref(h)) == [-1] * 4
        assert h.value is None  # the create entries clear *out
        h = ctypes.c_void_p(0xDEAD)
    # a null `out`
    assert _calls(ctypes.c_void_p(1), None, None)[2:] == [-1, -1]
    # the flags the entries do not take, and a width outside 1..256
    for opts in (M._opts(None, scalar_type="u32"), M._opts(None, scalar_type="u256"), M._opts(None, devices=[0]),
                 M._opts(13, windows=(0, 2)), M._opts(13, windows=(0, 2, 2)), M._opts(None, scalar_bits=0),
                 M._opts(None, scalar_bits=257)):
        assert _calls(ctypes.c_void_p(1), opts, ctypes.byref(h)) == [-1] * 4
