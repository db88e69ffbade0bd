"""CPU tests of the vector tables (include/msm.h msm_fixed_create_vector): the exported symbols, the
table's shape and the way a call is cut into parts, fold passes and slabs (msm_test_vector_plan: the
creation's own vector_table_plan and the evaluation's own vector_plan) against a restatement here, and
the argument rules that return before any device work."""
import ctypes
import subprocess

import pytest

import msm_amd as M

ENTRIES = ["msm_fixed_create_vector"]
HOOKS = ["msm_test_vector_plan", "msm_test_vector_slab", "msm_test_vector_group"]
MAX_BASES, MAX_BYTES, PART_CAP = 4096, 256 << 20, 256 << 20
FULL_LANES, FOLD = 1 << 18, 16
BLOCK_BYTES = 4 * 9 * 64 * 4  # X | Y | Z | T of 9 limbs for 64 rows


def _ceil(a, b):
    return -(-a // b)


def _table(k, w, b):
    b = b or 256
    wn = _ceil(b + 1, w)
    records = k * wn << (w - 1)
    return {"window_bits": w, "scalar_bits": b, "windows": wn, "records": records, "bytes": records * 128}


def _auto_w(k, b):
    """The widest w in 2..12 whose table fits the 256 MiB limit (w = 2 always does)."""
    return max(w for w in range(2, 13) if _table(k, w, b)["bytes"] <= MAX_BYTES)


def _cut(k, m, sw, cap=PART_CAP, forced=0):
    gmax = min(8, 64 // sw)
    if forced:
        G = min(forced, gmax)
    else:
        G = next((g for g in range(gmax, 1, -1) if m * _ceil(k, g) >= FULL_LANES), 1)
    P = _ceil(k, G)
    passes, p = 0, P
    while p > 1:
        p, passes = _ceil(p, FOLD), passes + 1
    per_block = (P + _ceil(P, FOLD)) * BLOCK_BYTES
    blocks = min(max(1, cap // per_block), max(1, _ceil(m, 64)))
    return {"G": G, "P": P, "passes": passes, "slab_rows": 64 * blocks, "part_bytes": blocks * per_block}


def test_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", M.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ENTRIES + HOOKS:
        assert name in exported, name
        assert hasattr(M.load(), name)
    assert hasattr(M.Bases, "vector_table")


@pytest.mark.parametrize("k", [1, 8, 9, 16, 17, 600, 4096])
def test_table_shape(k):
    for b in (0, 1, 64, 251, 256):
        for w in (0, 2, 5, 8, 12, 16):
            want = _table(k, w or _auto_w(k, b or 256), b)
            if want["bytes"] > MAX_BYTES:
                with pytest.raises(M.MsmError) as e:
                    M._test_vector_plan(k, w, b)
                assert e.value.code == -1
            else:
                assert M._test_vector_plan(k, w, b) == want, (k, w, b)
    if k <= 8:  # the records' count and place are msm_fixed_create's
        for w in (2, 8, 12):
            assert M._test_vector_plan(k, w, 256) == M._test_fixed_plan(k, w, 256)


def test_auto_width_is_the_widest_that_fits():
    assert [M._test_vector_plan(k)["window_bits"] for k in (1, 46, 47, 64, 256, 1024, 4096)] == [12, 12, 11, 11, 9, 6, 3]
    assert [M._test_vector_plan(k, 0, 64)["window_bits"] for k in (256, 1024, 4096)] == [11, 9, 6]
    for k in (1, 9, 100, 1000, 2000, 4096):
        for b in (1, 64, 256):
            p = M._test_vector_plan(k, 0, b)
            assert p["bytes"] <= MAX_BYTES
            wider = p["window_bits"] + 1
            assert wider == 13 or _table(k, wider, b)["bytes"] > MAX_BYTES


@pytest.mark.parametrize("k", [9, 16, 17, 600, 4096])
@pytest.mark.parametrize("sw", [1, 2, 8])
def test_cut_is_the_stated_rule(k, sw):
    for m in (1, 64, 65, 1 << 18):
        got = M._test_vector_plan(k, 2, 32 * sw, m, sw)
        want = _cut(k, m, sw)
        assert {n: got[n] for n in want} == want, (k, m, sw)
        G, P = got["G"], got["P"]
        assert 1 <= G <= 8 and G * sw <= 64 and P == _ceil(k, G)
        assert FOLD ** (got["passes"] - 1) < P <= FOLD ** got["passes"]  # passes = ceil(log_16 P)
        assert got["slab_rows"] % 64 == 0 and got["slab_rows"] >= 64
        assert got["part_bytes"] <= PART_CAP
        # the evaluation's P parts and the first pass's outputs, for every block of a slab
        assert got["part_bytes"] == got["slab_rows"] // 64 * (P + _ceil(P, FOLD)) * BLOCK_BYTES
        # enough lanes before a lane takes more than one base
        assert G == 1 or m * P >= FULL_LANES


def test_slab_and_group_hooks():
    try:
        M._test_vector_slab(1 << 20)
        for k, m, sw in ((17, 200, 8), (600, 3, 2), (4096, 1 << 18, 1)):
            got = M._test_vector_plan(k, 2, 32 * sw, m, sw)
            want = _cut(k, m, sw, cap=1 << 20)
            assert {n: got[n] for n in want} == want
            assert got["part_bytes"] <= 1 << 20 or got["slab_rows"] == 64  # one block at the least
        M._test_vector_slab(400_000)  # two blocks of 19 parts each
        assert M._test_vector_plan(17, 2, 256, 200, 8)["slab_rows"] == 128  # m = 200 runs as two slabs
        M._test_vector_slab(0)
        assert M._test_vector_plan(17, 2, 256, 200, 8)["slab_rows"] == 256
        for forced, sw, G in ((8, 8, 8), (8, 1, 8), (3, 8, 3), (100, 8, 8)):
            M._test_vector_group(forced)
            got = M._test_vector_plan(9, 2, 32 * sw, 5, sw)
            assert got["G"] == G and got["P"] == _ceil(9, G)
            want = _cut(9, 5, sw, forced=forced)
            assert {n: got[n] for n in want} == want
        M._test_vector_group(0)
        assert M._test_vector_plan(9, 2, 256, 5, 8)["G"] == 1
    finally:
        M._test_vector_slab(0)
        M._test_vector_group(0)


def test_plan_refusals():
    """k = 0 and 4097, a table over 256 MiB, w or b out of range: the creation's own plan refuses them."""
    for k, w, b in ((0, 8, 256), (4097, 2, 256), (4097, 0, 0), (4096, 4, 256), (4, 16, 256), (9, 1, 256), (9, 17, 256),
                    (9, 8, 257), (4096, 13, 1)):
        with pytest.raises(M.MsmError) as e:
            M._test_vector_plan(k, w, b)
        assert e.value.code == -1, (k, w, b)
    assert M._test_vector_plan(4096, 2, 256)["bytes"] < MAX_BYTES
    assert M._test_vector_plan(4096, 3, 256)["bytes"] < MAX_BYTES
    assert M._test_vector_plan(3, 16, 256)["bytes"] == 3 * 68 << 20


def test_fixed_create_still_refuses_nine_bases():
    with pytest.raises(M.MsmError) as e:
        M._test_fixed_plan(9, 8, 256)
    assert e.value.code == -1
    assert M._test_vector_plan(9, 8, 256)["records"] == 9 * 33 * 128


def test_argument_rules_return_before_device_work():
    L = M.load()
    vp = ctypes.c_void_p
    # no handle, and a token no creation handed out
    for t in (None, vp(0x7FFFFFF0)):
        h = vp(0xDEAD)
        assert L.msm_fixed_create_vector(t, None, 8, 256, None, ctypes.byref(h)) == -1
        assert h.value is None  # *out is cleared
    assert L.msm_fixed_create_vector(vp(1), None, 8, 256, None, None) == -1
    # the flags the entry does not take
    for opts in (M._opts(None, scalar_type="u32"), M._opts(None, scalar_type="u256"), M._opts(None, devices=[0]),
                 M._opts(13, windows=(0, 2)), M._opts(13, windows=(0, 2, 2)), M._opts(None, scalar_bits=64)):
        h = vp(0xDEAD)
        assert L.msm_fixed_create_vector(vp(1), None, 8, 256, opts, ctypes.byref(h)) == -1
        assert h.value is None
