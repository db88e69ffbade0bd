"""GPU tests of the launch layer's kernel tables (csrc/host_launch.h): every recode kernel that
recode_kernel can pick and every k_part_scatter instantiation of scatter_kernel, each launched, captured and
then replayed on new input at a new device address (repoint_inputs), bit-exact against the closed form over
k G bases (tests/_closed_form.py) -- never against another entry of the library.  A kernel missing from
is_recode_kernel's tables, a stale input pointer or an argument list of the wrong length shows as a wrong
second result.  (The chunk lengths of RED1_TABLE: tests/test_gpu_red_knobs.py, tests/test_gpu_red_state.py.)

n = 257 throughout: one full k_prepare_points block and a ragged one, the smallest n at which both branches
of the staging loops run.  The whole file, measured on an MI355X: 19 tests in 2.2 s, 1.6 s of it the first handle's creation."""
import functools
import random

import numpy as np
import pytest

import msm_amd as M
from _closed_form import closed_form, scalar_dot
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N = 257
K0, STEP = 3, 7  # the bases: P_i = (K0 + i STEP) G
R = O.R_ORDER

# name -> (value range, how a call says the format, handle levels and width, the call's width)
# and the recode kernel the plan takes (csrc/host_launch.h recode_kernel)
WIRE = (0, (1 << 256) - 1)
RECODES = {
    "wire-c10": (WIRE, {}, (1, None), 10),                 # k_recode_hist<u16>
    "wire-c13": (WIRE, {}, (1, None), 13),                 # k_recode_fixed<12, 14, FULL>
    "wire-c14": (WIRE, {}, (1, None), 14),                 # k_recode_fixed<13, 7, FULL>
    "wire-c15": (WIRE, {}, (1, None), 15),                 # k_recode_fixed<14, 16, FULL>
    "wire-c16": (WIRE, {}, (1, None), 16),                 # k_recode_fixed<15, 14, FULL>
    "wire-c15-folded": (WIRE, {}, (2, 15), None),          # a window range: k_recode_fixed<14, 16, not FULL>
    "wire-c17": (WIRE, {}, (1, None), 17),                 # k_recode_hist<u32>
    "narrow64": ((0, (1 << 64) - 1), dict(scalar_bits=64), (1, None), None),     # k_recode_narrow, two words
    "i16": ((-(1 << 15), (1 << 15) - 1), dict(scalar_type="i16"), (1, None), None),   # k_recode_native
    "u64": ((0, (1 << 64) - 1), dict(scalar_type="u64"), (1, None), None),       # k_recode_native
    "u128": ((0, (1 << 128) - 1), dict(scalar_type="u128"), (1, None), None),    # k_recode_wide
    "fr_mont": ((0, R - 1), dict(scalar_type="fr_mont"), (1, None), None),       # k_recode_wide
    "u256": (WIRE, dict(scalar_type="u256", scalar_bits=256), (1, None), None),  # k_recode_hist_le
}


@functools.lru_cache(maxsize=None)
def _points(n=N):
    pts = O.gen_points(n, k0=K0, step=STEP)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _values(lo, hi, seed):
    """N values of [lo, hi]: the greatest, the least and 0, then random ones."""
    rnd = random.Random(4100 + seed + hi.bit_length())
    return (hi, lo, 0) + tuple(rnd.randint(lo, hi) for _ in range(N - 3))


def _words(vals):
    """The values mod r as wire scalars: what the closed form takes."""
    return O.ints_to_be_words([v % R for v in vals])


def _pack(vals, how):
    ty = how.get("scalar_type")
    if ty in M.WIDE_TYPES:
        return M.scalars_to_wide(vals, ty)
    if ty:
        return M.scalars_to_native(vals, ty)
    return M.scalars_to_wire(list(vals), how.get("scalar_bits"))


def _dev(a):
    """A host array's bytes in a device tensor of its own: [rows, bytes per row] uint8."""
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1).copy()).cuda()


@pytest.fixture(scope="module")
def handles():
    """(levels, width) -> a handle over the N bases, and "wide": one over 2 N bases for the subsets."""
    hs = {key: M.Bases.from_wire(_points(), levels=key[0], window_size=key[1])
          for key in {case[2] for case in RECODES.values()}}
    hs["wide"] = M.Bases.from_wire(_points(2 * N), levels=1)
    yield hs
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("case", RECODES)
def test_every_recode_kernel_replayed_on_new_input(case, handles):
    (lo, hi), how, key, c = RECODES[case]
    vals = [_values(lo, hi, seed) for seed in range(2)]
    exp = [closed_form(K0, STEP, _words(v)) for v in vals]
    assert exp[0] != exp[1]
    dev = [_dev(_pack(v, how)) for v in vals]  # both alive: two addresses
    assert dev[0].data_ptr() != dev[1].data_ptr()
    h = handles[key]
    assert h.info["levels"] == key[0]
    got = [h.compute_device(d, window_size=c, **how) for d in dev]  # the capture, then its replay repointed
    assert got[0] == exp[0], case
    assert got[1] == exp[1], case
    assert got[1] != exp[0], case


@pytest.mark.parametrize("c", [13, 17])  # 16-bit and 32-bit digit codes
@pytest.mark.parametrize("form", ["plain", "range", "indexed"])
def test_every_scatter_instantiation(form, c, handles):
    import torch

    rnd = np.random.RandomState(17 * c + len(form))
    vals = [_values(*WIRE, seed) for seed in range(2)]
    dev = [_dev(_pack(v, {})) for v in vals]
    if form == "plain":
        idx = [np.arange(N)] * 2
        call = [lambda d=d: handles[(1, None)].compute_device(d, window_size=c) for d in dev]
    elif form == "range":
        idx = [N + np.arange(N)] * 2
        call = [lambda d=d: handles["wide"].compute_subset_device(d, first=N, m=N, window_size=c) for d in dev]
    else:
        idx = [rnd.randint(0, 2 * N, size=N) for _ in range(2)]
        for i in idx:
            i[:3] = (2 * N - 1, 0, i[5])  # the last record, the first, a repeat
        d_idx = [torch.from_numpy(i.astype(np.int32)).cuda() for i in idx]  # two index buffers too
        call = [lambda d=d, t=t: handles["wide"].compute_subset_device(d, indices=t, window_size=c)
                for d, t in zip(dev, d_idx)]
    exp = [O.scalar_mul(O.G, scalar_dot((K0 + STEP * i).astype(np.uint64), _words(v)) % R) for i, v in zip(idx, vals)]
    assert exp[0] != exp[1]
    got = [f() for f in call]
    assert got[0] == exp[0], (form, c)
    assert got[1] == exp[1], (form, c)
    assert got[1] != exp[0], (form, c)
