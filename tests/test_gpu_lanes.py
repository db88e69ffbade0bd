"""The per-lane point kernels' field code against its limb-exact model, limb for limb (pytest -m gpu).

k_shift_bases, k_decompress_x, k_scale_points and the fixed-base kernels run a whole lane of lazy
field code per point and hand on canonical words, which cannot show a value that is right mod p but
outside its contract.  Here the functions they are made of run on raw limbs (msm_kernels.hip
k_test_limbs_lane, msm_amd._test_limb_op) over tests/_lane_catalogue.py, and k_fixed_eval's
accumulators are read back as it left them (msm_amd._test_fixed_proj); every output limb is compared
with tests/_fp29_model.py, built for the WIDE_* masks the loaded library reports.
"""
import random

import numpy as np
import pytest

import _fp29_model as F
import _lane_catalogue as L
import msm_amd as M
from oracle import oracle as O
from test_gpu_limbs import arr, compare, flat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def masks():
    return M._test_wide_masks()


@pytest.fixture(scope="module")
def cat():
    return L.catalogue()


@pytest.fixture(scope="module")
def exp(masks):
    return L.expected(masks)


def test_small_functions(cat, exp):
    for op, name in (("sqr", "fe_sqr"), ("std_neg", "fe_std_neg"), ("is_one", "fe_mul_out_is_one")):
        rows = cat[op]
        compare(name, M._test_limb_op(op, arr(rows)), exp[op], lambda i: rows[i])


def test_pt_from_record(cat, exp):
    rows = cat["from_record"]
    compare("pt_from_record", M._test_limb_op("from_record", arr(rows)), [flat(p) for p in exp["from_record"]],
            lambda i: rows[i])


def test_shift_lane(cat, exp):
    rows = cat["shift_lane"]
    got = M._test_limb_op("shift_lane", arr([r for r, _, _ in rows]), arr([[s] for _, s, _ in rows]))
    compare("k_shift_bases lane", got, exp["shift_lane"], lambda i: rows[i])


def test_shift_lane_count_is_bounded(cat):
    rec = cat["shift_lane"][0][0]
    with pytest.raises(M.MsmError):
        M._test_limb_op("shift_lane", arr([rec]), arr([[256]]))


def test_fe_sqrt_ts(cat, exp):
    rows = cat["sqrt_ts"]
    compare("fe_sqrt_ts", M._test_limb_op("sqrt_ts", arr([u for u, _, _ in rows])), exp["sqrt_ts"],
            lambda i: (rows[i], exp["sqrt_trace"][i]))


def test_pt_mul_order(cat, exp):
    rows = cat["mul_order"]
    compare("pt_mul_order", M._test_limb_op("mul_order", arr([flat(p) for p, _, _ in rows])),
            [flat(q) for q in exp["mul_order"]], lambda i: rows[i])


# ---- k_fixed_eval's accumulators, as the kernel left them --------------------------------------------
class _Rows:
    """A [n, 32] record array as the model reads it: rows of Python ints, converted when touched."""

    def __init__(self, a):
        self.a = a

    def __getitem__(self, i):
        return [int(x) for x in self.a[i]]


def _fixed_scalars(k, w, b, m):
    """m rows of k scalars below 2^b: 2^(w-1) (the largest digit), 2^w - 1 (a carry into the next
    window), 0 (nothing added) and the all-ones scalar (a carry through every window) first, then
    random ones; the last live lane is all ones in every base.  The shape of three rows has no room
    for the 0, which the other shapes hold."""
    rnd = random.Random(100 * k + w)
    edge = [1 << (w - 1), (1 << w) - 1, 0, (1 << b) - 1, 1, (1 << (w - 1)) + 1, (1 << (b - 1)), ((1 << b) - 1) // 3]
    rows = [[edge[(i + j) % len(edge)] for j in range(k)] for i in range(len(edge))]
    rows += [[v] * k for v in edge[:4]]
    rows += [[rnd.randrange(1 << b) for _ in range(k)] for _ in range(m)]
    rows = rows[:m]
    rows[-1] = [(1 << b) - 1] * k  # the last live lane: a carry through every window of every base
    return rows


@pytest.mark.parametrize("k,w,b,m", [(1, 4, 16, 65), (3, 5, 31, 130), (1, 12, 256, 3)])
def test_fixed_eval_accumulators(masks, k, w, b, m):
    import torch

    rows = _fixed_scalars(k, w, b, m)
    sc = O.ints_to_be_words([s for row in rows for s in row]).reshape(m, k, 8)
    d_sc = torch.from_numpy(np.ascontiguousarray(sc).view(np.int32)).cuda()
    d_out = torch.zeros((m, 32), dtype=torch.int32, device="cuda")
    with M.Bases.from_wire(M.gen_points(8, k0=3, step=7), levels=1) as src, \
            src.fixed_table(first=0, count=k, window_bits=w, scalar_bits=b) as t:
        inf = t.info
        assert (inf["bases"], inf["window_bits"], inf["scalar_bits"]) == (k, w, b)
        Wn = inf["windows"]
        t.mul_device(d_sc, d_out, m)
        proj = M._test_fixed_proj(m)
        with t._records_handle() as h:
            records = _Rows(M._test_bases_records(h, 0))
    assert proj.shape == ((m + 63) // 64 * 64, 27)
    want = []
    for row in rows:
        digits = [M._test_fixed_digits(s, b, w)[0] for s in row]
        assert all(len(ds) == Wn for ds in digits)
        X, Y, _, Z = F.fixed_eval_chain(records, digits, w, Wn, masks)
        want.append(X + Y + Z)
    ident = F.pt_identity()
    want += [ident[0] + ident[1] + ident[3]] * (len(proj) - m)  # lanes past m: the identity's own limbs
    compare("k_fixed_eval accumulator", proj, want, lambda i: rows[i] if i < m else "a lane past m")
