"""The compiled field and curve code against its bit-exact model, limb for limb (pytest -m gpu).

The raw-limb hooks (msm_kernels.hip k_test_limbs*, msm_amd._test_limb_op / _test_records) take the
9 u32 limbs of every operand as they are and return every output limb as it is; each test runs one
op family on the operand catalogue (tests/_fp29_catalogue.py, self-checked against plain integers by
tests/test_fp29_model.py) and compares with tests/_fp29_model.py on every limb -- not mod p.  The
model is built for the WIDE_* masks the loaded library reports, so an MSM_NARROW_DIGITS variant
loaded through MSM_AMD_LIB is checked by the same tests.
"""
import numpy as np
import pytest

import _fp29_catalogue as C
import _fp29_model as F
import msm_amd as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def masks():
    return M._test_wide_masks()


@pytest.fixture(scope="module")
def cat(masks):
    return C.catalogue(masks)


def arr(rows):
    return np.array(rows, dtype=np.uint32)


def flat(pt):
    return [x for c in pt for x in c]


def compare(name, got, exp, operands):
    """Every output limb; the first differing element is reported with its operands."""
    exp = arr(exp).reshape(got.shape)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{name}: {bad.size} of {len(exp)} elements differ; element {i}: operands "
                             f"{operands(i)}, device {got[i].tolist()}, model {exp[i].tolist()}")


def test_build_masks(masks):
    assert masks in (F.DEFAULT_MASKS, F.NARROW_MASKS)


def test_fe_mul_w(cat, masks):
    for name, wide in C.mul_masks(masks).items():
        cases = cat["mul"][name]
        got = M._test_limb_op("mul_" + name, arr([a for a, _ in cases]), arr([b for _, b in cases]))
        compare(f"fe_mul_w<{wide:#x}> ({name})", got, [F.fe_mul_exact(a, b, wide) for a, b in cases], lambda i: cases[i])


def test_fe_mul_sd(cat, masks):
    cases = cat["mul_sd"]
    exp = [F.fe_mul_sd_exact(a, b, masks[0]) for a, b in cases]
    for op in ("mul_sd_u", "mul_sd_s"):
        got = M._test_limb_op(op, arr([a for a, _ in cases]), arr([b for _, b in cases]))
        compare("fe_mul_sd " + op, got, exp, lambda i: cases[i])


def test_small_constant_scaling(cat):
    for op, fn in (("mul_2d", F.fe_mul_2d_limbs), ("mul_d", F.fe_mul_d_limbs)):
        cases = cat[op]
        compare("fe_" + op, M._test_limb_op(op, arr(cases)), [fn(a) for a in cases], lambda i: cases[i])


def test_carry_ops(cat):
    for op, fn in (("sub", F.fe_sub), ("add_n", F.fe_add_n)):
        cases = cat[op]
        got = M._test_limb_op(op, arr([a for a, _ in cases]), arr([b for _, b in cases]))
        compare("fe_" + op, got, [fn(a, b) for a, b in cases], lambda i: cases[i])
    for op, fn in (("neg", F.fe_neg), ("dbl_n", F.fe_dbl_n)):
        cases = cat[op]
        compare("fe_" + op, M._test_limb_op(op, arr(cases)), [fn(a) for a in cases], lambda i: cases[i])


def test_canonical_forms(cat, masks):
    for op, fn in (("to_std", F.fe_to_std), ("to_host_mont", F.fe_to_host_mont)):
        cases = cat[op]
        compare("fe_" + op, M._test_limb_op(op, arr(cases)), [fn(a, masks) for a in cases], lambda i: cases[i])


def test_fe_inv(cat, masks):
    cases = cat["inv"]
    compare("fe_inv", M._test_limb_op("inv", arr(cases)), [F.fe_inv(a, masks) for a in cases], lambda i: cases[i])


def test_words(cat):
    cases = cat["from_words"]
    compare("fe_from_words_le", M._test_limb_op("from_words", arr(cases)), [F.fe_from_words_le(w) for w in cases],
            lambda i: cases[i])
    cases = cat["to_words"]
    compare("fe_to_words_le", M._test_limb_op("to_words", arr(cases)), [F.fe_to_words_le(a) for a in cases],
            lambda i: cases[i])
    cases = cat["words_lt_p"]
    compare("words_lt_p", M._test_limb_op("words_lt_p", arr(cases)), [[int(F.words_lt_p(w))] for w in cases],
            lambda i: cases[i])


def test_pt_add_and_dbl(cat, masks):
    cases = cat["pt_add"]
    got = M._test_limb_op("pt_add", arr([flat(p) for p, _, _ in cases]), arr([flat(q) for _, q, _ in cases]))
    compare("pt_add", got, [flat(F.pt_add(p, q, masks)) for p, q, _ in cases], lambda i: cases[i])
    cases = cat["pt_dbl"]
    got = M._test_limb_op("pt_dbl", arr([flat(p) for p, _ in cases]))
    compare("pt_dbl", got, [flat(F.pt_dbl(p, masks)) for p, _ in cases], lambda i: cases[i])


def test_pt_madd(cat, masks):
    cases = cat["pt_madd"]
    got = M._test_limb_op("pt_madd", arr([flat(p) for p, _, _, _ in cases]), arr([flat(r) for _, r, _, _ in cases]),
                          arr([ng for _, _, ng, _ in cases]))
    exp = []
    for p, rec, ng, _ in cases:
        q = (rec[1], rec[0], F.kt_neg_if(rec[2], True)) if ng else rec
        exp.append(flat(F.pt_madd(p, q, masks)))
    compare("pt_madd", got, exp, lambda i: cases[i])


@pytest.mark.parametrize("count", C.QUAD_COUNTS)
def test_pt_add_quad(cat, masks, count):
    cases = cat["pt_add_quad"][count]
    got = M._test_limb_op("pt_add_quad", arr([flat(p) for p, _, _ in cases]), arr([flat(q) for _, q, _ in cases]))
    compare(f"pt_add_quad x{count}", got, [flat(F.pt_add_quad(p, q, masks)) for p, q, _ in cases], lambda i: cases[i])


@pytest.mark.parametrize("fmt", (F.PT_FMT_WIRE, F.PT_FMT_XY, F.PT_FMT_XYZ), ids=("wire", "xy", "xyz"))
def test_records(cat, masks, fmt):
    rc = cat["records"][fmt]
    rec, err, sums = M._test_records(fmt, arr(rc["inputs"]), rc["entries"], arr([flat(a) for a in rc["accs"]]))
    model = [F.prepare_record(w, fmt, masks) for w in rc["inputs"]]
    assert err == 0
    compare("k_prepare_points record", rec, [r for r, _ in model], lambda i: rc["inputs"][i])
    records = [r for r, _ in model]
    exp = [flat(F.pt_madd(acc, F.load_pre_signed(records, ent), masks)) for ent, acc in zip(rc["entries"], rc["accs"])]
    compare("load_pre_signed + pt_madd", sums, exp, lambda i: (rc["entries"][i], rc["accs"][i]))


def test_record_error_word(masks):
    bad = [F.be_words(F.P) + F.be_words(1) + F.be_words(1), F.be_words(0) + F.be_words(1) + F.be_words(0)]
    rec, err, _ = M._test_records(F.PT_FMT_XYZ, arr(bad))
    assert err == F.ERR_COORD_RANGE | F.ERR_BAD_POINT
    compare("k_prepare_points record (rejected input)", rec, [F.prepare_record(w, F.PT_FMT_XYZ, masks)[0] for w in bad],
            lambda i: bad[i])
