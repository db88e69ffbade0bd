"""The bit-exact limb model (tests/_fp29_model.py) against plain integers, on the whole operand
catalogue (tests/_fp29_catalogue.py): value mod p, and the range and normalisation fp29.cuh / ec.cuh
state for each function.  Together with the catalogue's coverage conditions this shows the
reference alone is right at every entry before tests/test_gpu_limbs.py asks the device.
"""
import os
import re

import pytest

import _fp29_catalogue as C
import _fp29_model as F
from _fp29_model import LB, M32, MASK, NL, P, R, RINV, value_of
from oracle import oracle as O

MASK_SETS = [F.DEFAULT_MASKS, F.NARROW_MASKS]
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "webgpu-msm_amd", "csrc")


def normalised(r):
    return all(0 <= x <= MASK for x in r[:NL - 1]) and 0 <= r[NL - 1] <= M32


def test_model_constants_match_header():
    src = open(os.path.join(_CSRC, "fp29.cuh")).read()
    for name in ("P29", "R2_29", "ONE29", "R2H_29", "HALF29", "R256_29", "K8P29", "K5P29"):
        m = re.search(r"uint32_t " + name + r"\[NL\] = \{([^}]*)\}", src)
        assert [int(x.strip().rstrip("u")) for x in m.group(1).split(",")] == getattr(F, name), name
    dev = open(os.path.join(_CSRC, "msm_dev.h")).read()
    for name in ("PRE_WORDS", "PRE_HALF", "PRE_KT"):
        assert int(re.search(r"constexpr uint32_t " + name + r" = (\d+);", dev).group(1)) == getattr(F, name)
    assert sum(x << (32 * i) for i, x in enumerate(F.PW)) == P


def test_limb_op_table_matches_kernels():
    """msm_amd._LIMB_OPS numbers the ops as the LimbOp enum of msm_kernels.hip does."""
    import msm_amd as M
    src = open(os.path.join(_CSRC, "msm_kernels.hip")).read()
    body = re.search(r"enum LimbOp : int \{(.*?)LOP_COUNT", re.sub(r"//[^\n]*", "", src), re.S).group(1)
    names = [n.strip().split("=")[0].strip() for n in body.split(",") if n.strip()]
    alias = {"mul_sd_u": "LOP_MUL_SD_U", "mul_sd_s": "LOP_MUL_SD_S", "pt_add_quad": "LOP_PT_QUAD"}
    assert [alias.get(k, "LOP_" + k.upper()) for k in M._LIMB_OPS] == names
    assert [v[0] for v in M._LIMB_OPS.values()] == list(range(len(names)))


@pytest.mark.parametrize("masks", MASK_SETS, ids=("wide", "narrow"))
def test_fe_mul_w_catalogue(masks):
    cat = C.catalogue(masks)
    for name, wide in C.mul_masks(masks).items():
        hit = set()
        for a, b in cat["mul"][name]:
            tr = []
            r = F.fe_mul_exact(a, b, wide, tr)
            v = value_of(r)
            assert v % P == value_of(a) * value_of(b) * RINV % P, (name, a, b)
            assert v < 2 * P and normalised(r), (name, a, b)
            for k, (lo, m, _) in enumerate(tr):
                hit.add((k, lo if F.is_wide(wide, k) else lo & MASK))
                assert m == (~lo & (M32 if F.is_wide(wide, k) else MASK))
        missing = [(k, t) for k in range(NL) for t in C.mul_digit_targets(wide, k) if (k, t) not in hit]
        assert not missing, f"mask {name}: digit edges (step, low word) never reached: {missing}"


@pytest.mark.parametrize("masks", MASK_SETS, ids=("wide", "narrow"))
def test_fe_mul_sd_catalogue(masks):
    wide = masks[0]
    hit = set()
    for a, b in C.catalogue(masks)["mul_sd"]:
        tr = []
        r = F.fe_mul_sd_exact(a, b, wide, tr)
        v = value_of(r)
        assert v % P == F.signed_value_of(a) * F.signed_value_of(b) * RINV % P, (a, b)
        assert 0 <= v < 2 * P and normalised(r), (a, b)
        hit |= C.sd_marks(tr, wide)
    if masks != F.DEFAULT_MASKS:
        return  # the sign coverage is a condition on the shipped masks (see the catalogue's note)
    missing = sorted(C.sd_targets(wide) - hit, key=str)
    assert not missing, f"signed multiply: (step, kind, sign) never reached: {missing}"


def test_sd_top_carries_are_negative():
    """Why the catalogue holds no positive carry out of columns 15 and 16 of fe_mul_sd: none exists
    for operands in pt_madd's forms (|limbs| < 2^30 + 2^29, top limbs of values < 10p)."""
    lim, top = 3 << 29, (10 * P) >> (LB * (NL - 1))  # generous per-limb bounds of every call site
    red15 = M32 * F.P29[8] + MASK * F.P29[7]          # digits 7 (up to 32 bits) and 8 (29 bits)
    bias15 = F.P29[7] << F.DELTA_SD_LOG
    carry14 = (3 * lim * lim + 9 * M32 * MASK + (1 << 63)) >> LB  # column 14 and everything carried into it
    assert 2 * lim * top + red15 + bias15 + carry14 < 1 << 58     # so register 15 = column - 2^58 < 0
    # register 17 = 2^29 + carry_16 is the result's top limb, < 2^22 for a value < 2p: carry_16 < 0
    assert F.sd_seed(0xFF, 17) == 1 << 29 and (2 * P) >> (LB * (NL - 1)) < 1 << 22


def test_small_constant_scaling():
    cat = C.catalogue()
    for a in cat["mul_2d"]:
        r = F.fe_mul_2d_limbs(a)
        assert value_of(r) % P == F.K2D_INT * value_of(a) % P and value_of(r) < 3 * P and normalised(r), a
    for a in cat["mul_d"]:
        r = F.fe_mul_d_limbs(a)
        assert value_of(r) % P == F.KD_INT * value_of(a) % P and value_of(r) < 2 * P and normalised(r), a


def test_carry_ops():
    cat = C.catalogue()
    full_ripple = 0
    for a, b in cat["sub"]:
        r = F.fe_sub(a, b)
        assert value_of(r) == value_of(a) + 8 * P - value_of(b) and normalised(r), (a, b)
        u = F.fe_sub_u(a, b)
        full_ripple += u[0] >> LB == 1 and all(x == MASK for x in u[1:NL - 1])  # each limb carries only what it is handed
        if a == b:
            assert r == F.limbs_of(8 * P)
    assert full_ripple, "no fe_sub entry carries out of limb 0 through all eight limbs"
    for b in cat["neg"]:
        r = F.fe_neg(b)
        assert value_of(r) == 8 * P - value_of(b) and normalised(r), b
    for a, b in cat["add_n"]:
        r = F.fe_add_n(a, b)
        assert value_of(r) == value_of(a) + value_of(b) and normalised(r), (a, b)
    for a in cat["dbl_n"]:
        r = F.fe_dbl_n(a)
        assert value_of(r) == 2 * value_of(a) and normalised(r), a
    # the unnormalised differences of pt_add and of a negated record
    for a, b in cat["add_n"]:
        if value_of(b) < 2 * P:
            assert value_of(F.fe_sub_v(a, b)) == value_of(a) + 5 * P - value_of(b)
            assert value_of(F.kt_neg_if(b, True)) == 5 * P - value_of(b) and F.kt_neg_if(b, False) == b


def test_canonical_forms():
    cat = C.catalogue()
    one = [1] + [0] * (NL - 1)
    exact_p = {"to_std": 0, "to_host_mont": 0}
    for a in cat["to_std"]:
        r = F.fe_to_std(a)
        assert r == F.limbs_of(value_of(a) * RINV % P), a
        exact_p["to_std"] += F.fe_norm(F.fe_mul(a, one)) == F.P29
    for a in cat["to_host_mont"]:
        r = F.fe_to_host_mont(a)
        assert r == F.limbs_of(value_of(a) * RINV * (1 << 256) % P), a
        exact_p["to_host_mont"] += F.fe_norm(F.fe_mul(a, F.R256_29)) == F.P29
    assert exact_p["to_std"] >= 3 and exact_p["to_host_mont"] >= 3, exact_p  # p itself before the subtraction
    for v in (0, 1, P - 1):
        assert not F.fe_geq_p(F.limbs_of(v)) or v >= P
    assert F.fe_geq_p(F.P29) and F.fe_sub_p(F.P29) == [0] * NL and F.fe_sub_p(F.limbs_of(P + 1)) == one
    assert not F.fe_geq_p(F.limbs_of(P - 1)) and F.fe_geq_p(F.limbs_of(2 * P - 1))


def test_fe_inv():
    for a in C.catalogue()["inv"]:
        r = F.fe_inv(a)
        assert value_of(r) * value_of(a) % P == R * R % P, a
        assert value_of(r) < 2 * P and normalised(r)


def test_words():
    cat = C.catalogue()
    for w in cat["from_words"]:
        v = sum(x << (32 * i) for i, x in enumerate(w))
        r = F.fe_from_words_le(w)
        assert value_of(r) == v and normalised(r), w
    for a in cat["to_words"]:
        w = F.fe_to_words_le(a)
        assert sum(x << (32 * i) for i, x in enumerate(w)) == value_of(a) and all(0 <= x <= M32 for x in w), a
    for w in cat["words_lt_p"]:
        assert F.words_lt_p(w) == (sum(x << (32 * i) for i, x in enumerate(w)) < P), w
    assert sum(1 for w in cat["words_lt_p"] if sum(a != b for a, b in zip(w, F.PW)) == 1) >= 15


def affine_of(pt):
    X, Y, T, Z = (value_of(c) * RINV % P for c in pt)
    assert X * Y % P == T * Z % P, "X Y != T Z"
    zi = O.inv(Z)
    return (X * zi % P, Y * zi % P)


def check_point(pt, exp, note):
    assert all(value_of(c) < 2 * P and normalised(c) for c in pt), note
    assert affine_of(pt) == exp, note


@pytest.mark.parametrize("masks", MASK_SETS, ids=("wide", "narrow"))
def test_point_ops(masks):
    cat = C.catalogue(masks)
    for p, q, (pa, qa, note) in cat["pt_add"]:
        assert affine_of(p) == pa and affine_of(q) == qa
        check_point(F.pt_add(p, q, masks), O.aff_add(pa, qa), note)
    for p, (pa, _, note) in cat["pt_dbl"]:
        check_point(F.pt_dbl(p, masks), O.aff_add(pa, pa), note)
    for p, rec, ng, (pa, qa, note) in cat["pt_madd"]:
        q = (rec[1], rec[0], F.kt_neg_if(rec[2], True)) if ng else rec
        check_point(F.pt_madd(p, q, masks), O.aff_add(pa, O.aff_neg(qa) if ng else qa), (note, ng))
    assert sorted(cat["pt_add_quad"]) == [1, 15, 16, 17, 65]
    for cnt, pairs in cat["pt_add_quad"].items():
        assert len(pairs) == cnt
        for p, q, (pa, qa, note) in pairs:
            check_point(F.pt_add_quad(p, q, masks), O.aff_add(pa, qa), note)
    notes = {n for _, _, n in cat["pairs"]}
    assert {"P + P", "P + (-P)", "identity + Q", "order 2 + Q", "order 4 + Q"} <= notes
    assert O.aff_add(C.ORDER2, C.ORDER2) == O.IDENTITY and O.aff_add(C.ORDER4[0], C.ORDER4[0]) == C.ORDER2


@pytest.mark.parametrize("masks", MASK_SETS, ids=("wide", "narrow"))
def test_records(masks):
    h = pow(2, -1, P)
    for fmt, rc in C.catalogue(masks)["records"].items():
        records = []
        for words, (x, y) in zip(rc["inputs"], rc["affine"]):
            rec, err = F.prepare_record(words, fmt, masks)
            assert err == 0
            ymx, ypx = rec[0:NL], rec[F.PRE_HALF:F.PRE_HALF + NL]
            kt = rec[F.PRE_KT:F.PRE_KT + NL - 1] + [rec[NL]]
            for got, exp in ((ymx, (y - x) * h), (ypx, (y + x) * h), (kt, O.EDWARDS_D * x * y)):
                assert value_of(got) * RINV % P == exp % P and normalised(got), (fmt, x, y)
            assert value_of(kt) < 2 * P and value_of(ypx) < 4 * P and value_of(ymx) < 10 * P
            # the duplicated top limbs and the padding (msm_dev.h PRE_WORDS)
            assert rec[F.PRE_HALF + NL] == kt[NL - 1] and rec[NL + 1] == ypx[NL - 1] and rec[F.PRE_HALF + NL + 1] == ymx[NL - 1]
            assert rec[11] == rec[23] == 0 and len(rec) == F.PRE_WORDS
            records.append(rec)
        assert any(w[-8:] != [0] * 7 + [1] for w in rc["inputs"]) or fmt == F.PT_FMT_XY  # z != 1 inputs
        for ent, acc, (acc_aff, q_aff, sgn) in zip(rc["entries"], rc["accs"], rc["notes"]):
            q = F.load_pre_signed(records, ent)
            check_point(F.pt_madd(acc, q, masks), O.aff_add(acc_aff, O.aff_neg(q_aff) if sgn else q_aff), (fmt, ent))


def test_record_errors():
    bad_x = F.be_words(P) + F.be_words(1)
    assert F.prepare_record(bad_x, F.PT_FMT_XY)[1] == F.ERR_COORD_RANGE
    z0 = F.be_words(0) + F.be_words(1) + F.be_words(0)
    assert F.prepare_record(z0, F.PT_FMT_XYZ)[1] == F.ERR_BAD_POINT
