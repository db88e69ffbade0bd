"""Static limb-bound proof of the combine kernels' call sites (msm_kernels.hip k_combine_sum,
k_combine_one, k_combine_joint), with the interval model of tests/test_limb_bounds.py: every point they
hand to pt_add and pt_dbl has the coordinate forms those functions' proofs take, and the Z they leave
for k_fixed_normalise is the form fx_norm_prefix is proved for.  The kernels' bodies are pinned by
digest, so an edit fails here until the walk below is re-read."""
import re

from test_limb_bounds import (IDENTITY_PT, N_MUL, NL, ONE_B, PT, REC_YMX, REC_YPX, B, _body, _body_digest, _calls,
                              fe_inv, fe_mul, fe_norm, fe_sub_u, from_record_bounds, padd_bounds, pdbl_bounds,
                              stage_affine_bounds, within)
from _fp29_model import P


def fe_neg(b: B) -> B:
    """fp29.cuh fe_neg: K8P - b, normalised (pt_dbl's H is mirrored the same way)."""
    r = fe_norm(fe_sub_u(B([0] * NL, 0), b))
    assert within(r, B.normalised(8 * P))
    return r


def neg_bounds(p):
    """msm_kernels.hip cb_neg_if with neg set: X and T through fe_neg and a multiply by one."""
    return dict(X=fe_mul(fe_neg(p["X"]), ONE_B), Y=p["Y"], T=fe_mul(fe_neg(p["T"]), ONE_B), Z=p["Z"])


def is_operand(p) -> bool:
    return all(within(c, N_MUL) for c in p.values())


def rebuilt_points():
    """What a lane holds after pt_from_record and cb_neg_if: the rebuilt point, with either sign."""
    p = from_record_bounds(REC_YMX, REC_YPX)
    return p, neg_bounds(p)


def test_negated_point_is_a_legal_operand():
    p, n = rebuilt_points()
    assert is_operand(p) and is_operand(n)
    for q in (p, n, PT, IDENTITY_PT):
        assert is_operand(padd_bounds(n, q)) and is_operand(padd_bounds(q, n))
    assert is_operand(pdbl_bounds(n))
    # a ladder output negated (the form is the same: fe_mul outputs in, fe_mul outputs out)
    assert is_operand(neg_bounds(PT)) and is_operand(neg_bounds(IDENTITY_PT))


def test_sum_closes():
    """k_combine_sum: pt_add(A, +-B) on two rebuilt points."""
    p, n = rebuilt_points()
    for b in (p, n):
        assert is_operand(padd_bounds(p, b))


def joint_table():
    """k_combine_joint's table entries: the identity, A, +-B and A +- B (a pt_add output)."""
    p, n = rebuilt_points()
    entries = [IDENTITY_PT, p, n]
    for b in (p, n):
        ab = padd_bounds(p, b)
        assert is_operand(ab), "A + B is not a legal table entry"
        entries.append(ab)
    return entries


def test_joint_step_closes():
    """acc = pt_add(pt_dbl(acc), q) for every table entry q, from the identity and from any earlier step's
    output."""
    for acc0 in (IDENTITY_PT, PT):
        for q in joint_table():
            acc = acc0
            for _ in range(3):
                acc = padd_bounds(pdbl_bounds(acc), q)
                assert is_operand(acc)


def test_one_closes():
    """k_combine_one: k_scale_points' ladder over {O, S, 2S, 3S} for S of either sign, then
    pt_add(acc, plain) with the plain side's rebuilt point of either sign."""
    p, n = rebuilt_points()
    for s in (p, n):
        s2 = pdbl_bounds(s)
        s3 = padd_bounds(s2, s)
        for acc0 in (IDENTITY_PT, PT):
            for q in (IDENTITY_PT, s, s2, s3):
                acc = padd_bounds(pdbl_bounds(pdbl_bounds(acc0)), q)
                assert is_operand(acc)
                for plain in (p, n):
                    assert is_operand(padd_bounds(acc, plain))
    # b = 1 .. 2 with a zero digit, or a dead lane: the accumulator is still the identity
    for plain in (p, n):
        assert is_operand(padd_bounds(IDENTITY_PT, plain))


def test_z_for_normalise_is_a_multiply_output():
    """cb_store_proj stores a pt_add output's Z (fe_mul(F, G): the model returns N_MUL itself) or the
    identity's one for a lane past m -- the two forms test_remaining_call_sites walks fx_norm_prefix and
    fx_norm_emit with."""
    p, n = rebuilt_points()
    outs = [padd_bounds(p, n), padd_bounds(padd_bounds(pdbl_bounds(PT), p), n)]
    outs += [padd_bounds(pdbl_bounds(PT), q) for q in joint_table()]
    for out in outs:
        assert out["Z"] is N_MUL
    for z in (N_MUL, ONE_B):
        prefix = fe_mul(fe_mul(z, z), z)
        zi = fe_mul(fe_inv(prefix), prefix)
        stage_affine_bounds(fe_mul(N_MUL, zi), fe_mul(N_MUL, zi))


# the kernels and helpers the walk above mirrors; regenerate a digest with _body_digest("msm_kernels.hip", name)
REVIEWED = {
    ("msm_kernels.hip", "combine_digit"): "ac73eeb884c7b035",
    ("msm_kernels.hip", "cb_stage_side"): "8a7b42a5782b78e2",
    ("msm_kernels.hip", "cb_read_side"): "fba77dd08dec963e",
    ("msm_kernels.hip", "cb_neg_if"): "f5c0641e959976bf",
    ("msm_kernels.hip", "cb_stage_scalars"): "68328c78791469cc",
    ("msm_kernels.hip", "cb_my_scalar"): "49019339d3f61d64",
    ("msm_kernels.hip", "cb_store_proj"): "2dda687a7880e4ea",
    ("msm_kernels.hip", "k_combine_sum"): "e58f2f6991d9b79e",
    ("msm_kernels.hip", "k_combine_one"): "55d067403a3e6740",
    ("msm_kernels.hip", "k_combine_joint"): "fc411549059e73b3",
}
KERNELS = ("k_combine_sum", "k_combine_one", "k_combine_joint")


def test_mirrored_sources_unchanged():
    changed = {f"{f}:{n}": _body_digest(f, n) for (f, n), d in REVIEWED.items() if _body_digest(f, n) != d}
    assert not changed, f"the combine kernels changed -- re-check the walk above, then update REVIEWED with: {changed}"


def test_kernels_use_the_shared_pieces():
    """Every kernel rebuilds with pt_from_record, reads through the lane frame and stores through
    cb_store_proj; the field code they run is pt_add, pt_dbl, pt_sel and cb_neg_if alone."""
    for k in KERNELS:
        assert _calls(k, "pt_from_record") and _calls(k, "cb_read_side") and _calls(k, "cb_stage_side")
        assert _calls(k, "cb_store_proj") and _calls(k, "cb_neg_if")
        assert not re.search(r"\bfe_(mul|sub|add|neg|inv|sqr)\w*\(", _body("msm_kernels.hip", k)), k
    assert _calls("cb_read_side", "lane_read_record") and _calls("cb_read_side", "lane_gather_record")
    for helper, callee in (("cb_stage_side", "lane_stage_records"), ("cb_stage_scalars", "lane_stage_scalars")):
        assert re.search(r"\b%s<CB_THREADS>\(" % callee, _body("msm_kernels.hip", helper)), helper  # (templates)
    assert _calls("k_combine_one", "scale_digit") and _calls("k_combine_one", "scale_windows")
    assert _calls("k_combine_joint", "combine_digit")
    neg = _body("msm_kernels.hip", "cb_neg_if")
    assert neg.count("fe_mul(fe_neg(") == 2 and len(re.findall(r"\bfe_\w+\(", neg)) == 5  # two of each, and fe_one
