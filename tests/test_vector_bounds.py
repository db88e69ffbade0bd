"""Static limb-bound proof of the vector tables' call sites (msm_kernels.hip k_vector_build,
k_vector_eval, k_vector_fold), with the interval model of tests/test_limb_bounds.py, in the manner of
tests/test_combine_bounds.py: what k_vector_eval stores is a legal pt_add operand, the fold closes over
pt_add outputs and the identity, and the Z it leaves for k_fixed_normalise is the form fx_norm_prefix is
proved for.  The kernels' and their helpers' bodies are pinned by digest, so an edit fails here until
the walk below is re-read."""
import re

from test_limb_bounds import (IDENTITY_PT, N_MUL, ONE_B, PT, REC_KT, REC_YMX, REC_YPX, _body, _body_digest, _calls, fe_inv,
                              fe_mul, from_record_bounds, madd_bounds, padd_bounds, pdbl_bounds, stage_affine_bounds,
                              within)


def is_operand(p) -> bool:
    return all(within(c, N_MUL) for c in p.values())


def eval_outputs():
    """What a lane of k_vector_eval stores: the identity (no digit but 0, or a lane past m), or the output
    of a chain of pt_madd -- each coordinate an fe_mul or fe_mul_sd output, which madd_bounds proves to be
    N_MUL for an accumulator of either form and the table's records (k_prepare_points' forms) of either
    sign."""
    madd_bounds(REC_YMX, REC_YPX, REC_KT)
    return IDENTITY_PT, PT


def test_eval_stores_legal_add_operands():
    for p in eval_outputs():
        assert is_operand(p)
        for q in eval_outputs():
            assert is_operand(padd_bounds(p, q))
    # the chain itself: pt_madd takes its own output and the identity (test_limb_bounds.test_madd_bounds)
    assert within(IDENTITY_PT["Y"], N_MUL) and within(IDENTITY_PT["X"], N_MUL)


def test_fold_closes():
    """acc = pt_add(acc, part) from a loaded part on, for up to VX_FOLD parts and any number of passes:
    inputs are k_vector_eval's outputs or an earlier pass's, outputs are pt_add outputs (or, for a lone
    part, the part itself)."""
    forms = list(eval_outputs())
    for _ in range(3):  # three passes cover k = 4096 at G = 1
        new = []
        for acc in forms:
            for part in forms:
                out = acc
                for _ in range(3):  # the form is a fixed point after one addition
                    out = padd_bounds(out, part)
                    assert is_operand(out)
                new.append(out)
        forms = [IDENTITY_PT, PT] + new[:2]
    body = _body("msm_kernels.hip", "k_vector_fold")
    assert body.count("pt_add(") == 1 and "pt_madd" not in body  # the complete addition, and no other
    assert int(re.search(r"VX_FOLD = (\d+);", open(_src_path()).read()).group(1)) == 16


def _src_path():
    import os

    from test_limb_bounds import _CSRC
    return os.path.join(_CSRC, "msm_kernels.hip")


def test_z_for_normalise_is_a_multiply_output():
    """A table of k > 8 bases has at least two parts, so the last pass always adds: the Z it stores is
    pt_add's fe_mul(F, G) (the model returns N_MUL itself), also for the lanes past m, which add two
    identities.  A lone part's Z (the fold of one part, were it ever launched) is a pt_madd output or
    the identity's one.  These are the forms test_remaining_call_sites walks fx_norm_prefix and
    fx_norm_emit with."""
    for p in eval_outputs():
        for q in eval_outputs():
            assert padd_bounds(p, q)["Z"] is N_MUL
    for z in (N_MUL, ONE_B):
        prefix = fe_mul(fe_mul(z, z), z)
        zi = fe_mul(fe_inv(prefix), prefix)
        stage_affine_bounds(fe_mul(N_MUL, zi), fe_mul(N_MUL, zi))


def test_build_is_the_fixed_build_s_ladder():
    """k_vector_build runs k_fixed_build's statements on a rebuilt point: test_limb_bounds.test_ladder_closure's
    call sites."""
    p = from_record_bounds(REC_YMX, REC_YPX)
    for _ in range(3):
        p = pdbl_bounds(p)
        assert is_operand(p)
    for acc in (IDENTITY_PT, PT):
        out = padd_bounds(pdbl_bounds(acc), p)
        assert is_operand(out)
    zi = fe_inv(N_MUL)
    stage_affine_bounds(fe_mul(N_MUL, zi), fe_mul(N_MUL, zi))

    def lane(name):
        body = _body("msm_kernels.hip", name)
        return body[body.index("uint32_t rec[32];"):]

    fixed = lane("k_fixed_build").replace("lane_gather_record(recs, base, true, rec);", "GATHER")
    vector = lane("k_vector_build").replace("lane_gather_record(recs, bases[j], true, rec);", "GATHER")
    assert "GATHER" in fixed and fixed == vector


# the kernels and helpers the walk above mirrors; regenerate a digest with _body_digest("msm_kernels.hip", name)
REVIEWED = {
    ("msm_kernels.hip", "k_vector_build"): "8b6ac2cac75aa133",
    ("msm_kernels.hip", "vx_stage_rows"): "078e80721a2059ad",
    ("msm_kernels.hip", "k_vector_eval"): "1752dd74a17db346",
    ("msm_kernels.hip", "vx_load_point"): "57809f9c18048b4d",
    ("msm_kernels.hip", "k_vector_fold"): "a9c9485f23fb947c",
}


def test_mirrored_sources_unchanged():
    changed = {f"{f}:{n}": _body_digest(f, n) for (f, n), d in REVIEWED.items() if _body_digest(f, n) != d}
    assert not changed, f"the vector kernels changed -- re-check the walk above, then update REVIEWED with: {changed}"


def test_kernels_use_the_shared_pieces():
    """The evaluation is k_fixed_eval's loop over the part's bases; the field code the three kernels run
    is pt_madd, pt_add, pt_dbl, pt_sel, the rebuild and the affine epilogue alone."""
    ev = _body("msm_kernels.hip", "k_vector_eval")
    assert _calls("k_vector_eval", "vx_stage_rows") and _calls("k_vector_eval", "fixed_digit")
    assert _calls("k_vector_eval", "fixed_windows") and _calls("k_vector_eval", "load_pre_signed")
    assert "acc = pt_madd(acc, load_pre_signed(table, cur))" in ev
    assert "MSM_DEV_ERR_SCALAR_RANGE" in ev and "FX_NO_ENTRY" in ev
    for k in ("k_vector_eval", "k_vector_fold"):
        assert not re.search(r"\bfe_(mul|sub|add|neg|inv|sqr)\w*\(", _body("msm_kernels.hip", k)), k
    assert _calls("k_vector_fold", "vx_load_point") and _calls("k_vector_fold", "pt_add")
    for helper in ("pt_from_record", "lane_gather_record", "lane_stage_affine", "fe_inv", "pt_sel", "pt_dbl", "pt_add"):
        assert _calls("k_vector_build", helper), helper
    assert re.search(r"\blane_flush_points<FX_THREADS>\(", _body("msm_kernels.hip", "k_vector_build"))
    # k_fixed_eval's digit bookkeeping, with the part's first base added to the record's base
    fixed = _body("msm_kernels.hip", "k_fixed_eval")
    lam = fixed[fixed.index("auto next_entry"):fixed.index("xyzt acc")]
    mine = ev[ev.index("auto next_entry"):ev.index("xyzt acc")]
    assert mine.replace("((j0 + j) * Wn + win)", "(j * Wn + win)").replace(" ", "") == lam.replace(" ", "")
