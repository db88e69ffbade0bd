"""The bucket reduction on the device, shape by shape (tests/_red_catalogue.py) against the model
(tests/_red_model.py) and the Python oracle: k_bucket_reduce_1, k_red2_groups, k_red2_terms and
k_bucket_reduce_2 as a lone MSM's plan takes them.  Run on an MI355X: pytest -m gpu.

Every shape that needs no knob runs through compute_msm_device; the result is compared with the closed
form and the slot's red_U, red_T, red_G and window terms are read back (msm_test_red_state) and
compared with (weight mod r) G (tests/_red_check.py).  The knob-gated paths and chunk lengths run in
tests/test_gpu_red_knobs.py.  Every comparison is bit-exact.
"""
import pytest

import _red_catalogue as RC
import _red_check as K
import msm_amd as M

pytestmark = pytest.mark.gpu

PLAIN = [s.name for s in RC.plain()]


@pytest.mark.parametrize("name", PLAIN)
def test_shapes(name):
    st = K.run_and_check(name)
    s, pl, _, _ = K.case(name)
    # the plan's own chunk length on this device: 8 up to a 16-bit table, 16 above; k_bucket_reduce_2 by size at c = 19
    assert st["L"] == (8 if s.cw <= 16 else 16)
    assert st["path"] == ("reduce_2" if name == "c19_direct" else "groups+terms")
    assert not st["pairs"]


def test_empty_windows_after_populated_ones():
    """c8_empty_mid right after c8_sweep on the same slot: k_red2_groups returns early on windows 1 to 4 and
    leaves the sweep's group points in red_G; the terms of those windows must be identities all the same."""
    K.run_and_check("c8_sweep")
    st = K.run_and_check("c8_empty_mid", "c8_sweep")
    assert {1, 2, 3, 4} <= st["empty"]
    _, pl, res, _ = K.case("c8_empty_mid", "c8_sweep")
    assert "window:empty_after_populated" in res.events
    assert all(st["terms"][(w, t)] == (0, 1) for w in (1, 2, 3, 4) for t in range(pl.nterms))


def test_one_slot_small_wide_small():
    """A 128-bucket table, then 65,536 buckets per window, then the small one again on the same slot: the
    second small launch reads nothing of the wide one's chunk sums or group points."""
    for name in ("c8_sweep", "c17_groups", "c8_sweep", "c12_edges"):
        K.run_and_check(name)


def test_guard_bands():
    """A multi-group shape with every workspace buffer between guard bands, allocated at exactly the
    launch's own size: the reduction touches nothing outside red_U, red_T and red_G."""
    L = M.load()
    try:
        L.msm_shutdown()
        M._test_guard(True)
        for name in ("c13_groups", "c8_overflow"):
            M._test_guard_release()
            K.run_device(name)
            assert M._test_guard_check() == [], name
            K.check_state(name)
    finally:
        L.msm_shutdown()
        M._test_guard(False)


def test_dense_plan_is_read_like_any_other():
    """A dense-bucket launch (8-bit scalars at width 4 on a bases handle: three 3-bit windows of four
    buckets, one chunk each) leaves the same red_U, red_T, red_G and terms behind: msm_test_red_state needs
    nothing of the accumulation."""
    import numpy as np

    import _acc_catalogue as C
    from _narrow_model import recode

    n = 4096
    assert M._test_dense_plan(n, 1, False, 8, 4)["dense"] == 1
    rng = np.random.default_rng(8)
    vals = [int(v) for v in rng.integers(0, 256, size=n)]
    weight = [[0] * 4 for _ in range(3)]
    for i, v in enumerate(vals):
        digits, carry = recode(v, [3, 3, 3])
        assert carry == 0
        for w, d in enumerate(digits):
            if d:
                weight[w][abs(d) - 1] += (C.K0 + i * C.STEP) * (1 if d > 0 else -1)
    total = sum(v * (C.K0 + i * C.STEP) for i, v in enumerate(vals))
    with M.Bases.from_wire(M.gen_points(n, k0=C.K0, step=C.STEP), levels=1) as h:
        assert h.compute(M.scalars_to_wire(vals, scalar_bits=8), window_size=4, scalar_bits=8) == K.point(total % K.RM.R)
        st = M._test_red_state([(w, 0) for w in range(3)], [(w, 0, i) for w in range(3) for i in range(K.RM.RG_OUT)],
                               [(w, 0) for w in range(3)])
    assert (st["L"], st["nchunks"], st["ngroups"], st["nv"], st["nterms"], st["W"], st["B"]) == (8, 1, 1, 1, 1, 3, 4)
    assert st["path"] == "groups+terms" and not st["empty"]
    for w in range(3):
        U = sum((b + 1) * weight[w][b] for b in range(4)) % K.RM.R
        T = sum(weight[w]) % K.RM.R
        assert st["U"][(w, 0)] == K.point(U) and st["T"][(w, 0)] == K.point(T), w
        assert [st["G"][(w, 0, i)] for i in range(K.RM.RG_OUT)] == [K.point(U), K.point(T)] + [(0, 1)] * K.RM.RG_LOG, w
        assert st["terms"][(w, 0)] == K.point(U), w
