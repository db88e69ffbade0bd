"""The model of the bucket reduction (tests/_red_model.py) and its catalogue of shapes
(tests/_red_catalogue.py), checked on the CPU, and the reduction's host-side pieces through the
library's own code: the catalogue reaches every named branch class, the model's terms give
sum s_i k_i in both second-stage forms, every condition the model can flip is caught by some shape;
red1_lane / red1_group (msm_test_red_map) are bijections with the live chunks first, red2_term /
red2_term_group (msm_test_red_map_term) cover sum_c (U_c + c T_c) exactly, and collect_terms /
horner_run (msm_test_tail_plan) give the Python oracle's point for every chunk length.  No GPU.
"""
import numpy as np
import pytest

import _acc_catalogue as C
import _red_catalogue as RC
import _red_model as RM
import msm_amd as M
from oracle import oracle as O

SHAPES = RC.shapes()
NAMES = [s.name for s in SHAPES]
AFTER = {"c8_empty_mid": "c8_sweep"}  # the shape that ran before on the same slot (tests/test_gpu_red_state.py)
INVALID = 0xFFFFFFFF
_run = {}


def prev_nonempty(s):
    if s.name not in AFTER:
        return ()
    p = RC.shape(AFTER[s.name])
    return set(np.nonzero(p.sizes.reshape(-1, p.B).sum(axis=1))[0].tolist())


def run(s, flips=(), tree_knob=True):
    key = (s.name, tuple(flips), tree_knob)
    if key not in _run:
        mi = RC.model_inputs(s)
        _run[key] = RM.execute(RC.plan(s, tree_knob), mi["sizes"], mi["weight"], mi["lead"], flips=flips,
                               prev_nonempty=prev_nonempty(s))
    return _run[key]


def test_group_order():
    assert RM.R == O.R_ORDER


def test_plans_are_the_library_s():
    """The chunk length, chunk count and term count the model derives are the ones the library plans:
    L from launch_plan for the knob-free shapes, the rest from msm_test_red_map / msm_test_tail_plan."""
    for s in SHAPES:
        pl = RC.plan(s)
        m = M._test_red_map(s.n, chunk_len=s.L or 0, window_size=s.c)
        assert (m["L"], m["nchunks"], m["ngroups"], m["W"], m["B"]) == (pl.L, pl.nchunks, pl.ngroups, pl.W, pl.B), s.name
        t = M._test_tail_plan(s.n, chunk_len=s.L or 0, window_size=s.c)
        assert (t["nterms"], t["nv"], t["windows"]) == (pl.nterms, pl.nv, pl.W), s.name
    # what a lone MSM plans on the default device shape: L = 8 up to a 16-bit table, 16 above
    for c in range(4, 21):
        L = M.launch_plan(64, window_size=c)["chunk_len"]
        assert L == (8 if C.geometry(c)[2] <= 16 else 16), c


def test_coverage():
    """The union of the shapes' branch classes is the model's whole list, no more and no less.  (pytest -s
    prints the table: class, the shapes that reach it.)"""
    table = {}
    for s in SHAPES:
        for e in run(s).events:
            table.setdefault(e, []).append(s.name)
    for e in RM.EVENTS:
        print("%-34s %s" % (e, ", ".join(table.get(e, ["-"]))))
    assert sorted(table) == sorted(RM.EVENTS), (sorted(set(RM.EVENTS) - set(table)), sorted(set(table) - set(RM.EVENTS)))
    assert len(set(RM.EVENTS)) == len(RM.EVENTS)
    # what needs no knob reaches everything but the classes of a chunk length the default plan never takes
    plain = {e for s in RC.plain() for e in run(s).events}
    assert set(RM.EVENTS) - plain == {"chunk:short_last", "chunk:last_live_straddles_half", "ngroups:odd", "ngroups:64",
                                      "term:vslice_uneven", "term:bit_group_past_end", "L:two_bits"}


def test_shapes_are_small():
    for s in SHAPES:
        assert s.n <= 1024 and int(s.sizes.sum()) <= 4096, s.name
    assert sorted(s.name for s in SHAPES if s.slow) == ["c17_L4", "c17_L8", "c17_groups", "c19_direct"]


@pytest.mark.parametrize("name", NAMES)
def test_totals(name):
    """The model's tail over its terms, in the form the plan takes and in both forms by force, is
    sum_i s_i k_i mod r of the shape's inputs, and so is the plain sum_w 2^off_w sum_b (b + 1) B_{w,b}."""
    s = RC.shape(name)
    want = RC.expected_scalar(s)
    res = run(s)
    assert res.total == want
    assert res.total_direct == want
    if RC.plan(s).tree:
        assert res.total_tree == want
    assert run(s, tree_knob=False).total == want
    assert RM.plain_total(RC.plan(s), RC.model_inputs(s)["weight"]) == want
    # no live chunk sums to the identity: a dropped add could not hide there
    assert all(v != 0 for v in res.U.values()) and all(v != 0 for v in res.T.values())


@pytest.mark.parametrize("name", NAMES)
def test_inputs_match_recipe(name):
    s = RC.shape(name)
    inp = C.inputs(s)
    assert np.array_equal(np.bincount(inp["key"], minlength=s.nkeys), s.sizes)
    assert np.array_equal(C.check_recode(s), s.sizes)
    if name == "c8_overflow":
        assert sum(v >= 1 << 254 for v in inp["ints"]) == 3


def _differs(a, b):
    return [f for f in ("total", "total_direct", "total_tree", "U", "T", "G", "terms_tree", "terms_direct")
            if getattr(a, f) != getattr(b, f)]


@pytest.mark.parametrize("flip", sorted(RM.FLIPS))
def test_condition_sensitivity(flip):
    """With the condition flipped, some shape's total or a named intermediate comes out wrong.  (pytest -s
    prints the first shape that tells, and what changed.)"""
    for s in SHAPES:
        d = _differs(run(s), run(s, flips=(flip,)))
        if d:
            print("%-14s %-14s %s" % (flip, s.name, ", ".join(d)))
            assert "total" in d or "total_direct" in d or set(d) & {"U", "T", "G", "terms_tree", "terms_direct"}
            return
    pytest.fail("no catalogue shape tells %s (%s)" % (flip, RM.FLIPS[flip]))


def test_every_flip_changes_a_total():
    """Stronger than the above for all but the flips that leave a value nobody reads: the final total of
    some shape is wrong."""
    for flip in RM.FLIPS:
        assert any(run(s).total != run(s, flips=(flip,)).total or run(s).total_direct != run(s, flips=(flip,)).total_direct
                   for s in SHAPES), flip


# ---- the lane and group maps, through the kernels' own functions on the host ------------------------
LS = RM.RED1_LS


def _widths(c, scalar_bits=None):
    """(widths of the main windows, table width), as make_plan balances them."""
    T = 254 if scalar_bits is None else max(scalar_bits + 1, 4)
    wn = -(-T // c)
    q, nhi = divmod(T, wn)
    return [q + 1 if w < nhi else q for w in range(wn)], q + 1 if nhi else q


def _check_map(c, nm, L, windows=None, scalar_bits=None):
    main, cw = _widths(c, scalar_bits)
    m = M._test_red_map(100, nm=nm, chunk_len=L, window_size=c, windows=windows, scalar_bits=scalar_bits, extra=300)
    B, nch, G, W, Wr, w0 = m["B"], m["nchunks"], m["ngroups"], m["W"], m["Wr"], m["w0"]
    assert B == 1 << (cw - 1) and nch == -(-B // L) and G == -(-nch // 128) and m["L"] == L
    assert m["Wm"] == len(main) + 1 and W == nm * Wr
    if windows:
        assert (w0, Wr) == (windows[0], windows[1] - windows[0])
    elif scalar_bits is not None:
        assert (w0, Wr) == (0, len(main))
    else:
        assert (w0, Wr) == (0, len(main) + 1)
    # the buckets a canonical digit of window w0 + l can reach: none in the overflow window
    reach = np.array([(1 << (main[w0 + l] - 1)) if w0 + l < len(main) else 0 for l in range(Wr)], dtype=np.int64)
    lanes = m["lanes"].astype(np.int64)
    total = W * nch
    assert np.all(lanes[total:] == INVALID), "a lane past the end maps to a chunk"
    w, ch = lanes[:total, 0], lanes[:total, 1]
    assert w.max() < W and ch.max() < nch
    assert np.all(np.bincount(w * nch + ch, minlength=total) == 1), "not a bijection"
    live = ch * L < reach[w % Wr]
    assert np.all(np.diff(live.astype(np.int8)) <= 0), "a live chunk after a dead one"
    # every MSM's live chunks in one stretch, MSM by MSM
    nlive = int(live.sum())
    assert np.all(np.diff(w[:nlive] // Wr) >= 0) and np.all(np.diff(w[nlive:] // Wr) >= 0)
    groups = m["groups"].astype(np.int64)
    gt = W * G
    assert np.all(groups[gt:] == INVALID)
    gw, gg, gl = groups[:gt, 0], groups[:gt, 1], groups[:gt, 2]
    assert gw.max() < W and gg.max() < G
    assert np.all(np.bincount(gw * G + gg, minlength=gt) == 1)
    glive = gg * 128 * L < reach[gw % Wr]
    assert np.array_equal(glive, gl == 1)
    assert np.all(np.diff(glive.astype(np.int8)) <= 0)
    return m


@pytest.mark.parametrize("c", range(4, 21))
def test_lane_map_full_range(c):
    """Every (window, chunk) of every MSM exactly once, live chunks before dead ones, lanes past the end
    invalid; the same for k_bucket_reduce_1g's groups.  Every width, MSM count and chunk length."""
    for nm in (1, 2, 4, 8):
        for L in LS:
            _check_map(c, nm, L)


@pytest.mark.parametrize("c", range(4, 21))
def test_lane_map_window_ranges(c):
    main, cw = _widths(c)
    wm = len(main)
    nfull = sum(1 for x in main if x == cw)
    ranges = {"w0 > 0": (2, min(5, wm + 1)), "overflow window alone": (wm, wm + 1), "full-width windows alone": (0, min(2, nfull)),
              "narrow windows and the overflow": (wm - 1, wm + 1)}
    for why, r in ranges.items():
        for nm in (1, 2, 4, 8):
            for L in LS:
                m = _check_map(c, nm, L, windows=r)
                if why == "overflow window alone":  # live == 0: every lane is a dead one
                    assert np.array_equal(m["lanes"][:nm * m["nchunks"], 0], np.repeat(np.arange(nm), m["nchunks"]))
                if why == "full-width windows alone":  # dead == 0
                    assert m["Wr"] * m["nchunks"] * nm == len(m["lanes"]) - 300


@pytest.mark.parametrize("bits", [13, 64, 100, 128])
def test_lane_map_narrow_geometry(bits):
    for c in (8, 12, 13, 16, 17):
        for nm in (1, 2, 4, 8):
            for L in LS:
                _check_map(c, nm, L, scalar_bits=bits)


# ---- k_red2_terms' term map ------------------------------------------------------------------------
def _term_coefficients(nv, ngroups, cbits):
    """The coefficient every group point gets in sum_t weight_t term_t, weight 1 for a V slice and 2^k for
    bit term k (in units of L), from the library's own enumeration."""
    coef = np.zeros((ngroups, RM.RG_OUT), dtype=np.int64)
    for t in range(nv + cbits):
        d = M._test_red_map_term(nv, ngroups, t)
        wt = 1 if t < nv else 1 << (t - nv)
        assert d["idx"] == (0 if t < nv else 2 + t - nv if t - nv < RM.RG_LOG else 1)
        assert d["npts"] <= RM.RG_MAXG, "more points than k_red2_terms has quads"
        for g in d["groups"]:
            if g < ngroups:  # (k_red2_terms skips the others)
                coef[g, d["idx"]] += wt
    return coef


def _check_terms(nv, ngroups, cbits):
    coef = _term_coefficients(nv, ngroups, cbits)
    g = np.arange(ngroups)
    # sum_c (U_c + c T_c) = sum_g (V_g + 128 g S_g + sum_k 2^k R_{g,k}); R_{g,k} is zero for 2^k >= nchunks
    assert np.all(coef[:, 0] == 1), (nv, ngroups, coef[:, 0])
    assert np.array_equal(coef[:, 1], RM.RG_CH * g), (nv, ngroups, coef[:, 1])
    for k in range(RM.RG_LOG):
        assert np.all(coef[:, 2 + k] == ((1 << k) if k < cbits else 0)), (nv, ngroups, k)


def test_term_map_covers_every_group_point():
    for ngroups in range(1, 65):
        cbits = RM.RG_LOG + (ngroups - 1).bit_length()
        for nv in (1, 2):
            _check_terms(nv, ngroups, cbits)
    for nchunks in list(range(1, 301)) + [1 << k for k in range(9, 14)] + [342, 8191]:
        pl = RM.Plan([8, 3], 8 * nchunks, 8, 8)
        assert pl.nchunks == nchunks
        _check_terms(pl.nv, pl.ngroups, pl.cbits)


# ---- the host tail's value -------------------------------------------------------------------------
def _host_mont_words(v):
    m = v * (1 << 256) % O.P
    return [(m >> (32 * q)) & 0xFFFFFFFF for q in range(8)]


_pool = []


def pool():
    """64 points t G with their multipliers: computed once, shared."""
    if not _pool:
        rng = np.random.default_rng(97)
        for _ in range(64):
            t = int(rng.integers(1, 1 << 62))
            _pool.append((t, O.scalar_mul(O.G, t)))
    return _pool


@pytest.mark.parametrize("L", LS)
def test_tail_value(L):
    """collect_terms / horner_run on random terms t G (some identities, random Z), for every chunk length,
    four widths, the full range and a sub-range, 0, 1 and 3 helpers:
    ((sum_w 2^off_w (sum_v t_v + L sum_k 2^k t_k)) mod r) G by the Python oracle."""
    rng = np.random.default_rng(1000 + L)
    for c in (8, 13, 16, 17):
        main, _ = _widths(c)
        widths = main + [3]
        off = [sum(widths[:w]) for w in range(len(widths))]
        for windows in (None, (2, 6)):
            info = M._test_tail_plan(64, chunk_len=L, window_size=c, windows=windows)
            Wr, nterms, nv, w0 = info["windows"], info["nterms"], info["nv"], info["w0"]
            assert info["L"] == L and (w0, Wr) == ((0, len(widths)) if windows is None else (2, 4))
            terms = np.zeros((Wr * nterms, 32), np.uint32)
            want = 0
            for l in range(Wr):
                for t in range(nterms):
                    i = l * nterms + t
                    z = int(rng.integers(1, 1 << 62))
                    if rng.random() < 0.2:
                        mult, (x, y) = 0, O.IDENTITY
                    else:
                        mult, (x, y) = pool()[int(rng.integers(0, 64))]
                    for j, v in enumerate((x * z % O.P, y * z % O.P, x * y % O.P * z % O.P, z)):
                        terms[i, 8 * j: 8 * j + 8] = _host_mont_words(v)
                    want += (mult if t < nv else L * mult << (t - nv)) << off[w0 + l]
            exp = O.scalar_mul(O.G, want % O.R_ORDER)
            for helpers in (0, 1, 3):
                assert M._test_tail_plan(64, terms, helpers, chunk_len=L, window_size=c, windows=windows) == exp, \
                    (L, c, windows, helpers)


def test_hook_argument_rules():
    with pytest.raises(M.MsmError):
        M._test_red_map(64, chunk_len=11, window_size=8)
    with pytest.raises(M.MsmError):
        M._test_tail_plan(64, chunk_len=7, window_size=8)
    with pytest.raises(M.MsmError):
        M._test_red_map(64, nm=0, window_size=8)
