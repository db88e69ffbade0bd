"""One catalogue shape of the bucket reduction (tests/_red_catalogue.py) on the device, compared with
the Python oracle: shared by tests/test_gpu_red_state.py and the knob children of
tests/test_gpu_red_knobs.py.  Needs a GPU.

run_and_check(shape) runs the shape through compute_msm_device with an explicit window_size and
run_length, compares the result with the closed form, reads the slot back (msm_test_red_state) and
compares every U_c and T_c of a chunk with a live bucket, a fixed sample of empty chunks, every group
point of the non-empty windows and every term with (weight mod r) G, the weight from tests/_red_model.py
and the point from the oracle.  Integer work: every comparison is bit-exact.
"""
import functools
import os

import numpy as np

import _acc_catalogue as C
import _red_catalogue as RC
import _red_model as RM
import msm_amd as M
from _closed_form import closed_form
from oracle import oracle as O


def knobs():
    """What this process' environment says about the reduction's path (each knob is read once per process)."""
    e = os.environ
    return {"tree": e.get("MSM_RED2_TREE", "1") != "0", "fold": e.get("MSM_RED_FOLD", "0") == "1",
            "pairs": e.get("MSM_RED1_PAIRS", "0") == "1"}


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def _all_points():
    pts = M.gen_points(max(s.n for s in RC.shapes()), k0=C.K0, step=C.STEP)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _dpts(n):
    return _dev(_all_points()[:n])


@functools.lru_cache(maxsize=None)
def point(v):
    return O.scalar_mul(O.G, v) if v else O.IDENTITY


def prev_windows(prev):
    return set(np.nonzero(prev.sizes.reshape(-1, prev.B).sum(axis=1))[0].tolist()) if prev is not None else ()


@functools.lru_cache(maxsize=None)
def case(name, prev_name=None):
    """The shape's inputs, plan, model run and expected MSM: computed once, shared, never changed."""
    s = RC.shape(name)
    k = knobs()
    pl = RC.plan(s, tree_knob=k["tree"])
    mi = RC.model_inputs(s)
    res = RM.execute(pl, mi["sizes"], mi["weight"], mi["lead"],
                     prev_nonempty=prev_windows(RC.shape(prev_name) if prev_name else None))
    return s, pl, res, closed_form(C.K0, C.STEP, C.inputs(s)["scalars"])


def empty_sample(pl, res):
    """A fixed sample of chunks without a live bucket: the first, middle and last chunk of the first and last
    non-empty window, of the first empty window and of the last window."""
    full = sorted(set(range(pl.W)) - res.empty)
    ws = {full[0], full[-1], pl.W - 1} | ({min(res.empty)} if res.empty else set())
    cs = {0, 1 % pl.nchunks, pl.nchunks // 2, pl.nchunks - 1}
    return sorted((w, c) for w in ws for c in cs if (w, c) not in res.U)


def check_state(name, prev_name=None):
    s, pl, res, _ = case(name, prev_name)
    k = knobs()
    path = "fold" if (k["fold"] and pl.tree) else pl.path
    live = sorted(res.U)
    chunks = [] if path == "fold" else live + empty_sample(pl, res)
    gpts = [] if path == "reduce_2" else [(w, g, i) for (w, g) in sorted(res.G) for i in range(RM.RG_OUT)]
    terms = [(w, t) for w in range(pl.W) for t in range(pl.nterms)]
    st = M._test_red_state(chunks, gpts, terms)
    got = (st["L"], st["nchunks"], st["ngroups"], st["nv"], st["nterms"], st["W"], st["B"], st["c"], st["rg_out"])
    assert got == (pl.L, pl.nchunks, pl.ngroups, pl.nv, pl.nterms, pl.W, pl.B, s.cw, RM.RG_OUT), (name, got)
    assert st["path"] == path, (name, st["path"], path)
    assert st["pairs"] == (k["pairs"] and path != "fold"), name
    assert st["empty"] == res.empty, (name, sorted(st["empty"]), sorted(res.empty))
    for wc in chunks:
        assert st["U"][wc] == point(res.U.get(wc, 0)), (name, "U", wc, wc in res.U)
        assert st["T"][wc] == point(res.T.get(wc, 0)), (name, "T", wc, wc in res.T)
    for w, g, i in gpts:
        assert st["G"][(w, g, i)] == point(res.G[(w, g)][i]), (name, "G", w, g, i)
    for wt in terms:
        assert st["terms"][wt] == point(res.terms[wt]), (name, "term", wt)
    # what the launch did not write is refused, not handed out stale
    if path != "reduce_2" and res.empty:
        _refused(group_points=[(min(res.empty), 0, 0)])
    if path == "reduce_2":
        _refused(group_points=[(0, 0, 0)])
    if path == "fold":
        _refused(chunks=[(0, 0)])
    return st


def _refused(**kw):
    try:
        M._test_red_state(**kw)
    except M.MsmError:
        return
    raise AssertionError("msm_test_red_state handed out %r" % (kw,))


def run_device(name, prev_name=None):
    s, _, _, exp = case(name, prev_name)
    got = M.compute_msm_device(_dpts(s.n), _dev(C.inputs(s)["scalars"]), s.n, window_size=s.c, run_length=s.K)
    assert got == exp, name


def run_and_check(name, prev_name=None):
    run_device(name, prev_name)
    return check_state(name, prev_name)
