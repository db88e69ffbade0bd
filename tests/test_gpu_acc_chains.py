"""The run accumulation's bucket joins on the device, shape by shape (tests/_acc_catalogue.py) against
the control-flow model (tests/_acc_model.py): k_accumulate / acc_tile, k_chain_join, k_lead_scan and
the cross_key / lead_val add of the bucket reduction.  Run on an MI355X: pytest -m gpu.

Every shape runs through compute_msm_device with an explicit window_size and run_length; the result is
compared with the closed form, the slot's workspace is read back (msm_test_acc_state) and compared with
the model -- bucket_start, run_key, the sorted entries bucket by bucket, the skewed workgroups, the
second pass, cross_key, lead_open -- and the bucket table itself with (sum +-k_i) G from the Python
oracle, a crossing bucket after adding lead_val[g0 + 1].  Integer work: every comparison is bit-exact.
The model says which branch an input takes; it is never the reference for a value.
"""
import functools

import numpy as np
import pytest

import _acc_catalogue as C
import _acc_model as A
import msm_amd as M
from _closed_form import as_xy, closed_form
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SMALL = [s.name for s in C.shapes() if not s.large]
LARGE = [s.name for s in C.shapes() if s.large]
INVALID = 0xFFFFFFFF


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def _all_points():
    pts = M.gen_points(max(s.n for s in C.shapes()), k0=C.K0, step=C.STEP)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _dpts(n):
    return _dev(_all_points()[:n])


@functools.lru_cache(maxsize=None)
def _case(name):
    """The shape's inputs, layout, model walk and expected MSM: computed once, shared, never changed."""
    s = C.shape(name)
    inp = C.inputs(s)
    lay = s.layout(C.chunk_len(s))
    return s, inp, lay, A.execute(lay), closed_form(C.K0, C.STEP, inp["scalars"])


def _bucket_point(inp, lay, key):
    a, b = int(lay.bucket_start[key]), int(lay.bucket_start[key + 1])
    return O.scalar_mul(O.G, int(inp["weight"][a:b].sum()) % O.R_ORDER)


def _check_state(name, keys):
    """Read the slot back and compare it with the model; the bucket table for `keys`."""
    s, inp, lay, res, _ = _case(name)
    cross = {k: (int(lay.bucket_start[k]) // lay.K) // A.ACC_THREADS + 1 for k in res.crossing}
    keys = sorted(set(keys) | set(cross))
    st = M._test_acc_state(keys, sorted(set(cross.values())))
    assert (st["M"], st["K"], st["nkeys"], st["runs"], st["workgroups"], st["c"]) == \
        (lay.M, s.K, s.nkeys, lay.nruns, lay.nwg, s.cw), name
    assert np.array_equal(st["bucket_start"], lay.bucket_start), name
    assert np.array_equal(st["run_key"], lay.run_key), name
    # the sorted list holds, bucket by bucket, the wanted (record << 1) | sign words in some order
    key_of = np.repeat(np.arange(s.nkeys), lay.sizes)
    got = st["sorted_entry"][np.lexsort((st["sorted_entry"], key_of))]
    assert np.array_equal(got, inp["word"]), name
    assert st["skewed"] == res.skewed, name
    assert st["second_pass"] == res.second_pass, name
    want_cross = np.array([INVALID if k is None else k for k in res.cross_key], dtype=np.uint32)
    assert np.array_equal(st["cross_key"], want_cross), name
    assert st["lead_open"].tolist() == res.lead_open, name
    for k in keys:
        got = st["buckets"][k]
        if k in cross:
            got = O.aff_add(got, st["lead_val"][cross[k]])
        assert got == _bucket_point(inp, lay, k), (name, k, k in cross)
    return st


def _run_device(name):
    s, inp, _, _, exp = _case(name)
    got = M.compute_msm_device(_dpts(s.n), _dev(inp["scalars"]), s.n, window_size=s.c, run_length=s.K)
    assert got == exp, name


def _every_key(name):
    return np.nonzero(_case(name)[0].sizes)[0].tolist()


@pytest.mark.parametrize("name", SMALL)
def test_small_shapes(name):
    _run_device(name)
    st = _check_state(name, _every_key(name))
    # no piece of the launch summed to the identity, in the order the device's sort left the entries in
    s, _, lay, _, _ = _case(name)
    w = (C.K0 + (st["sorted_entry"].astype(np.int64) >> 1) * C.STEP) * (1 - 2 * (st["sorted_entry"].astype(np.int64) & 1))
    zero = []
    A.execute(lay, w.tolist(), pieces=lambda what, v: zero.append(what) if v == 0 else None)
    assert not zero, (name, zero[:5])


@pytest.mark.parametrize("name", LARGE)
def test_large_shapes(name):
    """One launch each: every crossing bucket and a fixed sample of 64 others."""
    _run_device(name)
    keys = _every_key(name)
    sample = np.random.default_rng(64).choice(len(keys), size=64, replace=False)
    _check_state(name, [keys[i] for i in sample] + keys[:2] + keys[-2:])


def test_wire_entry():
    s, inp, _, _, exp = _case("edges_k1")
    assert M.compute_msm_wire(_all_points()[:s.n], inp["scalars"], window_size=s.c, run_length=s.K) == exp
    _check_state("edges_k1", _every_key("edges_k1"))


def test_bases_handle_full_width():
    s, inp, _, _, exp = _case("wholewg_k1")
    with M.Bases.from_wire(_all_points()[:s.n], levels=1, window_size=s.c) as h:
        assert h.compute(inp["scalars"], window_size=s.c, run_length=s.K) == exp


SEQ = ("seq_a", "seq_b", "seq_c", "seq_a")


def test_one_slot_skewed_unskewed_skewed():
    """One plan, one slot: the captured graph is replayed with the previous launch's skew list, leads and
    staged heads still in the workspace.  The unskewed launch reports no skewed workgroup, the third its
    own and nothing of the first's, and every read-back is the launch's own."""
    plans = {(C.shape(n).n, C.shape(n).c, C.shape(n).K) for n in SEQ}
    assert len(plans) == 1
    assert _case("seq_a")[3].skewed and not _case("seq_b")[3].skewed and _case("seq_c")[3].skewed
    assert not set(_case("seq_a")[3].skewed) & set(_case("seq_c")[3].skewed)
    for name in SEQ:
        _run_device(name)
        _check_state(name, _every_key(name))


def test_many_device_members_share_a_launch():
    """The same three as members of one compute_msm_many_device call: the plan puts them into one launch,
    so the sorted lists follow one another and a tile of 256 runs spans the end of one member and the start
    of the next."""
    names = SEQ[:3]
    n = C.shape(names[0]).n
    s = C.shape(names[0])
    assert n <= 1 << 18  # (pipeline_batch: up to four MSMs of this size share a launch)
    assert all(_case(nm)[2].nruns % A.ACC_THREADS for nm in names[:2])
    out = M.compute_msm_many_device([_dpts(n)] * 3, [_dev(_case(nm)[1]["scalars"]) for nm in names], n,
                                    window_size=s.c, run_length=s.K)
    assert [as_xy(r) for r in out] == [_case(nm)[4] for nm in names]


def test_guard_bands():
    """A skewed and a straddle shape with every workspace buffer between guard bands, allocated at
    exactly the launch's own size: nothing outside a payload is touched, and the skew flags end cleared."""
    L = M.load()
    try:
        L.msm_shutdown()
        M._test_guard(True)
        for name in ("edges_k1", "unskewed_k1"):
            s, inp, _, _, exp = _case(name)
            d_sc = _dev(inp["scalars"])
            M._test_guard_release()  # (as test_gpu_guard.py's checked: every buffer at this call's own size)
            assert M.compute_msm_device(_dpts(s.n), d_sc, s.n, window_size=s.c, run_length=s.K) == exp, name
            assert M._test_guard_check() == [], name
            _check_state(name, _every_key(name)[:16])
    finally:
        L.msm_shutdown()
        M._test_guard(False)
