"""The control-flow model of the accumulation's joins (tests/_acc_model.py) and its catalogue of shapes
(tests/_acc_catalogue.py), checked on the CPU: the catalogue reaches every named branch class, the
model's symbolic joins give every bucket's plain sum, every condition the model can flip is caught by
some shape, and no piece of any shape's real inputs sums to the identity.  No GPU.
"""
import numpy as np
import pytest

import _acc_catalogue as C
import _acc_model as A
from oracle import oracle as O

SHAPES = C.shapes()
NAMES = [s.name for s in SHAPES]
_lay = {}


def layout(s):
    if s.name not in _lay:
        _lay[s.name] = s.layout(C.chunk_len(s))
    return _lay[s.name]


def coverage():
    """{event: the catalogue shapes that reach it, in catalogue order}."""
    table = {}
    for s in SHAPES:
        for e in A.execute(layout(s)).events:
            table.setdefault(e, []).append(s.name)
    return table


def test_group_order():
    assert A.R == O.R_ORDER


def test_coverage():
    """The union of the shapes' events is the model's whole list, no more and no less.  (pytest -s prints
    the table: event, the shapes that reach it.)"""
    table = coverage()
    for e in A.EVENTS:
        print("%-36s %s" % (e, ", ".join(table.get(e, ["-"]))))
    assert sorted(table) == sorted(A.EVENTS), (sorted(set(A.EVENTS) - set(table)), sorted(set(table) - set(A.EVENTS)))
    assert len(set(A.EVENTS)) == len(A.EVENTS)


def test_shapes_are_small():
    """One to a few workgroups at K in {1, 3, 4} and a few thousand entries; the three tile shapes are the
    only large ones, at K = 1 and at most 2^18 + 2^12 entries."""
    for s in SHAPES:
        lay = layout(s)
        assert s.K in (1, 3, 4)
        if s.large:
            assert s.K == 1 and lay.M <= (1 << 18) + (1 << 12)
        else:
            assert lay.M <= 3072 and lay.nwg <= 10, s.name
    assert sum(s.large for s in SHAPES) == 3
    assert len({s.c for s in SHAPES}) >= 3 and len({layout(s).L for s in SHAPES}) >= 2


@pytest.mark.parametrize("name", NAMES)
def test_totals_catalogue(name):
    s = C.shape(name)
    lay = layout(s)
    rng = np.random.default_rng(len(name) * 7919 + lay.M)
    w = rng.integers(1, 1 << 62, size=lay.M).tolist()
    res = A.execute(lay, w)
    assert res.totals == A.plain_totals(lay, w)
    assert res.second_pass == bool(res.skewed)


def random_layout(rng):
    K = int(rng.choice([1, 2, 3, 4, 5, 8]))
    budget = int(rng.integers(1, 4 * A.ACC_THREADS * K + 1))  # at most 4 workgroups
    p_empty = float(rng.choice([0.0, 0.2, 0.7, 0.95]))
    big = float(rng.choice([0.0, 0.02, 0.2]))  # buckets far past 5 K: long chains, open leads
    sizes, total = [], 0
    while total < budget:
        if rng.random() < p_empty:
            sizes.extend([0] * int(rng.integers(1, 20)))
            continue
        sz = int(rng.integers(0, 5 * K + 1))
        if rng.random() < big:
            sz = int(rng.integers(5 * K, 300 * K + 1))
        sz = min(sz, budget - total)
        sizes.append(sz)
        total += sz
    sizes.extend([0] * int(rng.integers(0, 12)))
    return A.Layout(sizes, K, B=8, L=8)


def test_totals_random_layouts():
    rng = np.random.default_rng(20250101)
    seen = set()
    for i in range(300):
        lay = random_layout(rng)
        w = rng.integers(1, 1 << 62, size=lay.M).tolist()
        res = A.execute(lay, w)
        assert res.totals == A.plain_totals(lay, w), (i, lay.K, lay.sizes.tolist())
        assert res.events <= set(A.EVENTS), (i, res.events - set(A.EVENTS))
        seen |= res.events
    assert len(seen) > len(A.EVENTS) // 2  # the sweep is no substitute for the catalogue, but it is not idle


@pytest.mark.parametrize("flip", sorted(A.FLIPS))
def test_condition_sensitivity(flip):
    """With the condition flipped, some catalogue shape's symbolic totals come out wrong (small shapes
    first; a large one only where no small one can tell)."""
    for s in sorted(SHAPES, key=lambda s: layout(s).M):
        lay = layout(s)
        w = np.random.default_rng(lay.M).integers(1, 1 << 62, size=lay.M).tolist()
        if A.execute(lay, w, flips=[flip]).totals != A.plain_totals(lay, w):
            return
    pytest.fail("no catalogue shape tells %s (%s)" % (flip, A.FLIPS[flip]))


@pytest.mark.parametrize("name", NAMES)
def test_no_hidden_piece(name):
    """Every piece of the shape's real inputs -- a run's part of a bucket, a head, a tail, a walk, a partial
    chain, a lead_val, a bucket's total -- has a signed sum of multipliers that is nonzero mod r: a dropped
    add could not hide behind the identity."""
    s = C.shape(name)
    lay = layout(s)
    inp = C.inputs(s)
    zero = []

    def piece(what, v):
        if v % A.R == 0:
            zero.append(what)

    res = A.execute(lay, inp["weight"].tolist(), pieces=piece)
    assert not zero, zero[:10]
    # ... and in whatever order the device's sort leaves a bucket's entries: a bucket has one sign, and its
    # multipliers sum to less than r
    negs = np.bincount(inp["key"], weights=inp["word"] & 1, minlength=s.nkeys).astype(np.int64)
    assert np.all((negs == 0) | (negs == s.sizes))
    assert int(np.abs(inp["weight"]).sum()) < A.R
    assert all(v != 0 for v in res.totals.values())
    assert res.totals == A.plain_totals(lay, inp["weight"].tolist())


@pytest.mark.parametrize("name", NAMES)
def test_inputs_match_recipe(name):
    """The scalars recode (tests/_narrow_model.py) to exactly the recipe's entries, key by key, and the
    entry list is sorted by key with one word per entry."""
    s = C.shape(name)
    inp = C.inputs(s)
    assert inp["scalars"].shape == (s.n, 8) and inp["n"] == s.n
    assert np.array_equal(np.bincount(inp["key"], minlength=s.nkeys), s.sizes)
    assert np.all(np.diff(inp["key"]) >= 0)
    if s.large:
        idx = np.unique(np.concatenate([np.arange(600), np.random.default_rng(3).integers(0, s.n, 400),
                                        np.arange(s.n - 600, s.n)])).tolist()
        got = C.check_recode(s, idx)
        want = np.bincount(inp["key"][np.isin(inp["word"] >> 1, idx)], minlength=s.nkeys)
        assert np.array_equal(got, want)
    else:
        assert np.array_equal(C.check_recode(s), s.sizes)


def test_both_signs_are_used():
    neg = {s.name: int((C.inputs(s)["word"] & 1).sum()) for s in SHAPES}
    assert sum(1 for v in neg.values() if v) >= len(SHAPES) - 2, neg  # (a shape in one window has no negative digit)
    for s in SHAPES:
        assert int((C.inputs(s)["word"] & 1).sum()) < len(C.inputs(s)["word"])

