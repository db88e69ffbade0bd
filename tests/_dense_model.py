"""The dense-bucket accumulation's plan (host_plan.h dense_launch / dense_entries) and its segment
map (k_dense_segments) restated in plain Python, for tests/test_dense_plan.py and
tests/test_gpu_dense.py."""
import numpy as np

from _narrow_model import auto_width, geometry

DENSE_MIN = 128           # entries per bucket of the widest window from which a narrow launch is dense
DENSE_MAX_KEYS = 1 << 13  # keys (W * B) above which a launch takes the existing path
DENSE_K = 4096            # a dense plan's run length
ROUND_WAVES = 4 * 4 * 256  # the default device shape: 4 waves per SIMD, 4 SIMDs, 256 CUs


def pipelined_window(n, best):
    """The width of an 8-word launch of a pipelined run (host_plan.h pipelined_window)."""
    if n >= 7 << 16:
        return 16
    if n >= 1 << 17:
        return 15
    if n >= 1 << 15:
        return 14
    return best


def unit_bound(m_max, nkeys, E):
    return m_max // (64 * E) + nkeys


def entries_per_lane(m_max, nkeys, round_waves=ROUND_WAVES):
    """The smallest multiple of 4 in 4..64 whose grid bound is one round of resident waves; past one
    round at E = 64, the smallest of that many whole rounds."""
    rounds = max(1, -(-unit_bound(m_max, nkeys, 64) // round_waves))
    for E in range(4, 64, 4):
        if unit_bound(m_max, nkeys, E) <= rounds * round_waves:
            return E
    return 64


def dense_plan(n, nm, b, c, c0):
    """{dense, E, nkeys, units} of a launch of nm narrow MSMs of n b-bit scalars at width c (0: the
    auto width from the size's usual width c0)."""
    if b >= 254:
        return None  # the 8-word launch: never dense
    widths = geometry(b, c or auto_width(n, b, c0))
    cw = max(widths)
    W = nm * len(widths)
    nkeys = W << (cw - 1)
    if n >> (cw - 1) < DENSE_MIN or nkeys > DENSE_MAX_KEYS:
        return {"dense": 0, "E": 0, "nkeys": nkeys, "units": 0}
    E = entries_per_lane(W * n, nkeys)
    return {"dense": 1, "E": E, "nkeys": nkeys, "units": unit_bound(W * n, nkeys, E)}


def segment_map(sizes, S):
    """seg_base [nkeys + 1] and unit_key [live units] of buckets of the given sizes."""
    segs = -(-np.asarray(sizes, dtype=np.int64) // S)
    seg_base = np.concatenate([[0], np.cumsum(segs)])
    return seg_base, np.repeat(np.arange(len(sizes)), segs)


def size_vectors(nkeys, m, S, seed=0):
    """Bucket-size vectors of nkeys keys holding at most m entries: everything in one key (the first,
    the last), one entry per key, alternating empty keys, segment-edge sizes, and random ones."""
    rnd = np.random.RandomState(1000 + seed)
    out = []
    for k in (0, nkeys - 1):
        v = np.zeros(nkeys, np.int64)
        v[k] = m
        out.append(v)
    out.append((np.arange(nkeys) < m).astype(np.int64))  # one entry per key (as far as m goes)
    v = np.zeros(nkeys, np.int64)
    v[::2] = m // max(1, (nkeys + 1) // 2)
    out.append(v)
    out.append(v[::-1].copy())
    edge = np.array([S - 1, S, S + 1, 0, 1, 2 * S, 2 * S + 1, 63, 64, 65], np.int64)
    v = np.resize(edge, nkeys)
    v[np.cumsum(v) > m] = 0  # as many keys as m fills
    out.append(v)
    for _ in range(3):
        p = rnd.dirichlet(np.full(nkeys, 0.3))
        out.append(rnd.multinomial(int(rnd.randint(0, m + 1)), p).astype(np.int64))
    out.append(np.zeros(nkeys, np.int64))
    return out
