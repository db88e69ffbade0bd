"""Narrow scalars on a prepared-bases handle through the JS drop-in (webgpu-msm_amd/js/submission.mjs)
on the GPU: compute_msm_prepared(handle, scalars, { scalarBits: 64 }) against the oracle on the
zero-extended scalars, for a flat Uint32Array and for bigints, alone and beside `first` and `indices`,
and the rejection of a bigint that does not fit."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import msm_amd as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "webgpu-msm_amd", "js", "submission.mjs")
NODE = shutil.which("node")
BITS = 64


def _oracle(pts, vals):
    return O.msm(np.ascontiguousarray(pts), M.scalars_to_wire(vals), window=10, threads=4)


@pytest.mark.skipif(NODE is None, reason="node not installed")
@pytest.mark.parametrize("levels", [0, 2])
def test_prepared_bases_narrow_scalars_js(levels, tmp_path):
    n, m, first = 257, 100, 157
    pts = O.gen_points(n, k0=21, step=13)
    rnd = random.Random(64)
    full = [rnd.getrandbits(BITS) for _ in range(n)]
    full[:4] = [0, 1, (1 << BITS) - 1, 1 << (BITS - 1)]
    sub = [rnd.getrandbits(BITS) for _ in range(m)]
    sub[0] = (1 << BITS) - 1
    idx = [int(v) for v in np.random.RandomState(3).randint(0, n, size=m)]
    idx[0], idx[1], idx[2] = n - 1, 0, n - 1
    exp_full = _oracle(pts, full)
    exp_range = _oracle(pts[first:first + m], sub)
    exp_prefix = _oracle(pts[:m], sub)
    exp_index = _oracle(pts[idx], sub)
    wide = O.xorshift_scalars(n, seed=77)
    exp_wide = _oracle(pts, wide)
    rows = [[O.be_words_to_int(pts[i, 8 * j: 8 * j + 8]) for j in range(4)] for i in range(n)]
    data = json.dumps({"pts": [[str(v) for v in r] for r in rows], "full": [str(s) for s in full],
                       "sub": [str(s) for s in sub], "wide": [str(s) for s in wide], "idx": idx})
    script = f"""
import * as m from {json.dumps(JS)};
const d = {data};
const points = d.pts.map(([x, y, t, z]) => ({{x: BigInt(x), y: BigInt(y), t: BigInt(t), z: BigInt(z)}}));
const full = d.full.map(BigInt), sub = d.sub.map(BigInt), wide = d.wide.map(BigInt);
const idx = Uint32Array.from(d.idx);
const flat = (v) => {{   // two big-endian words per 64-bit scalar
  const a = new Uint32Array(2 * v.length);
  v.forEach((s, i) => {{ a[2 * i] = Number(s >> 32n); a[2 * i + 1] = Number(s & 0xffffffffn); }});
  return a;
}};
const show = (r) => r.x.toString() + "," + r.y.toString();
const outcome = async (f) => {{ try {{ await f(); return "resolved"; }} catch (e) {{ return "rejected:" + (e.code !== undefined ? e.code : e.name); }} }};
(async () => {{
  const h = m.prepare_bases(points, {{ levels: {levels} }});
  const b = {BITS};
  const r = [];
  r.push(show(await m.compute_msm_prepared(h, flat(full), {{ scalarBits: b }})));
  r.push(show(await m.compute_msm_prepared(h, full, {{ scalarBits: b }})));
  r.push(show(await m.compute_msm_prepared(h, flat(sub), {{ scalarBits: b, first: {first} }})));
  r.push(show(await m.compute_msm_prepared(h, sub, {{ scalarBits: b, first: {first} }})));
  r.push(show(await m.compute_msm_prepared(h, sub, {{ scalarBits: b }})));                 // the prefix
  r.push(show(await m.compute_msm_prepared(h, flat(sub), {{ scalarBits: b, indices: idx }})));
  r.push(show(await m.compute_msm_prepared(h, wide)));                                     // the plain call, as before
  const big = full.slice(); big[{n} - 1] = 1n << 64n;
  r.push(await outcome(() => m.compute_msm_prepared(h, big, {{ scalarBits: b }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, full, {{ scalarBits: 0 }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, full, {{ scalarBits: 257 }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, flat(sub), {{ scalarBits: b, first: {n - m + 1} }})));
  const hi = flat(full); hi[0] = 2;                                                        // bit 33 of a 33-bit scalar
  r.push(await outcome(() => m.compute_msm_prepared(h, hi, {{ scalarBits: 33 }})));
  r.push(show(await m.compute_msm_prepared(h, full, {{ scalarBits: b }})));
  m.release_bases(h);
  console.log(r.join(";"));
}})().catch((e) => {{ console.error(e); process.exit(3); }});
"""
    path = tmp_path / "run_js_narrow.mjs"
    path.write_text(script)
    out = subprocess.run([NODE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    r = out.stdout.strip().split(";")
    xy = lambda s: tuple(int(v) for v in s.split(","))  # noqa: E731
    assert xy(r[0]) == exp_full and xy(r[1]) == exp_full
    assert xy(r[2]) == exp_range and xy(r[3]) == exp_range
    assert xy(r[4]) == exp_prefix and xy(r[5]) == exp_index
    assert xy(r[6]) == exp_wide
    assert r[7] == "rejected:RangeError"          # a bigint >= 2^64 never reaches the library
    assert r[8].startswith("rejected") and r[9].startswith("rejected")
    assert r[10] == "rejected:-1" and r[11] == "rejected:-1"
    assert xy(r[12]) == exp_full
