"""Native integer scalars on a prepared-bases handle through the JS drop-in
(webgpu-msm_amd/js/submission.mjs) on the GPU: compute_msm_prepared(handle, typedArray, { scalarType })
for an Int8Array, a Uint8Array bitmap and a BigInt64Array, each alone and beside `first` and `indices`,
against the oracle on the magnitudes over points negated by hand where the value is negative, and the
rejection of a typed array of another class."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "webgpu-msm_amd", "js", "submission.mjs")
NODE = shutil.which("node")


def _negate(pts):
    neg = pts.copy()
    for i in range(len(pts)):
        for j in (0, 2):  # x -> -x mod p, t -> -t mod p
            v = O.be_words_to_int(pts[i, 8 * j: 8 * j + 8])
            neg[i, 8 * j: 8 * j + 8] = O.int_to_be_words((O.P - v) % O.P)
    return neg


def _oracle(pts, neg, vals):
    sel = np.array([v < 0 for v in vals], dtype=bool)
    p = np.ascontiguousarray(np.where(sel[:, None], neg, pts))
    return O.msm(p, O.ints_to_be_words([abs(v) for v in vals]), window=10, threads=4)


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_prepared_bases_native_scalars_js(tmp_path):
    n, m, first = 257, 100, 157
    pts = O.gen_points(n, k0=21, step=13)
    neg = _negate(pts)
    rnd = random.Random(65)
    idx = [int(v) for v in np.random.RandomState(4).randint(0, n, size=m)]
    idx[0], idx[1], idx[2] = n - 1, 0, n - 1
    cases, exp = {}, {}
    for ty, lo, hi in (("i8", -128, 127), ("bit", 0, 1), ("i64", -(1 << 63), (1 << 63) - 1)):
        full = [rnd.randint(lo, hi) for _ in range(n)]
        full[:4] = [0, 1, hi, lo]
        sub = [rnd.randint(lo, hi) for _ in range(m)]
        sub[0] = lo
        cases[ty] = {"full": [str(v) for v in full], "sub": [str(v) for v in sub]}
        exp[ty] = (_oracle(pts, neg, full), _oracle(pts[first:first + m], neg[first:first + m], sub),
                   _oracle(pts[idx], neg[idx], sub))
    rows = [[O.be_words_to_int(pts[i, 8 * j: 8 * j + 8]) for j in range(4)] for i in range(n)]
    data = json.dumps({"pts": [[str(v) for v in r] for r in rows], "cases": cases, "idx": idx})
    script = f"""
import * as m from {json.dumps(JS)};
const d = {data};
const points = d.pts.map(([x, y, t, z]) => ({{x: BigInt(x), y: BigInt(y), t: BigInt(t), z: BigInt(z)}}));
const idx = Uint32Array.from(d.idx);
const pack = {{
  i8: (v) => Int8Array.from(v.map(Number)),
  i64: (v) => BigInt64Array.from(v.map(BigInt)),
  bit: (v) => {{   // scalar i is bit i & 7 of byte i >> 3; the pad bits of the last byte are set
    const a = new Uint8Array(Math.ceil(v.length / 8));
    v.forEach((s, i) => {{ a[i >> 3] |= Number(s) << (i & 7); }});
    if (v.length % 8) a[a.length - 1] |= (0xff << (v.length % 8)) & 0xff;
    return a;
  }},
}};
const show = (r) => r.x.toString() + "," + r.y.toString();
const outcome = async (f) => {{ try {{ await f(); return "resolved"; }} catch (e) {{ return "rejected:" + (e.code !== undefined ? e.code : e.name); }} }};
(async () => {{
  const h = m.prepare_bases(points, {{ levels: 0 }});
  const r = [];
  for (const ty of ["i8", "bit", "i64"]) {{
    const full = pack[ty](d.cases[ty].full), sub = pack[ty](d.cases[ty].sub);
    const count = ty === "bit" ? {{ m: {m} }} : {{}};
    r.push(show(await m.compute_msm_prepared(h, full, {{ scalarType: ty, ...(ty === "bit" ? {{ m: {n} }} : {{}}) }})));
    r.push(show(await m.compute_msm_prepared(h, sub, {{ scalarType: ty, first: {first}, ...count }})));
    r.push(show(await m.compute_msm_prepared(h, sub, {{ scalarType: ty, indices: idx }})));
  }}
  const i8 = pack.i8(d.cases.i8.full);
  r.push(await outcome(() => m.compute_msm_prepared(h, new Uint8Array(i8.buffer), {{ scalarType: "i8" }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, i8, {{ scalarType: "bit", m: {n} }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, new Float64Array({n}), {{ scalarType: "i64" }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, i8, {{ scalarType: "i128" }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, i8, {{ scalarType: "i8", scalarBits: 3 }})));  // -128 at b = 3
  r.push(await outcome(() => m.compute_msm_prepared(h, i8, {{ scalarType: "i8", scalarBits: 9 }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, i8, {{ scalarType: "i8", first: 1 }})));        // past the end
  r.push(show(await m.compute_msm_prepared(h, i8, {{ scalarType: "i8", scalarBits: 8 }})));
  m.release_bases(h);
  console.log(r.join(";"));
}})().catch((e) => {{ console.error(e); process.exit(3); }});
"""
    path = tmp_path / "run_js_native.mjs"
    path.write_text(script)
    out = subprocess.run([NODE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    r = out.stdout.strip().split(";")
    xy = lambda s: tuple(int(v) for v in s.split(","))  # noqa: E731
    for k, ty in enumerate(("i8", "bit", "i64")):
        assert tuple(xy(s) for s in r[3 * k: 3 * k + 3]) == exp[ty], ty
    assert r[9:13] == ["rejected:TypeError"] * 4      # a class mismatch never reaches the library
    assert r[13] == "rejected:-1" and r[14] == "rejected:-1" and r[15] == "rejected:-1"
    assert xy(r[16]) == exp["i8"][0]
