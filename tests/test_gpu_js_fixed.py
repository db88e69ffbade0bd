"""Fixed-base tables through the JS drop-in (webgpu-msm_amd/js/submission.mjs) on the GPU:
prepare_fixed_base and fixed_base_mul on 300 rows for one and two bases, bigint and Uint32Array
scalars, narrow scalars, { asBases } feeding compute_msm_prepared, and a scalar wider than the call's
width refused.  Results are checked against the Python call on the same inputs."""
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
N = 300


@pytest.mark.parametrize("case", ["k1_bigint", "k1_u32", "k2_bigint", "k2_u32", "k2_bits64", "k2_asBases", "k1_refused"])
def test_fixed_base_js(case, tmp_path):
    assert NODE is not None, "node is needed for the JS surface"
    k = int(case[1])
    what = case.split("_")[1]
    pts = M.gen_points(4, k0=21, step=13)
    rnd = random.Random(5 + k)
    bits = 64 if what in ("bits64", "refused") else 256
    scalars = [rnd.getrandbits(bits) for _ in range(N * k)]
    scalars[0], scalars[1] = (1 << bits) - 1, 0
    opts = {"scalarBits": 64} if what == "bits64" else {}
    if what == "asBases":
        opts = {"asBases": True, "levels": 2}
    tab = {"indices": [2, 0]} if k == 2 else {"first": 1, "count": 1}
    with M.Bases.from_wire(pts, levels=1) as b, b.fixed_table(**tab) as t:
        exp = t.mul(O.ints_to_be_words(scalars).reshape(N, k, 8))
    if what == "refused":
        scalars[7] = 1 << 64  # the call says 64 bits
        opts = {"scalarBits": 64}
    msm_sc = O.xorshift_scalars(N, seed=77)
    exp_msm = O.msm(exp, O.ints_to_be_words(msm_sc), window=10, threads=8)
    data = json.dumps({"pts": [int(v) for v in pts.reshape(-1)], "sc": [str(s) for s in scalars], "tab": tab,
                       "msm": [str(s) for s in msm_sc], "opts": opts})
    script = f"""
import * as m from {json.dumps(JS)};
const d = {data};
const scalars = d.sc.map(BigInt);
const flat = (vals, words) => {{ const a = new Uint32Array(vals.length * words);
  vals.forEach((v, i) => {{ let b = v; for (let k = words - 1; k >= 0; k--) {{ a[words * i + k] = Number(b & 0xffffffffn); b >>= 32n; }} }});
  return a; }};
const tab = d.tab;
if (tab.indices) tab.indices = Uint32Array.from(tab.indices);
(async () => {{
  const h = m.prepare_bases(Uint32Array.from(d.pts), {{ levels: 1 }});
  const t = m.prepare_fixed_base(h, tab);
  m.release_bases(h);  // the table keeps its own records
  let input = scalars;
  if ("{what}" === "u32") input = flat(scalars, 8);
  if ("{what}" === "refused") {{
    let threw = [];
    const narrow = flat(scalars.map((v) => v & 0x1ffffffffn), 2);
    narrow[2 * 7] |= 2;  // bit 33 of scalar 7
    for (const [inp, o] of [[scalars, d.opts], [narrow, {{ scalarBits: 33 }}]]) {{
      try {{ m.fixed_base_mul(t, inp, o); threw.push("no"); }} catch (e) {{ threw.push(e.constructor.name + (e.code || "")); }}
    }}
    console.log(["refused", threw.join("|"), t.bases, t.windowBits, t.scalarBits].join(";"));
  }} else {{
    const out = m.fixed_base_mul(t, input, d.opts);
    if (d.opts.asBases) {{
      const r = await m.compute_msm_prepared(out, d.msm.map(BigInt));
      const rel = m.release_bases(out);
      console.log(["handle", out.n, out.levels, r.x.toString(), r.y.toString(), rel].join(";"));
    }} else {{
      console.log(["wire", out instanceof Uint32Array, out.length, Array.from(out).join(",")].join(";"));
    }}
  }}
  console.log(["release", m.release_fixed_base(t), m.release_fixed_base(t)].join(";"));
}})().catch((e) => {{ console.error(e); process.exit(3); }});
"""
    path = tmp_path / "run_js_fixed.mjs"
    path.write_text(script)
    out = subprocess.run([NODE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    first, last = out.stdout.strip().split("\n")
    assert last == "release;0;-1"
    fields = first.split(";")
    if what == "asBases":
        kind, hn, hl, x, y, rel = fields
        assert (kind, int(hn), int(hl), int(rel)) == ("handle", N, 2, 0)
        assert (int(x), int(y)) == exp_msm
    elif what == "refused":
        # a bigint at or above 2^64 is refused when it is packed, a stray bit in narrow words by the library
        kind, threw, bases, wbits, sbits = fields
        assert kind == "refused" and threw == "RangeError|Error-1"
        assert (int(bases), int(wbits), int(sbits)) == (1, 12, 256)
    else:
        kind, is_u32, length, words = fields
        assert (kind, is_u32, int(length)) == ("wire", "true", N * 32)
        got = np.array([int(v) for v in words.split(",")], dtype=np.uint32).reshape(-1, 32)
        assert np.array_equal(got, exp)
