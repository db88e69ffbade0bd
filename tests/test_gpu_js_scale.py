"""Per-point scalar multiples through the JS drop-in (webgpu-msm_amd/js/submission.mjs) on the GPU:
scale_bases_prepared's wire output for bigint and Uint32Array scalars, narrow scalars and an index
list, and { asBases } feeding compute_msm_prepared and release_bases.  Expected values come from
Python: s_i = (A + i B) / k_i mod r on the bases k_i G gives gen_points(n, A, B) word for word."""
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
N, K0, STEP, A, B = 200, 21, 13, 9, 4


def _inputs():
    pts = O.gen_points(N, k0=K0, step=STEP)
    exp = O.gen_points(N, k0=A, step=B)
    ss = [(A + i * B) * pow(K0 + i * STEP, -1, O.R_ORDER) % O.R_ORDER + (i % 3 == 2) * (1 + i % 27) * O.R_ORDER
          for i in range(N)]
    return pts, ss, exp


def _affine(rec):
    return (O.be_words_to_int(rec[:8]), O.be_words_to_int(rec[8:16]))


@pytest.mark.parametrize("case", ["bigint", "u32", "bits64", "indices", "asBases"])
def test_scale_bases_js(case, tmp_path):
    assert NODE is not None, "node is needed for the JS surface"
    pts, ss, exp = _inputs()
    rnd = random.Random(5)
    opts, idx, scalars = {}, None, ss
    if case == "bits64":
        scalars = [rnd.getrandbits(64) for _ in range(N)]
        scalars[0], scalars[1] = (1 << 64) - 1, 0
        exp = O.affine_to_wire([O.c_scalar_mul(_affine(pts[i]), scalars[i]) for i in range(N)])
        opts = {"scalarBits": 64}
    elif case == "indices":
        idx = [rnd.randrange(N) for _ in range(N + 50)]  # repeats, m > n
        scalars = [ss[i] for i in idx]
        exp = exp[idx]
    elif case == "asBases":
        opts = {"asBases": True, "levels": 2}
    msm_sc = O.xorshift_scalars(len(scalars), seed=77)
    exp_msm = O.msm(exp, O.ints_to_be_words(msm_sc), window=10, threads=8)
    data = json.dumps({"pts": [int(v) for v in pts.reshape(-1)], "sc": [str(s) for s in scalars], "idx": idx,
                       "msm": [str(s) for s in msm_sc], "opts": opts})
    script = f"""
import * as m from {json.dumps(JS)};
const d = {data};
const scalars = d.sc.map(BigInt);
const flat = (vals, words) => {{ const a = new Uint32Array(vals.length * words);
  vals.forEach((v, i) => {{ let b = v; for (let k = words - 1; k >= 0; k--) {{ a[words * i + k] = Number(b & 0xffffffffn); b >>= 32n; }} }});
  return a; }};
const opts = d.opts;
if (d.idx) opts.indices = Uint32Array.from(d.idx);
(async () => {{
  const h = m.prepare_bases(Uint32Array.from(d.pts), {{ levels: 1 }});
  let input = scalars;
  if ("{case}" === "u32") input = flat(scalars, 8);
  const out = m.scale_bases_prepared(h, input, opts);
  if (opts.asBases) {{
    const r = await m.compute_msm_prepared(out, d.msm.map(BigInt));
    const rel = m.release_bases(out), again = m.release_bases(out);
    console.log(["handle", out.n, out.levels, r.x.toString(), r.y.toString(), rel, again].join(";"));
  }} else {{
    console.log(["wire", out instanceof Uint32Array, out.length, Array.from(out).join(",")].join(";"));
  }}
  m.release_bases(h);
}})().catch((e) => {{ console.error(e); process.exit(3); }});
"""
    path = tmp_path / "run_js_scale.mjs"
    path.write_text(script)
    out = subprocess.run([NODE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    fields = out.stdout.strip().split(";")
    if case == "asBases":
        kind, hn, hl, x, y, rel, again = fields
        assert (kind, int(hn), int(hl)) == ("handle", N, 2)
        assert (int(x), int(y)) == exp_msm
        assert (int(rel), int(again)) == (0, -1)
    else:
        kind, is_u32, length, words = fields
        assert (kind, is_u32, int(length)) == ("wire", "true", len(scalars) * 32)
        got = np.array([int(v) for v in words.split(",")], dtype=np.uint32).reshape(-1, 32)
        assert np.array_equal(got, exp)
