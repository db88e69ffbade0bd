"""Resident prepared bases through the JS drop-in (webgpu-msm_amd/js/submission.mjs) on the GPU:
prepare_bases + compute_msm_prepared against compute_msm on the same inputs, a second scalar vector
on the same handle, and a use after release_bases."""
import json
import os
import shutil
import subprocess

import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "webgpu-msm_amd", "js", "submission.mjs")
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node not installed")
@pytest.mark.parametrize("form,levels", [("bigint", 0), ("u32", 2), ("flat", 2)])
def test_prepared_bases_js(form, levels, tmp_path):
    n = 4096
    pts = O.gen_points(n, k0=21, step=13)
    ss = [O.xorshift_scalars(n, seed=77), O.xorshift_scalars(n, seed=78)]
    exp = [O.closed_form_msm([21 + 13 * i for i in range(n)], s) for s in ss]
    rows = [[O.be_words_to_int(pts[i, 8 * j: 8 * j + 8]) for j in range(4)] for i in range(n)]
    data = json.dumps({"pts": [[str(v) for v in r] for r in rows], "sc": [[str(s) for s in v] for v in ss]})
    script = f"""
import * as m from {json.dumps(JS)};
const d = {data};
const toWords = (v) => {{ const w = new Uint32Array(8); let b = BigInt(v);
  for (let i = 7; i >= 0; i--) {{ w[i] = Number(b & 0xffffffffn); b >>= 32n; }} return w; }};
let points, scalars;
if ("{form}" === "bigint") {{
  points = d.pts.map(([x, y, t, z]) => ({{x: BigInt(x), y: BigInt(y), t: BigInt(t), z: BigInt(z)}}));
  scalars = d.sc.map((v) => v.map(BigInt));
}} else if ("{form}" === "u32") {{
  points = d.pts.map(([x, y, t, z]) => ({{x: toWords(x), y: toWords(y), t: toWords(t), z: toWords(z)}}));
  scalars = d.sc.map((v) => v.map(toWords));
}} else {{  // flat wire buffers: n x 32 and n x 8 words
  points = new Uint32Array(d.pts.length * 32);
  d.pts.forEach((r, i) => r.forEach((v, j) => points.set(toWords(v), 32 * i + 8 * j)));
  scalars = d.sc.map((vec) => {{ const s = new Uint32Array(vec.length * 8);
    vec.forEach((v, i) => s.set(toWords(v), 8 * i)); return s; }});
}}
const show = (r) => r.x.toString() + "," + r.y.toString();
(async () => {{
  const plain = await m.compute_msm(points, scalars[0]);
  const h = m.prepare_bases(points, {{ levels: {levels} }});
  const a = await m.compute_msm_prepared(h, scalars[0]);
  const b = await m.compute_msm_prepared(h, scalars[1]);   // the handle again, other scalars
  const rel = m.release_bases(h);
  let after = "resolved";
  try {{ await m.compute_msm_prepared(h, scalars[0]); }} catch (e) {{ after = "rejected"; }}
  console.log([show(plain), show(a), show(b), h.n, h.levels, rel, m.release_bases(h), after].join(";"));
}})().catch((e) => {{ console.error(e); process.exit(3); }});
"""
    path = tmp_path / "run_js_bases.mjs"
    path.write_text(script)
    out = subprocess.run([NODE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    plain, a, b, hn, hl, rel, rel2, after = out.stdout.strip().split(";")
    xy = lambda s: tuple(int(v) for v in s.split(","))  # noqa: E731
    assert xy(plain) == exp[0] and xy(a) == exp[0] and xy(b) == exp[1]
    assert (int(hn), int(rel), int(rel2), after) == (n, 0, -1, "rejected")
    assert int(hl) == (levels or 1)
