"""Compressed points through the JS drop-in (webgpu-msm_amd/js/submission.mjs) on the GPU:
prepare_bases(xs, {form}) + compute_msm_prepared against the closed form, decompress_points feeding
compute_msm, and a bad x rejecting with the library's code."""
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
@pytest.mark.parametrize("form,inputs,levels", [("x", "bigint", 0), ("x", "flat", 2), ("x_ysign", "bigint", 2),
                                                ("x_ysign", "flat", 1)])
def test_compressed_bases_js(form, inputs, levels, tmp_path):
    n = 2048
    pts = O.gen_points(n, k0=21, step=13)
    ss = O.xorshift_scalars(n, seed=77)
    exp = O.closed_form_msm([21 + 13 * i for i in range(n)], ss)
    xy = [(O.be_words_to_int(pts[i, :8]), O.be_words_to_int(pts[i, 8:16])) for i in range(n)]
    signs = [y > O.P - y for _, y in xy]
    nonres = next(x for x in range(1, 200) if O.sqrt_mod((O.P - x * x - 1) * O.inv(O.EDWARDS_D * x * x - 1)) is None)
    data = json.dumps({"xs": [str(x) for x, _ in xy], "signs": signs, "sc": [str(s) for s in ss],
                       "wire": [int(v) for v in pts[:3].reshape(-1)], "bad": str(nonres), "p": str(O.P)})
    script = f"""
import * as m from {json.dumps(JS)};
const d = {data};
const toWords = (v) => {{ const w = new Uint32Array(8); let b = BigInt(v);
  for (let i = 7; i >= 0; i--) {{ w[i] = Number(b & 0xffffffffn); b >>= 32n; }} return w; }};
const form = "{form}", ysign = form === "x_ysign";
let xs = d.xs.map(BigInt), opts = {{ form, levels: {levels} }};
const flat = (vals, signs) => {{ const a = new Uint32Array(vals.length * 8);
  vals.forEach((v, i) => {{ a.set(toWords(v), 8 * i); if (signs && signs[i]) a[8 * i] = (a[8 * i] | 0x80000000) >>> 0; }});
  return a; }};
let input = xs;
if ("{inputs}" === "flat") input = flat(xs, ysign ? d.signs : null);
else if (ysign) opts.signs = d.signs;
const scalars = d.sc.map(BigInt);
const show = (r) => r.x.toString() + "," + r.y.toString();
const codeOf = (f) => {{ try {{ f(); return "ok"; }} catch (e) {{ return String(e.code); }} }};
(async () => {{
  const h = m.prepare_bases(input, opts);
  const a = await m.compute_msm_prepared(h, scalars);
  m.release_bases(h);
  const wire = m.decompress_points(input, opts);
  const head = Array.from(wire.subarray(0, 96)).join(",") === d.wire.join(",");
  const b = await m.compute_msm(wire, flat(scalars));
  const badXs = xs.slice(0, 100); badXs[64] = BigInt(d.bad);
  const badOpts = {{ form, signs: ysign ? d.signs.slice(0, 100) : undefined }};
  const bad = codeOf(() => m.prepare_bases(badXs, badOpts));
  const bad2 = codeOf(() => m.decompress_points(badXs, badOpts));
  badXs[3] = BigInt(d.p);
  const range = codeOf(() => m.prepare_bases(badXs, badOpts));
  const good = m.prepare_bases(xs.slice(0, 100), badOpts);  // and a good creation after them
  console.log([show(a), show(b), h.n, h.levels, wire.length, head, bad, bad2, range, good.n].join(";"));
  m.release_bases(good);
}})().catch((e) => {{ console.error(e); process.exit(3); }});
"""
    path = tmp_path / "run_js_compressed.mjs"
    path.write_text(script)
    out = subprocess.run([NODE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    a, b, hn, hl, wl, head, bad, bad2, rng, good = out.stdout.strip().split(";")
    as_xy = lambda s: tuple(int(v) for v in s.split(","))  # noqa: E731
    assert as_xy(a) == exp and as_xy(b) == exp
    assert (int(hn), int(hl), int(wl), head) == (n, levels or 1, n * 32, "true")
    assert (bad, bad2, rng, int(good)) == ("-4", "-4", "-3", 100)
