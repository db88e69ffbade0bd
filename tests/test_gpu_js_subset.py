"""Subset MSMs on a prepared-bases handle through the JS drop-in (webgpu-msm_amd/js/submission.mjs)
on the GPU: compute_msm_prepared(handle, scalars, { first }) and ({ indices }) against the closed
form, the plain call on the same handle between them, and the out-of-range rejections."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "webgpu-msm_amd", "js", "submission.mjs")
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node not installed")
@pytest.mark.parametrize("levels", [0, 2])
def test_prepared_bases_subsets_js(levels, tmp_path):
    n, m, first, k0, step = 257, 100, 157, 21, 13
    pts = O.gen_points(n, k0=k0, step=step)
    full = O.xorshift_scalars(n, seed=77)
    sub = O.xorshift_scalars(m, seed=78)
    idx = [int(v) for v in np.random.RandomState(3).randint(0, n, size=m)]
    idx[0], idx[1], idx[2] = n - 1, 0, n - 1
    ks = [k0 + step * i for i in range(n)]
    exp_full = O.closed_form_msm(ks, full)
    exp_range = O.closed_form_msm(ks[first:first + m], sub)
    exp_prefix = O.closed_form_msm(ks[:m], sub)
    exp_index = O.closed_form_msm([ks[i] for i in idx], sub)
    rows = [[O.be_words_to_int(pts[i, 8 * j: 8 * j + 8]) for j in range(4)] for i in range(n)]
    data = json.dumps({"pts": [[str(v) for v in r] for r in rows], "full": [str(s) for s in full],
                       "sub": [str(s) for s in sub], "idx": idx})
    script = f"""
import * as m from {json.dumps(JS)};
const d = {data};
const points = d.pts.map(([x, y, t, z]) => ({{x: BigInt(x), y: BigInt(y), t: BigInt(t), z: BigInt(z)}}));
const full = d.full.map(BigInt), sub = d.sub.map(BigInt);
const idx = Uint32Array.from(d.idx);
const show = (r) => r.x.toString() + "," + r.y.toString();
const outcome = async (f) => {{ try {{ await f(); return "resolved"; }} catch (e) {{ return "rejected:" + e.code; }} }};
(async () => {{
  const h = m.prepare_bases(points, {{ levels: {levels} }});
  const a = await m.compute_msm_prepared(h, sub, {{ first: {first} }});
  const b = await m.compute_msm_prepared(h, sub, {{ indices: idx }});
  const c = await m.compute_msm_prepared(h, full);              // the plain call, as before
  const p = await m.compute_msm_prepared(h, sub, {{}});           // the prefix
  const bad = Uint32Array.from(idx); bad[{m} - 1] = {n};
  const e1 = await outcome(() => m.compute_msm_prepared(h, sub, {{ indices: bad }}));
  const e2 = await outcome(() => m.compute_msm_prepared(h, sub, {{ first: {n - m + 1} }}));
  const e3 = await outcome(() => m.compute_msm_prepared(h, sub, {{ first: 1, indices: idx }}));
  const e4 = await outcome(() => m.compute_msm_prepared(h, sub, {{ indices: idx.subarray(1) }}));
  const e5 = await outcome(() => m.compute_msm_prepared(h, sub));   // fewer scalars than points
  const again = await m.compute_msm_prepared(h, sub, {{ indices: idx }});
  m.release_bases(h);
  const e6 = await outcome(() => m.compute_msm_prepared(h, sub, {{ indices: idx }}));
  console.log([show(a), show(b), show(c), show(p), show(again), e1, e2, e3, e4, e5, e6].join(";"));
}})().catch((e) => {{ console.error(e); process.exit(3); }});
"""
    path = tmp_path / "run_js_subset.mjs"
    path.write_text(script)
    out = subprocess.run([NODE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    a, b, c, p, again, e1, e2, e3, e4, e5, e6 = out.stdout.strip().split(";")
    xy = lambda s: tuple(int(v) for v in s.split(","))  # noqa: E731
    assert xy(a) == exp_range and xy(b) == exp_index and xy(c) == exp_full and xy(p) == exp_prefix
    assert xy(again) == exp_index
    assert (e1, e2, e3) == ("rejected:-1",) * 3
    assert e4.startswith("rejected") and e5.startswith("rejected") and e6 == "rejected:-1"
