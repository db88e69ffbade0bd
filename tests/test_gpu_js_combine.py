"""Pairwise combinations through the JS drop-in (webgpu-msm_amd/js/submission.mjs) on the GPU:
combine_bases_prepared's wire output for per-point scalars, { sub }, a broadcast scalar and a second
handle, { keep } feeding compute_msm_prepared and release_bases, and one argument error.  Expected values
come from Python: on the bases k_i G, a_i k_i + b_i k_(OFF + i) = A + i B mod r gives gen_points(M, A, B)
word for word."""
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
N, OFF, M, K0, STEP, A, B = 200, 100, 100, 21, 13, 9, 4
R = O.R_ORDER


def _k(i):
    return K0 + i * STEP


def _inputs():
    pts = O.gen_points(N, k0=K0, step=STEP)
    exp = O.gen_points(M, k0=A, step=B)
    rnd = random.Random(9)
    a = [rnd.getrandbits(256) for _ in range(M)]
    b = [(A + i * B - a[i] * _k(i)) * pow(_k(OFF + i), -1, R) % R + (i % 3 == 2) * (1 + i % 27) * R for i in range(M)]
    return pts, a, b, exp


@pytest.mark.parametrize("case", ["records", "sub", "broadcast", "other", "sum", "keep", "error"])
def test_combine_bases_js(case, tmp_path):
    assert NODE is not None, "node is needed for the JS surface"
    pts, a, b, exp = _inputs()
    opts = {"bFirst": OFF}
    sc = {"a": [str(v) for v in a], "b": [str(v) for v in b]}
    bc = {}
    if case == "sub":  # a_i A_i - (r - b_i) B_i: the same points
        sc["b"] = [str((R - v % R) % R) for v in b]
        opts["sub"] = True
    elif case == "broadcast":  # x P_i + y P_(OFF + i), 16-bit x and y: a progression again
        x, y = 0xBEEF, 0x1234
        sc, bc = {}, {"a": str(x), "b": str(y)}
        opts.update(scalarBits=16, m=M)
        exp = O.gen_points(M, k0=x * K0 + y * _k(OFF), step=STEP * (x + y))
    elif case == "other":  # the B_i from a second handle, by index
        opts = {"bIndices": list(range(M))}
    elif case == "sum":  # P_(OFF + i) - P_i = OFF STEP G for every i
        sc = {}
        opts = {"aFirst": OFF, "sub": True, "m": M}
        exp = O.gen_points(M, k0=OFF * STEP, step=0)
    elif case == "keep":
        opts.update(keep=True, levels=2)
    elif case == "error":
        opts["bFirst"] = OFF + 1  # the B range runs past the handle's end
    msm_sc = O.xorshift_scalars(M, seed=77)
    exp_msm = O.msm(exp, O.ints_to_be_words(msm_sc), window=10, threads=8)
    data = json.dumps({"pts": [int(v) for v in pts.reshape(-1)], "sc": sc, "bc": bc, "msm": [str(s) for s in msm_sc],
                       "opts": opts, "off": OFF})
    script = f"""
import * as m from {json.dumps(JS)};
const d = {data};
const opts = d.opts;
for (const k of ["a", "b"]) {{
  if (d.sc[k]) opts[k] = d.sc[k].map(BigInt);
  if (d.bc[k]) opts[k] = BigInt(d.bc[k]);
}}
if (opts.bIndices) opts.bIndices = Uint32Array.from(opts.bIndices);
(async () => {{
  const all = Uint32Array.from(d.pts);
  const h = m.prepare_bases(all, {{ levels: 1 }});
  let h2;
  if ("{case}" === "other") {{
    h2 = m.prepare_bases(all.subarray(32 * d.off), {{ levels: 1 }});
    opts.other = h2;
  }}
  let out;
  try {{
    out = m.combine_bases_prepared(h, opts);
  }} catch (e) {{
    console.log(["threw", e.message].join(";"));
    return;
  }}
  if (opts.keep) {{
    const r = await m.compute_msm_prepared(out, d.msm.map(BigInt));
    const rel = m.release_bases(out), again = m.release_bases(out);
    console.log(["handle", out.n, out.levels, r.x.toString(), r.y.toString(), rel, again].join(";"));
  }} else {{
    console.log(["wire", out instanceof Uint32Array, out.length, Array.from(out).join(",")].join(";"));
  }}
  m.release_bases(h);
  if (h2) m.release_bases(h2);
}})().catch((e) => {{ console.error(e); process.exit(3); }});
"""
    path = tmp_path / "run_js_combine.mjs"
    path.write_text(script)
    out = subprocess.run([NODE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    fields = out.stdout.strip().split(";")
    if case == "error":
        assert fields[0] == "threw" and "invalid" in fields[1].lower(), fields
    elif case == "keep":
        kind, hn, hl, x, y, rel, again = fields
        assert (kind, int(hn), int(hl)) == ("handle", M, 2)
        assert (int(x), int(y)) == exp_msm
        assert (int(rel), int(again)) == (0, -1)
    else:
        kind, is_u32, length, words = fields
        assert (kind, is_u32, int(length)) == ("wire", "true", M * 32)
        got = np.array([int(v) for v in words.split(",")], dtype=np.uint32).reshape(-1, 32)
        assert np.array_equal(got, exp)
