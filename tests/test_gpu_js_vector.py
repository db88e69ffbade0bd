"""Vector tables through the JS drop-in (webgpu-msm_amd/js/submission.mjs) on the GPU:
prepare_vector_base over 12 bases and fixed_base_mul on 100 rows, with Uint32Array and BigInt scalars,
checked word for word against the Python call on the same inputs; the token is released twice."""
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
K, N = 12, 100


def test_vector_base_js(tmp_path):
    assert NODE is not None, "node is needed for the JS surface"
    pts = M.gen_points(16, k0=21, step=13)
    rnd = random.Random(12)
    scalars = [rnd.getrandbits(256) for _ in range(N * K)]
    scalars[0], scalars[1] = (1 << 256) - 1, 0
    tab = {"first": 3, "count": K, "windowBits": 5}
    with M.Bases.from_wire(pts, levels=1) as b, b.vector_table(first=3, count=K, window_bits=5) as t:
        exp = t.mul(O.ints_to_be_words(scalars).reshape(N, K, 8))
        info = t.info
    # the Python call itself against the oracle, on the first rows
    for i in range(3):
        assert O.words_xy(exp[i]) == O.msm(pts[3:3 + K], O.ints_to_be_words(scalars[i * K:(i + 1) * K]), window=4)
    data = json.dumps({"pts": [int(v) for v in pts.reshape(-1)], "sc": [str(s) for s in scalars], "tab": tab})
    script = f"""
import * as m from {json.dumps(JS)};
const d = {data};
const scalars = d.sc.map(BigInt);
const flat = (vals, words) => {{ const a = new Uint32Array(vals.length * words);
  vals.forEach((v, i) => {{ let b = v; for (let k = words - 1; k >= 0; k--) {{ a[words * i + k] = Number(b & 0xffffffffn); b >>= 32n; }} }});
  return a; }};
const h = m.prepare_bases(Uint32Array.from(d.pts), {{ levels: 1 }});
const t = m.prepare_vector_base(h, d.tab);
m.release_bases(h);  // the table keeps its own records
let refused = "no";
try {{ m.prepare_fixed_base(h, d.tab); }} catch (e) {{ refused = e.constructor.name; }}
console.log(["table", t.bases, t.windowBits, t.scalarBits, t.windows, t.records, t.bytes, refused].join(";"));
for (const input of [flat(scalars, 8), scalars]) {{
  const out = m.fixed_base_mul(t, input);
  console.log(["wire", out instanceof Uint32Array, out.length, Array.from(out).join(",")].join(";"));
}}
console.log(["release", m.release_fixed_base(t), m.release_fixed_base(t)].join(";"));
"""
    path = tmp_path / "run_js_vector.mjs"
    path.write_text(script)
    out = subprocess.run([NODE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    table, u32, big, last = out.stdout.strip().split("\n")
    assert last == "release;0;-1"
    fields = table.split(";")
    assert fields[0] == "table" and fields[-1] != "no"  # (prepare_fixed_base: a released handle, and k > 8)
    assert [int(v) for v in fields[1:7]] == [info[n] for n in ("bases", "window_bits", "scalar_bits", "windows", "records",
                                                               "bytes")]
    assert info["bases"] == K
    for line in (u32, big):
        kind, is_u32, length, words = line.split(";")
        assert (kind, is_u32, int(length)) == ("wire", "true", N * 32)
        got = np.array([int(v) for v in words.split(",")], dtype=np.uint32).reshape(-1, 32)
        assert np.array_equal(got, exp)
