"""Wide native scalars on a prepared-bases handle through the JS drop-in
(webgpu-msm_amd/js/submission.mjs) on the GPU: compute_msm_prepared(handle, typedArray, { scalarType })
for "u128", "i128", "u256" and "fr_mont" on n = 4097, as a BigUint64Array, a Uint32Array and a Uint8Array,
against the oracle on the magnitudes over points negated by hand where the value is negative, and the
rejection of an array of a wrong length or of another class."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import msm_amd as M
from test_gpu_native import _negated, _oracle
from test_gpu_wide import N, TYPES, _entry_case, _expected, _pack, _points, _values

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "webgpu-msm_amd", "js", "submission.mjs")
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_prepared_bases_wide_scalars_js(tmp_path):
    first, m = 1999, 1001
    np.ascontiguousarray(_points(N)).astype("<u4").tofile(tmp_path / "points.bin")
    for ty in TYPES:
        _pack(ty).astype("<u8").tofile(tmp_path / f"{ty}.bin")
    _, _, sub, rng, _, _ = _entry_case("fr_mont")
    sub[0].astype("<u8").tofile(tmp_path / "fr_sub.bin")
    script = f"""
import * as m from {json.dumps(JS)};
import fs from "node:fs";
const load = (name) => {{ const b = fs.readFileSync({json.dumps(str(tmp_path))} + "/" + name); return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength); }};
const show = (r) => r.x.toString() + "," + r.y.toString();
const outcome = async (f) => {{ try {{ await f(); return "resolved"; }} catch (e) {{ return "rejected:" + (e.code !== undefined ? e.code : e.name); }} }};
(async () => {{
  const h = m.prepare_bases(new Uint32Array(load("points.bin")), {{ levels: 1 }});
  const r = [];
  for (const ty of {json.dumps(list(TYPES))}) {{
    const buf = load(ty + ".bin");
    r.push(show(await m.compute_msm_prepared(h, new BigUint64Array(buf), {{ scalarType: ty }})));
    r.push(show(await m.compute_msm_prepared(h, new Uint32Array(buf), {{ scalarType: ty }})));
    r.push(show(await m.compute_msm_prepared(h, new Uint8Array(buf), {{ scalarType: ty }})));
  }}
  const fr = load("fr_mont.bin");
  r.push(show(await m.compute_msm_prepared(h, new BigUint64Array(load("fr_sub.bin")), {{ scalarType: "fr_mont", first: {first} }})));
  r.push(show(await m.compute_msm_prepared(h, new BigUint64Array(fr), {{ scalarType: "fr_mont", scalarBits: 251 }})));
  // one element short (an options object is a subset call: the prefix of as many bases), then what is
  // rejected: a torn element, more elements than bases, another class, another width, a value past the
  // width, an unknown name
  r.push(show(await m.compute_msm_prepared(h, new BigUint64Array(fr, 0, 4 * {N - 1}), {{ scalarType: "fr_mont" }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, new BigUint64Array(fr, 0, 4 * {N} - 1), {{ scalarType: "fr_mont" }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, new Uint8Array(fr, 0, 32 * {N} - 1), {{ scalarType: "u256" }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, new BigUint64Array(fr), {{ scalarType: "u128" }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, new BigInt64Array(fr), {{ scalarType: "fr_mont" }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, new Float64Array(fr), {{ scalarType: "u256" }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, new BigUint64Array(fr), {{ scalarType: "fr_mont", scalarBits: 253 }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, new BigUint64Array(load("u256.bin")), {{ scalarType: "u256", scalarBits: 200 }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, new BigUint64Array(load("u256.bin")), {{ scalarType: "fr_mont" }})));
  r.push(await outcome(() => m.compute_msm_prepared(h, new BigUint64Array(fr), {{ scalarType: "u512" }})));
  r.push(show(await m.compute_msm_prepared(h, new BigUint64Array(fr), {{ scalarType: "fr_mont" }})));
  m.release_bases(h);
  console.log(r.join(";"));
}})().catch((e) => {{ console.error(e); process.exit(3); }});
"""
    path = tmp_path / "run_js_wide.mjs"
    path.write_text(script)
    out = subprocess.run([NODE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    r = out.stdout.strip().split(";")
    xy = lambda s: tuple(int(v) for v in s.split(","))  # noqa: E731
    for k, ty in enumerate(TYPES):
        assert [xy(s) for s in r[3 * k: 3 * k + 3]] == [_expected(ty)] * 3, ty
    assert xy(r[12]) == rng[0] and xy(r[13]) == _expected("fr_mont")
    assert xy(r[14]) == _oracle(_values("fr_mont")[:N - 1], _points(N)[:N - 1], _negated(N)[:N - 1])
    # a torn element (by limbs and by bytes) never reaches the library; 2 n elements are past the handle's bases
    assert r[15:17] == ["rejected:RangeError"] * 2 and r[17] == "rejected:-1"
    assert r[18:20] == ["rejected:TypeError"] * 2  # another class
    assert r[20:23] == ["rejected:-1"] * 3          # the library's own: the width, a magnitude, an a >= r
    assert r[23] == "rejected:TypeError"
    assert xy(r[24]) == _expected("fr_mont")        # the handle stays usable
    assert M.WIDE_TYPES.keys() == TYPES.keys()
