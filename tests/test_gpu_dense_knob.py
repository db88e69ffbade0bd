"""MSM_DENSE_MIN, the A/B knob of the dense-bucket accumulation: read once per process, so each
setting runs in a child process of its own over the same narrow calls, bit-exact against the oracle.
1 forces the path onto launches of 16 entries per bucket; a huge value sends the booleans' one
giant bucket down the run-based accumulation, as before the path existed."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [{root!r}, {root!r} + "/webgpu-msm_amd", {root!r} + "/tests"]
import msm_amd as M
from oracle import oracle as O
from test_gpu_subset import _dev, _points

n = 4097
pts = _points(n)
rnd = np.random.RandomState(41)
out = {{"dense": [], "ok": []}}
with M.Bases.from_wire(pts, levels=1) as h:
    for b, c in ((1, 0), (8, 0), (8, 4), (12, 0)):
        sc = rnd.randint(0, 1 << b, size=(n, 1)).astype(np.uint32)
        full = np.zeros((n, 8), np.uint32)
        full[:, 7:] = sc
        exp = O.msm(pts, full, window=10, threads=8)
        out["dense"].append(M._test_dense_plan(n, 1, False, b, c)["dense"])
        out["ok"].append(h.compute(sc, window_size=c or None, scalar_bits=b) == exp
                         and h.compute_device(_dev(sc), window_size=c or None, scalar_bits=b) == exp)
print(json.dumps(out))
"""


@pytest.mark.parametrize("dense_min,dense", [(None, [1, 0, 1, 0]), ("1", [1, 1, 1, 1]), (str(1 << 30), [0, 0, 0, 0])])
def test_knob_moves_the_threshold_and_results_stay_exact(dense_min, dense):
    env = {k: v for k, v in os.environ.items() if k != "MSM_DENSE_MIN"}
    if dense_min is not None:
        env["MSM_DENSE_MIN"] = dense_min
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["dense"] == dense
    assert out["ok"] == [True] * 4
