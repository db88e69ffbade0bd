"""The bucket reduction's knob-gated paths and chunk lengths on the device: k_bucket_reduce_1 / _1p / _1g
at every instantiated chunk length, k_red2_terms at exactly 64 groups, k_bucket_reduce_2 by knob and by
size.  Run on an MI355X: pytest -m gpu.

Every knob is read once per process, so each setting runs in a child process of its own, one at a time
(as tests/test_gpu_knobs.py does it): the small knob-free shapes of tests/_red_catalogue.py plus the
shapes that need that setting, each with the state comparison of tests/_red_check.py.  A child that ends
on a signal or at its time limit fails the test with the child's stderr; nothing is retried.
"""
import json
import os
import subprocess
import sys

import pytest

import _red_catalogue as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys
sys.path[:0] = [{root!r}, {root!r} + "/webgpu-msm_amd", {root!r} + "/tests"]
import _red_check as K
out = []
for name in {names!r}:
    st = K.run_and_check(name)
    out.append([name, st["L"], st["ngroups"], st["path"], st["pairs"]])
print(json.dumps(out))
"""

SETTINGS = [
    {"MSM_RED_L": "4"},         # the shortest chain; c = 17: 128 groups, k_bucket_reduce_2 by size
    {"MSM_RED_L": "8"},         # c = 17: exactly 64 groups
    {"MSM_RED_L": "9"},
    {"MSM_RED_L": "10"},        # c = 14: seven groups
    {"MSM_RED_L": "12"},        # c = 13: three groups, a partial last group
    {"MSM_RED_L": "17"},
    {"MSM_RED_L": "20"},
    {"MSM_RED2_TREE": "0"},     # k_bucket_reduce_2 at every size
    {"MSM_RED1_PAIRS": "1"},    # the first stage on lane pairs
    {"MSM_RED_FOLD": "1"},      # first stage and group trees in one launch: no red_U / red_T
]
# Seconds a child may take: measured 2.4 to 2.7 s each on an MI355X (the interpreter's and the library's
# start, ten small shapes, and for MSM_RED_L = 4 and 8 a 65,536-bucket table); the limit leaves room
# for a cold start on a busy machine.
TIMEOUT = 60


def _names(env):
    return [s.name for s in RC.small() + RC.for_env(env)]


def test_every_knob_shape_has_a_setting():
    ran = {n for env in SETTINGS for n in _names(env)}
    assert ran == {s.name for s in RC.shapes() if not (s.slow and not s.env)}


@pytest.mark.parametrize("env", SETTINGS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_knob_children(env):
    names = _names(env)
    e = dict(os.environ)
    e.update(env)
    try:
        r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, names=names)], env=e, capture_output=True,
                           text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired as t:
        pytest.fail("%s: the child ran past %d s\n%s" % (env, TIMEOUT, (t.stderr or "")[-2000:]))
    assert r.returncode == 0, (env, r.returncode, r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert [o[0] for o in out] == names
    L = int(env.get("MSM_RED_L", 0))
    for name, got_L, ngroups, path, pairs in out:
        s = RC.shape(name)
        if L:
            assert got_L == L, (name, got_L)
        want = "reduce_2" if (env.get("MSM_RED2_TREE") == "0" or ngroups > 64) else \
            "fold" if env.get("MSM_RED_FOLD") == "1" else "groups+terms"
        assert path == want, (name, path, want)
        assert pairs == (env.get("MSM_RED1_PAIRS") == "1"), name
        if s.env:
            assert got_L == s.L
    if L == 8:
        assert ("c17_L8", 8, 64, "groups+terms", False) in [tuple(o) for o in out]
    if L == 4:
        assert ("c17_L4", 4, 128, "reduce_2", False) in [tuple(o) for o in out]
    if L == 12:
        assert ("c13_L12", 12, 3, "groups+terms", False) in [tuple(o) for o in out]
