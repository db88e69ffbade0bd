"""The guard hooks' parts that need no device (csrc/host_guard.h, msm_test_guard*): the name table
covers every buffer the headers declare, and the switch toggles while nothing is allocated."""
import os
import re

import msm_amd as M

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "webgpu-msm_amd", "csrc")


def _declared_bufs(header, struct):
    """The names declared as `Buf a, b;` inside `struct <struct> { ... }` of a csrc header."""
    with open(os.path.join(CSRC, header)) as f:
        src = f.read()
    body = src[src.index(f"struct {struct} {{"):]
    body = body[:body.index("\n};")]
    names = []
    for decl in re.findall(r"^  Buf ([^;]+);", body, flags=re.M):
        names += [n.strip() for n in decl.split(",")]
    return names


def test_every_declared_buffer_is_in_the_name_table():
    names = M._test_guard_names()
    assert len(names) == len(set(names))
    ws = [n for n in _declared_bufs("host_ctx.h", "Workspace") if not n.startswith("dummy_")]  # tuning builds only
    assert len(ws) >= 30 and names[:len(ws)] == ws  # each_buf passes them in declaration order
    assert names[len(ws)] == "h_out"
    ctx = _declared_bufs("host_ctx.h", "DevCtx")
    assert ctx == ["shared_pts", "host_sc", "host_pts"] and names[len(ws) + 1:len(ws) + 4] == ctx
    assert _declared_bufs("host_bases.h", "Bases") == ["rec"]
    assert names[len(ws) + 4:] == ["bases_rec", "bases_prep_err"]
    assert M.load().msm_test_guard_name(len(names)) is None


def test_switch_toggles_while_nothing_is_allocated():
    M.load().msm_shutdown()
    assert M._test_guard(False) is False
    try:
        assert M._test_guard(True) is False
        assert M._test_guard(True) is True
        assert M._test_guard_check() == []  # no context: nothing to read, and none is created
        M._test_guard_release()
    finally:
        assert M._test_guard(False) is True
    assert M._test_guard(False) is False
