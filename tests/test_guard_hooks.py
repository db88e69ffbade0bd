"""The guard hooks' parts that need no device (csrc/host_guard.h, msm_test_guard*): the name table
covers every buffer the headers declare, and the switch toggles while nothing is allocated."""
import os
import re

import pytest

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


def test_poison_hooks_are_exported():
    L = M.load()
    for name in ("msm_test_guard_fill", "msm_test_guard_poison", "msm_test_guard_peek"):
        assert getattr(L, name) is not None
    assert callable(M._test_guard_fill) and callable(M._test_guard_poison) and callable(M._test_guard_peek)


def test_fill_word_is_bounded_and_the_previous_one_returned():
    assert M._test_guard_fill(0) == 0  # the default
    try:
        assert M._test_guard_fill(3) == 0
        assert M._test_guard_fill(1) == 3
        for word in (4, 5, 0xA5, 1 << 16, 0x80000000, 0xFFFFFFFF):
            with pytest.raises(M.MsmError) as e:
                M._test_guard_fill(word)
            assert e.value.code == -1, word
            assert M._test_guard_fill(1) == 1, word  # a refused word changes nothing
        assert M._test_guard_fill(2) == 1
    finally:
        M._test_guard_fill(0)
    assert M._test_guard_fill(0) == 0


def test_peek_refuses_what_it_cannot_read():
    """No device context in this process (msm_shutdown): no payload to read, whatever the range."""
    M.load().msm_shutdown()
    names = M._test_guard_names()
    for buffer in (len(names), len(names) + 7, 0xFFFFFFFF):  # past the table
        with pytest.raises(M.MsmError) as e:
            M._test_guard_peek(buffer, 0, 1)
        assert e.value.code == -1, buffer
    for name in ("g_head", "err", "h_out", "shared_pts", "bases_rec", "bases_prep_err"):
        for first, words in ((0, 1), (0, 0), (1 << 40, 4)):
            with pytest.raises(M.MsmError) as e:
                M._test_guard_peek(name, first, words)
            assert e.value.code == -1, (name, first, words)
    with pytest.raises(M.MsmError):
        M._test_guard_peek("g_head", 0, 1, slot=4)
    with pytest.raises(M.MsmError):
        M._test_guard_peek("g_head", 0, 1, slot=-1)
    M._test_guard_poison()  # no context, guard off: nothing to do, and no error


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
