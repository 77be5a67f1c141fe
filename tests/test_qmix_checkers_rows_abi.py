"""CPU: the C ABI of the Checkers QMIX train-step data side (part of ABI 9, additive) -- cm3_qmix_checkers_rows_f32 declared,
exported, bound; the cm3_qmix_checkers_rows layout as a C compiler sees it; every invalid argument refused with a readable error
before anything touches a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "cm3_qmix_checkers_rows_f32"
FAKE = 0x1000                                      # 16-byte aligned, never dereferenced: validation fails first
FIELDS = ["obs_self_t", "obs_self_v", "obs_others", "actions_prev", "goals", "obs_self_t_f64", "goals_onehot", "q", "argmax",
          "onehot", "q_max", "n_rows"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    return _lib


def test_header_declares_and_library_exports_the_entry(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cm3_amd.h")).read(), flags=re.S)
    handle = built.lib()
    assert re.search(r"\b%s\s*\(" % ENTRY, text)
    assert hasattr(handle, ENTRY)
    assert ENTRY in built.SYMBOLS
    assert built.ABI_VERSION == 9 and handle.cm3_abi_version() == 9
    assert re.search(r"#define\s+CM3_ABI_VERSION\s+9\b", text)


def test_rows_struct_layout_matches_the_header(built, tmp_path):
    """sizeof and every field offset of cm3_qmix_checkers_rows (an anonymous-tag struct), as a C compiler sees include/cm3_amd.h,
    against the ctypes mirror."""
    cls = built.QmixCheckersRows
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cm3_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(cm3_qmix_checkers_rows));']
    for fname, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(cm3_qmix_checkers_rows, %s));' % (fname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert ctypes.sizeof(cls) == got["size"] == 88
    assert [f for f, _ in cls._fields_] == FIELDS
    for fname, _ in cls._fields_:
        assert getattr(cls, fname).offset == got[fname], fname
    text = open(os.path.join(ROOT, "include", "cm3_amd.h")).read()
    assert not re.search(r"typedef struct cm3_qmix_checkers_rows", text)  # (anonymous tag: tests/test_abi.py's table stays as it is)


def _desc(built, **kw):
    d = built.ActorCheckersDesc()
    d.n_envs, d.n_agents, d.stage, d.n_obs = 0, 2, 0, 2                    # n_envs, epsilon, seed, env_id_base, stage, stride: not read
    d.conv_f, d.n_conv_linear, d.n_h1, d.n_h2, d.n_actions = 6, 32, 256, 256, 5
    d.epsilon, d.precision, d.obs_self_t_stride = 7.0, 0, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _weights(built, packed=FAKE):
    w = built.ActorCheckersWeights()
    w.packed = packed
    return w


def _rows(built, **kw):
    r = built.QmixCheckersRows()
    r.obs_self_t, r.obs_self_v, r.obs_others, r.actions_prev, r.goals = FAKE, FAKE, FAKE, FAKE, FAKE
    r.argmax, r.n_rows = FAKE, 100
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _refused(built, needle, desc="default", weights="default", rows="default"):
    handle = built.lib()
    d = _desc(built) if desc == "default" else desc
    w = _weights(built) if weights == "default" else weights
    r = _rows(built) if rows == "default" else rows
    rc = handle.cm3_qmix_checkers_rows_f32(None if d is None else ctypes.byref(d), None if w is None else ctypes.byref(w),
                                           None if r is None else ctypes.byref(r), None)
    assert rc == -1
    assert needle in handle.cm3_last_error(), handle.cm3_last_error()


@pytest.mark.parametrize("field,value,needle", [
    ("n_agents", 0, b"n_agents"), ("n_agents", 9, b"n_agents"), ("n_h1", 128, b"256"), ("conv_f", 8, b"conv_f"),
    ("n_actions", 4, b"5 actions"), ("n_obs", 1, b"n_obs"), ("precision", 1, b"precision"), ("precision", 3, b"precision")])
def test_invalid_descriptor_is_refused_without_a_gpu(built, field, value, needle):
    _refused(built, needle, desc=_desc(built, **{field: value}))


def test_fields_that_are_not_read_do_not_matter(built):
    """n_envs 0, epsilon 7, stage 0 and a zero stride pass the descriptor check: the first complaint is about the rows."""
    _refused(built, b"n_rows", rows=_rows(built, n_rows=0))


def test_null_arguments_are_refused(built):
    _refused(built, b"null desc", desc=None)
    _refused(built, b"null weights", weights=None)
    _refused(built, b"packed", weights=_weights(built, packed=None))
    _refused(built, b"null rows", rows=None)


@pytest.mark.parametrize("name", ["obs_self_t", "obs_self_v", "obs_others", "actions_prev", "goals"])
def test_missing_input_is_refused(built, name):
    _refused(built, b"missing inputs", rows=_rows(built, **{name: None}))


def test_rows_without_an_output_are_refused(built):
    _refused(built, b"no output requested", rows=_rows(built, argmax=None))
    for name in ("q", "onehot", "q_max"):                                  # any single output is enough to pass THIS check
        _refused(built, b"n_rows", rows=_rows(built, argmax=None, n_rows=0, **{name: FAKE}))


@pytest.mark.parametrize("n_rows", [0, -1, 64 * (2 ** 31 - 1) + 1])
def test_row_count_out_of_range_is_refused(built, n_rows):
    _refused(built, b"n_rows", rows=_rows(built, n_rows=n_rows))


@pytest.mark.parametrize("name,value", [("obs_self_t_f64", 2), ("obs_self_t_f64", -1), ("goals_onehot", 2), ("goals_onehot", -1)])
def test_form_flag_other_than_0_or_1_is_refused(built, name, value):
    _refused(built, b"form flags", rows=_rows(built, **{name: value}))


@pytest.mark.parametrize("kw,needle", [
    (dict(obs_self_t=FAKE + 8), b"misaligned inputs"), (dict(obs_self_t=FAKE + 8, obs_self_t_f64=1), b"misaligned inputs"),
    (dict(obs_self_v=FAKE + 8), b"misaligned inputs"), (dict(obs_others=FAKE + 8), b"misaligned inputs"),
    (dict(actions_prev=FAKE + 2), b"misaligned inputs"), (dict(goals=FAKE + 8, goals_onehot=1), b"misaligned inputs"),
    (dict(onehot=FAKE + 8), b"misaligned outputs"), (dict(q=FAKE + 2), b"misaligned outputs"),
    (dict(argmax=FAKE + 2), b"misaligned outputs"), (dict(q_max=FAKE + 2), b"misaligned outputs")])
def test_misaligned_pointer_is_refused(built, kw, needle):
    _refused(built, needle, rows=_rows(built, **kw))


def test_index_goals_need_no_alignment(built):
    """the uint8 index form is read a byte per row: an odd address passes the alignment check (the next complaint is n_rows)"""
    _refused(built, b"n_rows", rows=_rows(built, goals=FAKE + 1, n_rows=0))


@pytest.mark.parametrize("desc_kw,weights,rows_kw,needle", [
    ({"n_obs": 1, "precision": 1}, "default", {}, b"n_obs"),
    ({"precision": 1}, None, {}, b"precision 0 (float32) or 2"),
    ({}, None, None, b"null weights"),
    ({}, "unpacked", None, b"weights->packed is NULL"),
    ({}, "default", None, b"null rows"),
    ({}, "default", {"goals": None, "argmax": None}, b"missing inputs"),
    ({}, "default", {"argmax": None, "n_rows": 0}, b"no output requested"),
    ({}, "default", {"n_rows": 0, "goals_onehot": 2}, b"n_rows must be positive"),
    ({}, "default", {"n_rows": 64 * (2 ** 31 - 1) + 1, "goals_onehot": 2}, b"more than a grid"),
    ({}, "default", {"goals_onehot": 2, "obs_self_v": FAKE + 8}, b"form flags"),
    ({}, "default", {"obs_self_v": FAKE + 8, "argmax": FAKE + 2}, b"misaligned inputs")])
def test_checks_fire_in_their_order(built, desc_kw, weights, rows_kw, needle):
    """Two consecutive checks violated at once: the earlier one's message is the one reported."""
    w = {None: None, "default": _weights(built), "unpacked": _weights(built, packed=None)}[weights]
    _refused(built, needle, desc=_desc(built, **desc_kw), weights=w, rows=None if rows_kw is None else _rows(built, **rows_kw))


def test_soft_update_and_greedy_rows_exist_on_the_agent():
    from cm3_amd.qmix import CheckersQmixAgent
    assert callable(CheckersQmixAgent.greedy_rows) and callable(CheckersQmixAgent.enqueue_rows)
    assert callable(CheckersQmixAgent.soft_update_from)
