"""CPU: the C ABI of the CM3 Checkers actor over transition rows (part of ABI 9, additive) -- cm3_actor_checkers_rows_f32 declared,
exported, bound; the cm3_actor_checkers_rows layout as a C compiler sees it; every invalid argument refused with a readable error
before anything touches a GPU; the Python surface that goes with it."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "cm3_actor_checkers_rows_f32"
FAKE = 0x1000                                      # 16-byte aligned, never dereferenced: validation fails first
FIELDS = ["obs_self_t", "obs_self_v", "obs_others", "actions_prev", "goals", "obs_self_t_f64", "goals_onehot", "probs", "actions",
          "onehot", "epsilon_dev", "n_rows", "row_id_base", "draw", "_pad"]
INPUTS = FIELDS[:5]


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
    """sizeof and every field offset of cm3_actor_checkers_rows (an anonymous-tag struct), as a C compiler sees include/cm3_amd.h,
    against the ctypes mirror."""
    cls = built.ActorCheckersRows
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cm3_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(cm3_actor_checkers_rows));']
    for fname, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(cm3_actor_checkers_rows, %s));' % (fname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert ctypes.sizeof(cls) == got["size"] == 104 and got["size"] % 8 == 0
    assert [f for f, _ in cls._fields_] == FIELDS
    for fname, _ in cls._fields_:
        assert getattr(cls, fname).offset == got[fname], fname
    # the inputs and the two form flags sit where cm3_qmix_checkers_rows has them
    for fname in FIELDS[:7]:
        assert getattr(cls, fname).offset == getattr(built.QmixCheckersRows, fname).offset, fname
    text = open(os.path.join(ROOT, "include", "cm3_amd.h")).read()
    assert not re.search(r"typedef struct cm3_actor_checkers_rows", text)    # (anonymous tag: tests/test_abi.py's table stays as it is)


def _desc(built, **kw):
    d = built.ActorCheckersDesc()
    d.n_envs, d.n_agents, d.stage, d.n_obs = 0, 2, 2, 2                      # n_envs, env_id_base, obs_self_t_stride: not read
    d.conv_f, d.n_conv_linear, d.n_h1, d.n_h2, d.n_actions = 6, 32, 256, 256, 5
    d.epsilon, d.precision, d.seed = 0.25, 0, 12341
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _weights(built, packed=FAKE):
    w = built.ActorCheckersWeights()
    w.packed = packed
    return w


def _rows(built, **kw):
    r = built.ActorCheckersRows()
    for name in INPUTS:
        setattr(r, name, FAKE)
    r.actions, r.n_rows = FAKE, 100
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _refused(built, needle, desc="default", weights="default", rows="default"):
    handle = built.lib()
    d = _desc(built) if desc == "default" else desc
    w = _weights(built) if weights == "default" else weights
    r = _rows(built) if rows == "default" else rows
    ref = lambda x: None if x is None else ctypes.byref(x)              # noqa: E731
    rc = getattr(handle, ENTRY)(ref(d), ref(w), ref(r), None)
    assert rc == -1
    assert needle in handle.cm3_last_error(), handle.cm3_last_error()


@pytest.mark.parametrize("field,value,needle", [
    ("n_agents", 0, b"n_agents"), ("n_agents", 9, b"n_agents"), ("conv_f", 8, b"conv_f 6"), ("n_conv_linear", 64, b"conv_linear 32"),
    ("n_h1", 128, b"h1 256"), ("n_h2", 128, b"h2 256"), ("n_actions", 4, b"5 actions"), ("n_obs", 1, b"n_obs"),
    ("precision", 3, b"precision"), ("precision", -1, b"precision"), ("stage", 0, b"stage"), ("stage", 3, b"stage"),
    ("epsilon", 1.5, b"epsilon"), ("epsilon", -0.1, b"epsilon")])
def test_rows_invalid_descriptor_is_refused_without_a_gpu(built, field, value, needle):
    _refused(built, needle, desc=_desc(built, **{field: value}))


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("stage", [1, 2])
def test_every_precision_and_stage_passes_the_descriptor_checks(built, precision, stage):
    """(the call then stops at the NEXT check: no output requested)"""
    _refused(built, b"no output requested", desc=_desc(built, precision=precision, stage=stage), rows=_rows(built, actions=None))


def test_rows_null_arguments_are_refused(built):
    _refused(built, b"null desc", desc=None)
    _refused(built, b"null weights", weights=None)
    _refused(built, b"null rows", rows=None)


def test_rows_without_packed_weights_are_refused(built):
    _refused(built, b"weights->packed is NULL", weights=_weights(built, packed=None))


@pytest.mark.parametrize("name", INPUTS)
def test_rows_missing_input_is_refused(built, name):
    _refused(built, b"missing inputs", rows=_rows(built, **{name: None}))
    assert name.encode() in built.lib().cm3_last_error()


def test_rows_without_an_output_are_refused(built):
    _refused(built, b"no output requested", rows=_rows(built, actions=None))
    for name in ("probs", "onehot"):                                       # any single output is enough to pass THIS check
        _refused(built, b"n_rows", rows=_rows(built, actions=None, n_rows=0, **{name: FAKE}))


@pytest.mark.parametrize("n_rows", [0, -1, 64 * (2 ** 31 - 1) + 1])
def test_rows_count_out_of_range_is_refused(built, n_rows):
    _refused(built, b"n_rows", rows=_rows(built, n_rows=n_rows))


@pytest.mark.parametrize("name,value", [("obs_self_t_f64", 2), ("obs_self_t_f64", -1), ("goals_onehot", 2), ("goals_onehot", -1)])
def test_rows_form_flag_out_of_range_is_refused(built, name, value):
    _refused(built, b"form flags", rows=_rows(built, **{name: value}))
    assert name.encode() in built.lib().cm3_last_error()


@pytest.mark.parametrize("kw,needle", [
    ({"obs_self_t": FAKE + 8}, b"misaligned inputs"), ({"obs_self_t": FAKE + 8, "obs_self_t_f64": 1}, b"misaligned inputs"),
    ({"obs_self_v": FAKE + 8}, b"misaligned inputs"), ({"obs_others": FAKE + 8}, b"misaligned inputs"),
    ({"actions_prev": FAKE + 2}, b"misaligned inputs"), ({"goals": FAKE + 8, "goals_onehot": 1}, b"misaligned inputs"),
    ({"onehot": FAKE + 8}, b"misaligned outputs"), ({"probs": FAKE + 2}, b"misaligned outputs"),
    ({"actions": FAKE + 2}, b"misaligned outputs")])
def test_rows_misaligned_pointer_is_refused(built, kw, needle):
    _refused(built, needle, rows=_rows(built, **kw))


def test_index_goals_need_no_alignment(built):
    """(uint8 index goals at an odd address pass the alignment check: the call stops at the next one it is made to fail)"""
    _refused(built, b"misaligned outputs", rows=_rows(built, goals=FAKE + 1, onehot=FAKE + 8))


@pytest.mark.parametrize("desc_kw,weights,rows_kw,needle", [
    ({"n_agents": 0}, None, {}, b"n_agents"),
    ({}, None, None, b"null weights"),
    ({"precision": 3}, "default", None, b"null rows"),
    ({"precision": 3, "stage": 0}, "default", {}, b"precision must be"),
    ({"stage": 0, "epsilon": 1.5}, "default", {}, b"stage must be"),
    ({"epsilon": 1.5}, "unpacked", {}, b"epsilon must be"),
    ({}, "unpacked", {"goals": None}, b"weights->packed is NULL"),
    ({}, "default", {"goals": None, "actions": None}, b"missing inputs"),
    ({}, "default", {"actions": None, "n_rows": 0}, b"no output requested"),
    ({}, "default", {"n_rows": 0, "goals_onehot": 2}, b"n_rows must be positive"),
    ({}, "default", {"n_rows": 64 * (2 ** 31 - 1) + 1, "goals_onehot": 2}, b"more than a grid"),
    ({}, "default", {"goals_onehot": 2, "obs_self_v": FAKE + 8}, b"form flags"),
    ({}, "default", {"obs_self_v": FAKE + 8, "actions": FAKE + 2}, b"misaligned inputs")])
def test_rows_checks_fire_in_their_order(built, desc_kw, weights, rows_kw, needle):
    """Two consecutive checks violated at once: the earlier one's message is the one reported."""
    w = {None: None, "default": _weights(built), "unpacked": _weights(built, packed=None)}[weights]
    _refused(built, needle, desc=_desc(built, **desc_kw), weights=w, rows=None if rows_kw is None else _rows(built, **rows_kw))


def test_the_actor_has_the_rows_methods():
    from cm3_amd.actor import CheckersActor
    for name in ("enqueue_rows", "probs_rows", "sample_rows", "soft_update_from"):
        assert callable(getattr(CheckersActor, name)), name


def _host_columns(checkers):
    import torch
    B, N = 3, 2
    z = lambda *s: torch.zeros(*s)                                          # noqa: E731
    if checkers:
        return {"grid": z(B, 3, 9, 2), "vec": z(B, N, 4), "obs_others": z(B, N, 2), "obs_self_t": z(B, N, 5, 5, 3),
                "obs_self_v": z(B, N, 4), "actions_prev": z(B, N).long(), "actions": z(B, N).long(), "reward": z(B),
                "local_rewards": z(B, N), "next_grid": z(B, 3, 9, 2), "next_vec": z(B, N, 4), "next_obs_others": z(B, N, 2),
                "next_obs_self_t": z(B, N, 5, 5, 3), "next_obs_self_v": z(B, N, 4), "done": z(B).bool(), "goals": z(B, N, 2)}
    return {"v_global": z(B, N, 4), "obs_others": z(B, N, 4), "v_local": z(B, N, 4), "actions": z(B, N).long(), "reward": z(B),
            "reward_local": z(B, N), "v_global_next": z(B, N, 4), "obs_others_next": z(B, N, 4), "v_local_next": z(B, N, 4),
            "done": z(B).bool(), "goals": z(B, N, 2)}


def _unreachable(ops, feed):
    raise AssertionError("run must not be reached: %s" % (ops,))


@pytest.mark.parametrize("which", ["target_actor", "actor"])
def test_train_step_feeds_refuses_device_actors_on_host_columns(which):
    from cm3_amd.actor import CheckersActor
    from cm3_amd.batch import train_step_feeds
    stand_in = object.__new__(CheckersActor)                                # (no GPU behind it: the check comes before any use)
    with pytest.raises(ValueError, match="device columns"):
        train_step_feeds(_host_columns(True), _unreachable, 0.99, 0.1, env="checkers", **{which: stand_in})


@pytest.mark.parametrize("which", ["target_actor", "actor"])
def test_train_step_feeds_refuses_an_actor_of_the_other_env(which):
    from cm3_amd.actor import CheckersActor, ParticleActor
    from cm3_amd.batch import train_step_feeds
    with pytest.raises(ValueError, match="CheckersActors.*ParticleActor"):
        train_step_feeds(_host_columns(True), _unreachable, 0.99, 0.1, env="checkers", **{which: object.__new__(ParticleActor)})
    with pytest.raises(ValueError, match="ParticleActors.*CheckersActor"):
        train_step_feeds(_host_columns(False), _unreachable, 0.99, 0.1, env="particle", **{which: object.__new__(CheckersActor)})
