"""CPU: the C ABI of the CM3 Checkers critics over transition rows (part of ABI 9, additive) -- cm3_critic_checkers_packed_bytes /
_pack / _rows_f32 declared, exported, bound; the three structs' layout as a C compiler sees it; every invalid argument refused
with a readable error before anything touches a GPU; train_step_feeds' refusals of critics it cannot use."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cm3_critic_checkers_packed_bytes", "cm3_critic_checkers_pack", "cm3_critic_checkers_rows_f32")
FAKE = 0x1000                                      # 16-byte aligned, never dereferenced: validation fails first
GLOBAL, CREDIT = 0, 1
ROWS, PAIRS, CF = 0, 1, 2
INPUTS = ("grid", "vec", "goals", "windows", "obs_self_v")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    return _lib


def test_header_declares_and_library_exports_the_entries(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cm3_amd.h")).read(), flags=re.S)
    handle = built.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(handle, name), name
        assert name in built.SYMBOLS, name
    assert built.ABI_VERSION == 9 and handle.cm3_abi_version() == 9
    assert re.search(r"#define\s+CM3_ABI_VERSION\s+9\b", text)
    import cm3_amd
    from cm3_amd.critic import CheckersCritic
    assert cm3_amd.CheckersCritic is CheckersCritic
    for name in ("repack", "soft_update_from", "enqueue", "q_rows", "q_pairs", "q_counterfactual"):
        assert callable(getattr(CheckersCritic, name)), name


def test_struct_layouts_match_the_header(built, tmp_path):
    structs = {"cm3_critic_checkers_desc": built.CriticCheckersDesc, "cm3_critic_checkers_weights": built.CriticCheckersWeights,
               "cm3_critic_checkers_rows": built.CriticCheckersRows}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cm3_amd.h"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        c, f, v = line.split()
        got[(c, f)] = int(v)
    for cname, cls in structs.items():
        assert ctypes.sizeof(cls) == got[(cname, "size")], cname
        for fname, _ in cls._fields_:
            assert getattr(cls, fname).offset == got[(cname, fname)], (cname, fname)
    assert [f for f, _ in built.CriticCheckersWeights._fields_] == [
        "conv_w", "conv_b", "conv_o_w", "conv_o_b", "w_b1", "b_b1", "w_b1_h2", "w_b2", "b_b2", "w_b2_h2", "w_out", "b_out", "packed"]
    assert [f for f, _ in built.CriticCheckersRows._fields_] == [
        "form", "reward_f64", "grid_f64", "windows_f64", "goals_onehot", "reserved", "grid", "vec", "goals", "actions", "windows",
        "obs_self_v", "reward", "done", "gamma", "q", "q64", "td", "n_steps"]


def test_packed_bytes(built):
    fn = built.lib().cm3_critic_checkers_packed_bytes
    for n in range(1, 9):
        assert fn(n, GLOBAL) > 0 and fn(n, GLOBAL) % 16 == 0
        assert (fn(n, CREDIT) > 0) == (n > 1) and fn(n, CREDIT) % 16 == 0
    # Toeplitz [64 x 112] + 112, [80 x 160] + 160, branch 1 [288 x 256] + 256, h2 [256 x 256], out [256 x 16] + 16 at one agent
    one = 64 * 112 + 112 + 80 * 160 + 160 + 288 * 256 + 256 + 256 * 256 + 256 * 16 + 16
    assert fn(1, GLOBAL) == 4 * one
    # + branch 2 [K2 -> whole groups of 16][32] + 32 and 32 more inputs of h2: K2 = 18 -> 32 (global, N = 3), 12 -> 16 (credit)
    assert fn(3, GLOBAL) == 4 * (one + 32 * 32 + 32 + 32 * 256)
    assert fn(3, CREDIT) == 4 * (one + 16 * 32 + 32 + 32 * 256)
    assert fn(8, GLOBAL) == 4 * (one + 64 * 32 + 32 + 32 * 256)
    for n, kind in ((0, GLOBAL), (9, GLOBAL), (10, CREDIT), (4, 2), (4, -1), (1, CREDIT)):
        assert fn(n, kind) == 0


def _desc(built, **kw):
    d = built.CriticCheckersDesc()
    d.n_agents, d.stage, d.kind = 4, 2, CREDIT
    d.grid_h, d.grid_w, d.grid_c, d.win_h, d.win_w, d.win_c = 3, 9, 2, 5, 5, 3
    d.n_h1_1, d.n_h1_2, d.n_h2 = 256, 32, 256
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _weights(built, **kw):
    w = built.CriticCheckersWeights()
    for f, _ in built.CriticCheckersWeights._fields_:
        setattr(w, f, FAKE)
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def _rows(built, **kw):
    r = built.CriticCheckersRows()
    r.form, r.n_steps, r.gamma, r.actions, r.q = PAIRS, 100, 0.99, FAKE, FAKE
    r.grid_f64 = r.windows_f64 = r.goals_onehot = 1
    for name in INPUTS:
        setattr(r, name, FAKE)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _refused(built, needle, desc="default", weights="default", rows="default"):
    handle = built.lib()
    d = _desc(built) if desc == "default" else desc
    w = _weights(built) if weights == "default" else weights
    r = _rows(built) if rows == "default" else rows
    ref = lambda x: None if x is None else ctypes.byref(x)      # noqa: E731
    rc = handle.cm3_critic_checkers_rows_f32(ref(d), ref(w), ref(r), None)
    assert rc == -1
    assert needle in handle.cm3_last_error(), handle.cm3_last_error()


def test_null_arguments_are_refused(built):
    _refused(built, b"null desc", desc=None)
    _refused(built, b"null weights", weights=None)
    _refused(built, b"null rows", rows=None)
    _refused(built, b"packed weights are NULL", weights=_weights(built, packed=None))


@pytest.mark.parametrize("kw,needle", [
    ({"n_agents": 0}, b"n_agents must be in 1..8"), ({"n_agents": 9}, b"n_agents must be in 1..8"),
    ({"kind": 2}, b"kind must be"), ({"kind": -1}, b"kind must be"), ({"stage": 0}, b"stage must be 1 or 2"),
    ({"stage": 3}, b"stage must be 1 or 2"),
    ({"n_agents": 1}, b"Q_credit_checkers exists at stage 2 with more than one agent only"),
    ({"stage": 1}, b"Q_credit_checkers exists at stage 2 with more than one agent only"),
    ({"kind": GLOBAL, "stage": 1}, b"Q_global_checkers runs at stage 1 with one agent"),
    ({"kind": GLOBAL, "n_agents": 1}, b"Q_global_checkers runs at stage 1 with one agent"),
    ({"grid_w": 8}, b"3x9x2 grid and a 5x5x3 window"), ({"grid_h": 4}, b"3x9x2 grid"), ({"grid_c": 3}, b"3x9x2 grid"),
    ({"win_h": 3}, b"5x5x3 window"), ({"win_w": 7}, b"5x5x3 window"), ({"win_c": 1}, b"5x5x3 window"),
    ({"n_h1_1": 128}, b"256/32/256"), ({"n_h1_2": 128}, b"256/32/256"), ({"n_h2": 32}, b"256/32/256")])
def test_invalid_descriptor_is_refused_without_a_gpu(built, kw, needle):
    _refused(built, needle, desc=_desc(built, **kw))
    handle = built.lib()
    assert handle.cm3_critic_checkers_pack(ctypes.byref(_desc(built, **kw)), ctypes.byref(_weights(built)), FAKE, None) == -1
    assert needle in handle.cm3_last_error()


@pytest.mark.parametrize("desc_kw,form", [
    ({}, ROWS), ({}, 3), ({}, -1),                                                  # credit: PAIRS and CF
    ({"kind": GLOBAL}, PAIRS), ({"kind": GLOBAL}, CF),                              # global at N > 1: ROWS
    ({"kind": GLOBAL, "n_agents": 1, "stage": 1}, PAIRS), ({"kind": GLOBAL, "n_agents": 1, "stage": 1}, 3)])
def test_a_form_the_kind_does_not_have_is_refused(built, desc_kw, form):
    _refused(built, b"does not exist for kind", desc=_desc(built, **desc_kw), rows=_rows(built, form=form))


@pytest.mark.parametrize("desc_kw,form,n_steps", [
    ({}, PAIRS, 0), ({}, PAIRS, -5),
    ({}, PAIRS, (2 ** 31 - 1) // 16 + 1), ({}, CF, (2 ** 31 - 1) // 80 + 1), ({"kind": GLOBAL}, ROWS, (2 ** 31 - 1) // 4 + 1),
    ({"kind": GLOBAL, "n_agents": 1, "stage": 1}, CF, (2 ** 31 - 1) // 5 + 1), ({"n_agents": 8}, CF, 2 ** 40)])
def test_row_count_out_of_range_is_refused(built, desc_kw, form, n_steps):
    _refused(built, b"n_steps", desc=_desc(built, **desc_kw), rows=_rows(built, form=form, n_steps=n_steps))


def test_missing_inputs_are_refused(built):
    for name in INPUTS:
        _refused(built, b"missing inputs: grid, vec, goals, windows and obs_self_v", rows=_rows(built, **{name: None}))
    _refused(built, b"read actions", rows=_rows(built, actions=None))
    _refused(built, b"read actions", desc=_desc(built, kind=GLOBAL), rows=_rows(built, form=ROWS, actions=None))
    _refused(built, b"td needs reward and done", rows=_rows(built, td=FAKE, done=FAKE))
    _refused(built, b"td needs reward and done", rows=_rows(built, td=FAKE, reward=FAKE))


def test_outputs(built):
    _refused(built, b"no output requested", rows=_rows(built, q=None))
    _refused(built, b"td is not defined for the counterfactual form", rows=_rows(built, form=CF, td=FAKE, reward=FAKE, done=FAKE))
    # the counterfactual form reads no actions: without them it passes that check and fails a later one
    _refused(built, b"misaligned", rows=_rows(built, form=CF, actions=None, q=FAKE + 2))


@pytest.mark.parametrize("kw,needle", [
    ({"vec": FAKE + 4}, b"misaligned inputs"), ({"obs_self_v": FAKE + 4}, b"misaligned inputs"), ({"actions": FAKE + 2}, b"misaligned inputs"),
    ({"grid": FAKE + 4}, b"misaligned inputs"), ({"windows": FAKE + 1}, b"misaligned inputs"), ({"goals": FAKE + 4}, b"misaligned inputs"),
    ({"td": FAKE, "done": FAKE, "reward": FAKE + 4, "reward_f64": 1}, b"misaligned reward"),
    ({"td": FAKE, "done": FAKE, "reward": FAKE + 2}, b"misaligned reward"),
    ({"q": FAKE + 2}, b"misaligned outputs"), ({"q64": FAKE + 4}, b"misaligned outputs"),
    ({"td": FAKE + 4, "done": FAKE, "reward": FAKE}, b"misaligned outputs")])
def test_misaligned_pointer_is_refused(built, kw, needle):
    _refused(built, needle, rows=_rows(built, **kw))
    _refused(built, b"misaligned packed", weights=_weights(built, packed=FAKE + 8))


def test_narrow_inputs_need_no_alignment(built):
    """int8 grids / windows and uint8 goals at odd addresses pass the alignment check (the next refusal is another one)"""
    r = _rows(built, grid=FAKE + 1, windows=FAKE + 3, goals=FAKE + 5, grid_f64=0, windows_f64=0, goals_onehot=0, q=None)
    _refused(built, b"no output requested", rows=r)


def test_pack_validates_before_launching(built):
    handle = built.lib()
    fn = handle.cm3_critic_checkers_pack
    d = _desc(built)
    assert fn(None, ctypes.byref(_weights(built)), FAKE, None) == -1 and b"null desc" in handle.cm3_last_error()
    assert fn(ctypes.byref(d), None, FAKE, None) == -1 and b"null weights" in handle.cm3_last_error()
    assert fn(ctypes.byref(d), ctypes.byref(_weights(built)), None, None) == -1 and b"packed is NULL" in handle.cm3_last_error()
    for name in ("conv_w", "conv_b", "conv_o_w", "conv_o_b", "w_b1", "b_b1", "w_b1_h2", "w_out", "b_out"):
        assert fn(ctypes.byref(d), ctypes.byref(_weights(built, **{name: None})), FAKE, None) == -1, name
        assert b"missing weights" in handle.cm3_last_error(), name
    assert fn(ctypes.byref(d), ctypes.byref(_weights(built, w_b2=None)), FAKE, None) == -1
    assert b"missing stage-2 weights" in handle.cm3_last_error()
    assert fn(ctypes.byref(d), ctypes.byref(_weights(built)), FAKE + 4, None) == -1 and b"misaligned packed" in handle.cm3_last_error()


# ---- train_step_feeds: critics it cannot use (no GPU: the critics are bare objects, the refusal comes before any launch) ----
def _bare(cls_name, kind, n):
    from cm3_amd import critic
    cls = getattr(critic, cls_name)
    c = cls.__new__(cls)
    c.kind, c.n, c.stage = kind, n, 1 if n == 1 else 2
    return c


def _checkers_cols(B=3, N=2):
    import torch
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)                        # noqa: E731
    Lo = 2 * max(N - 1, 1)
    return {"grid": z(B, 3, 9, 2), "vec": z(B, N, 4), "obs_others": z(B, N, Lo), "obs_self_t": z(B, N, 5, 5, 3),
            "obs_self_v": z(B, N, 4), "actions_prev": z(B, N).long(), "actions": z(B, N).long(), "reward": z(B),
            "local_rewards": z(B, N), "next_grid": z(B, 3, 9, 2), "next_vec": z(B, N, 4), "next_obs_others": z(B, N, Lo),
            "next_obs_self_t": z(B, N, 5, 5, 3), "next_obs_self_v": z(B, N, 4), "done": z(B).bool(), "goals": z(B, N, 2).long()}


def _particle_cols(B=3, N=2):
    import torch
    z = lambda *s: torch.zeros(*s)                                              # noqa: E731
    return {"v_global": z(B, N, 4), "obs_others": z(B, N, 4), "v_local": z(B, N, 4), "actions": z(B, N).long(), "reward": z(B),
            "reward_local": z(B, N), "v_global_next": z(B, N, 4), "obs_others_next": z(B, N, 4), "v_local_next": z(B, N, 4),
            "done": z(B).bool(), "goals": z(B, N, 2)}


def _never(ops, feed):
    raise AssertionError("run was called: the refusal must come first")


def test_a_critic_of_the_other_envs_class_is_refused():
    from cm3_amd.batch import train_step_feeds
    with pytest.raises(ValueError, match="q_credit takes a ParticleCritic of kind 'credit' for 2 agents, got a CheckersCritic"):
        train_step_feeds(_particle_cols(), _never, 0.99, 0.1, use_V=False, q_credit=_bare("CheckersCritic", "credit", 2))
    for cols in ({}, _checkers_cols()):                                        # (before the columns are read)
        with pytest.raises(ValueError, match="q_global_target is a ParticleCritic; env='checkers' has no device critics of that class"):
            train_step_feeds(cols, _never, 0.99, 0.1, env="checkers", use_V=False, q_global_target=_bare("ParticleCritic", "global", 2))
    with pytest.raises(ValueError, match="q_credit takes a CheckersCritic"):
        train_step_feeds(_checkers_cols(), _never, 0.99, 0.1, env="checkers", use_V=False, q_credit=object())


@pytest.mark.parametrize("kw,needle", [
    ({"q_global_target": ("credit", 2)}, "q_global_target takes a CheckersCritic of kind 'global' for 2 agents"),
    ({"q_credit_target": ("global", 2)}, "q_credit_target takes a CheckersCritic of kind 'credit' for 2 agents"),
    ({"q_credit": ("global", 2)}, "q_credit takes a CheckersCritic of kind 'credit' for 2 agents"),
    ({"q_credit": ("credit", 4)}, "q_credit takes a CheckersCritic of kind 'credit' for 2 agents"),
    ({"q_global_target": ("global", 3)}, "q_global_target takes a CheckersCritic of kind 'global' for 2 agents")])
def test_train_step_feeds_refuses_a_checkers_critic_of_the_wrong_kind_or_agent_count(kw, needle):
    from cm3_amd.batch import train_step_feeds
    critics = {k: _bare("CheckersCritic", *v) for k, v in kw.items()}
    with pytest.raises(ValueError, match=re.escape(needle)):
        train_step_feeds(_checkers_cols(), _never, 0.99, 0.1, env="checkers", use_V=False, **critics)


def test_train_step_feeds_refuses_checkers_critics_on_host_columns():
    from cm3_amd.batch import train_step_feeds
    with pytest.raises(ValueError, match="evaluate device columns"):
        train_step_feeds(_checkers_cols(), _never, 0.99, 0.1, env="checkers", use_V=False,
                         q_global_target=_bare("CheckersCritic", "global", 2))
    with pytest.raises(ValueError, match="kind 'global' for 1 agents"):       # one agent: q_credit is the Q_global_main critic
        train_step_feeds(_checkers_cols(N=1), _never, 0.99, 0.1, env="checkers", use_V=False, q_credit=_bare("CheckersCritic", "credit", 2))
    with pytest.raises(ValueError, match="evaluate device columns"):
        train_step_feeds(_checkers_cols(N=1), _never, 0.99, 0.1, env="checkers", use_V=False, q_credit=_bare("CheckersCritic", "global", 1))
