"""CPU: the C ABI of the CM3 particle critics over transition rows (part of ABI 9, additive) -- cm3_critic_particle_packed_bytes /
_pack / _rows_f32 declared, exported, bound; the three structs' layout as a C compiler sees it; every invalid argument refused
with a readable error before anything touches a GPU; train_step_feeds' refusals of critics it cannot use."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cm3_critic_particle_packed_bytes", "cm3_critic_particle_pack", "cm3_critic_particle_rows_f32")
FAKE = 0x1000                                      # 16-byte aligned, never dereferenced: validation fails first
GLOBAL, CREDIT = 0, 1
ROWS, PAIRS, CF = 0, 1, 2


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
    for name, value in (("CM3_CRITIC_GLOBAL", 0), ("CM3_CRITIC_CREDIT", 1), ("CM3_CRITIC_ROWS", 0), ("CM3_CRITIC_PAIRS", 1),
                        ("CM3_CRITIC_CF", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    assert (built.CRITIC_GLOBAL, built.CRITIC_CREDIT, built.CRITIC_ROWS, built.CRITIC_PAIRS, built.CRITIC_CF) == (0, 1, 0, 1, 2)


def test_struct_layouts_match_the_header(built, tmp_path):
    structs = {"cm3_critic_particle_desc": built.CriticParticleDesc, "cm3_critic_particle_weights": built.CriticParticleWeights,
               "cm3_critic_rows": built.CriticRows}
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
    assert [f for f, _ in built.CriticRows._fields_] == ["form", "reward_f64", "state", "goals", "actions", "reward", "done", "gamma",
                                                          "q", "q64", "td", "n_steps"]
    assert [f for f, _ in built.CriticParticleWeights._fields_] == ["w_b1", "b_b1", "w_b1_h2", "w_b2", "b_b2", "w_b2_h2", "w_out",
                                                                     "packed"]


def test_packed_bytes(built):
    fn = built.lib().cm3_critic_particle_packed_bytes
    for n in range(1, 11):
        assert fn(n, GLOBAL) > 0 and fn(n, GLOBAL) % 16 == 0
        assert (fn(n, CREDIT) > 0) == (n > 1)
    # branch 1 [4][64][4] + bias 64, h2 [4][64][16], out [64][16] at one agent
    assert fn(1, GLOBAL) == 4 * (1024 + 64 + 4096 + 1024)
    # + branch 2 [4][2][64][S2P] + bias 128 and 48 k-steps of h2: K2 = 27 -> 7 k-steps -> stride 8 (global), 16 -> 4 -> 4 (credit)
    assert fn(4, GLOBAL) == 4 * (1024 + 64 + 512 * 8 + 128 + 4 * 64 * 48 + 1024)
    assert fn(4, CREDIT) == 4 * (1024 + 64 + 512 * 4 + 128 + 4 * 64 * 48 + 1024)
    for n, kind in ((0, GLOBAL), (11, GLOBAL), (4, 2), (4, -1)):
        assert fn(n, kind) == 0


def _desc(built, **kw):
    d = built.CriticParticleDesc()
    d.n_agents, d.stage, d.kind, d.n_h1_1, d.n_h1_2, d.n_h2 = 4, 2, CREDIT, 64, 128, 64
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _weights(built, **kw):
    w = built.CriticParticleWeights()
    for f, _ in built.CriticParticleWeights._fields_:
        setattr(w, f, FAKE)
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def _rows(built, **kw):
    r = built.CriticRows()
    r.form, r.state, r.goals, r.actions, r.q, r.n_steps, r.gamma = PAIRS, FAKE, FAKE, FAKE, FAKE, 100, 0.99
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _refused(built, needle, desc="default", weights="default", rows="default"):
    handle = built.lib()
    d = _desc(built) if desc == "default" else desc
    w = _weights(built) if weights == "default" else weights
    r = _rows(built) if rows == "default" else rows
    ref = lambda x: None if x is None else ctypes.byref(x)      # noqa: E731
    rc = handle.cm3_critic_particle_rows_f32(ref(d), ref(w), ref(r), None)
    assert rc == -1
    assert needle in handle.cm3_last_error(), handle.cm3_last_error()


def test_null_arguments_are_refused(built):
    _refused(built, b"null desc", desc=None)
    _refused(built, b"null weights", weights=None)
    _refused(built, b"null rows", rows=None)
    _refused(built, b"packed weights are NULL", weights=_weights(built, packed=None))


@pytest.mark.parametrize("kw,needle", [
    ({"n_agents": 0}, b"n_agents must be in 1..10"), ({"n_agents": 11}, b"n_agents must be in 1..10"),
    ({"kind": 2}, b"kind must be"), ({"kind": -1}, b"kind must be"), ({"stage": 0}, b"stage must be 1 or 2"),
    ({"stage": 3}, b"stage must be 1 or 2"),
    ({"n_agents": 1}, b"Q_credit exists at stage 2 with more than one agent only"),
    ({"stage": 1}, b"Q_credit exists at stage 2 with more than one agent only"),
    ({"kind": GLOBAL, "stage": 1}, b"Q_global_1output runs at stage 1 with one agent"),
    ({"kind": GLOBAL, "n_agents": 1}, b"Q_global_1output runs at stage 1 with one agent"),
    ({"n_h1_1": 128}, b"64/128/64"), ({"n_h1_2": 64}, b"64/128/64"), ({"n_h2": 32}, b"64/128/64")])
def test_invalid_descriptor_is_refused_without_a_gpu(built, kw, needle):
    _refused(built, needle, desc=_desc(built, **kw))
    handle = built.lib()
    assert handle.cm3_critic_particle_pack(ctypes.byref(_desc(built, **kw)), ctypes.byref(_weights(built)), FAKE, None) == -1
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
    ({"kind": GLOBAL, "n_agents": 1, "stage": 1}, CF, (2 ** 31 - 1) // 5 + 1), ({"n_agents": 10}, CF, 2 ** 40)])
def test_row_count_out_of_range_is_refused(built, desc_kw, form, n_steps):
    _refused(built, b"n_steps", desc=_desc(built, **desc_kw), rows=_rows(built, form=form, n_steps=n_steps))


def test_missing_inputs_are_refused(built):
    for name in ("state", "goals"):
        _refused(built, b"missing inputs: state and goals", rows=_rows(built, **{name: None}))
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
    ({"state": FAKE + 8}, b"misaligned inputs"), ({"goals": FAKE + 4}, b"misaligned inputs"), ({"actions": FAKE + 2}, b"misaligned inputs"),
    ({"td": FAKE, "done": FAKE, "reward": FAKE + 4, "reward_f64": 1}, b"misaligned reward"),
    ({"td": FAKE, "done": FAKE, "reward": FAKE + 2}, b"misaligned reward"),
    ({"q": FAKE + 2}, b"misaligned outputs"), ({"q64": FAKE + 4}, b"misaligned outputs"),
    ({"td": FAKE + 4, "done": FAKE, "reward": FAKE}, b"misaligned outputs")])
def test_misaligned_pointer_is_refused(built, kw, needle):
    _refused(built, needle, rows=_rows(built, **kw))
    _refused(built, b"misaligned packed", weights=_weights(built, packed=FAKE + 8))


def test_pack_validates_before_launching(built):
    handle = built.lib()
    fn = handle.cm3_critic_particle_pack
    d = _desc(built)
    assert fn(None, ctypes.byref(_weights(built)), FAKE, None) == -1 and b"null desc" in handle.cm3_last_error()
    assert fn(ctypes.byref(d), None, FAKE, None) == -1 and b"null weights" in handle.cm3_last_error()
    assert fn(ctypes.byref(d), ctypes.byref(_weights(built)), None, None) == -1 and b"packed is NULL" in handle.cm3_last_error()
    assert fn(ctypes.byref(d), ctypes.byref(_weights(built, w_out=None)), FAKE, None) == -1 and b"missing weights" in handle.cm3_last_error()
    assert fn(ctypes.byref(d), ctypes.byref(_weights(built, w_b2=None)), FAKE, None) == -1
    assert b"missing stage-2 weights" in handle.cm3_last_error()
    assert fn(ctypes.byref(d), ctypes.byref(_weights(built)), FAKE + 4, None) == -1 and b"misaligned packed" in handle.cm3_last_error()


# ---- train_step_feeds: critics it cannot use (no GPU: the critics are bare objects, the refusal comes before any launch) ----
def _bare_critic(kind, n):
    from cm3_amd.critic import ParticleCritic
    c = ParticleCritic.__new__(ParticleCritic)
    c.kind, c.n, c.stage = kind, n, 1 if n == 1 else 2
    return c


def _host_cols(B=3, N=2):
    import torch
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)      # noqa: E731
    L = 4 * max(N - 1, 1)
    return {"v_global": r(B, N, 4), "obs_others": r(B, N, L), "v_local": r(B, N, 4), "actions": torch.randint(0, 5, (B, N), generator=g),
            "reward": r(B), "reward_local": r(B, N), "v_global_next": r(B, N, 4), "obs_others_next": r(B, N, L),
            "v_local_next": r(B, N, 4), "done": torch.zeros(B, dtype=torch.bool), "goals": r(B, N, 2)}


def _never(ops, feed):
    raise AssertionError("run was called: the refusal must come first")


@pytest.mark.parametrize("kw,needle", [
    ({"q_global_target": ("credit", 2)}, "q_global_target takes a ParticleCritic of kind 'global' for 2 agents"),
    ({"q_credit_target": ("global", 2)}, "q_credit_target takes a ParticleCritic of kind 'credit' for 2 agents"),
    ({"q_credit": ("global", 2)}, "q_credit takes a ParticleCritic of kind 'credit' for 2 agents"),
    ({"q_credit": ("credit", 4)}, "q_credit takes a ParticleCritic of kind 'credit' for 2 agents"),
    ({"q_global_target": ("global", 3)}, "q_global_target takes a ParticleCritic of kind 'global' for 2 agents")])
def test_train_step_feeds_refuses_a_critic_of_the_wrong_kind_or_agent_count(kw, needle):
    from cm3_amd.batch import train_step_feeds
    critics = {k: _bare_critic(*v) for k, v in kw.items()}
    with pytest.raises(ValueError, match=re.escape(needle)):
        train_step_feeds(_host_cols(), _never, 0.99, 0.1, use_V=False, **critics)


def test_train_step_feeds_refuses_what_is_no_critic():
    from cm3_amd.batch import train_step_feeds
    with pytest.raises(ValueError, match="q_credit takes a ParticleCritic"):
        train_step_feeds(_host_cols(), _never, 0.99, 0.1, use_V=False, q_credit=object())
    with pytest.raises(ValueError, match="kind 'global' for 1 agents"):     # one agent: q_credit is the Q_global_main critic
        train_step_feeds(_host_cols(N=1), _never, 0.99, 0.1, use_V=False, q_credit=_bare_critic("credit", 2))


def test_train_step_feeds_refuses_critics_on_host_columns_and_on_checkers():
    from cm3_amd.batch import train_step_feeds
    with pytest.raises(ValueError, match="evaluate device columns"):
        train_step_feeds(_host_cols(), _never, 0.99, 0.1, use_V=False, q_global_target=_bare_critic("global", 2))
    with pytest.raises(ValueError, match="evaluate device columns"):
        train_step_feeds(_host_cols(N=1), _never, 0.99, 0.1, use_V=False, q_credit=_bare_critic("global", 1))
    with pytest.raises(ValueError, match="env='checkers' has no device critics"):
        train_step_feeds({}, _never, 0.99, 0.1, env="checkers", q_credit_target=_bare_critic("credit", 2))
