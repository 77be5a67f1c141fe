"""CPU: the C ABI of the Checkers QMIX mixer over transition rows (part of ABI 9, additive) -- cm3_qmix_mixer_checkers_packed_bytes /
_pack / _rows_f32 declared, exported, bound; the three structs' layout as a C compiler sees it; every invalid argument refused with a
readable error before anything touches a GPU; qmix_train_step_feeds' refusals of a target_mixer it cannot use under env="checkers"."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cm3_qmix_mixer_checkers_packed_bytes", "cm3_qmix_mixer_checkers_pack", "cm3_qmix_mixer_checkers_rows_f32")
FAKE = 0x1000                                      # 16-byte aligned, never dereferenced: validation fails first
WEIGHTS = ["conv_w", "conv_b", "hyper_w_1", "hyper_w_final", "hyper_b_1", "hyper_b_final_l1", "hyper_b_final"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    return _lib


def test_header_declares_and_library_exports_the_entries(built):
    raw = open(os.path.join(ROOT, "include", "cm3_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    handle = built.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(handle, name), name
        assert name in built.SYMBOLS, name
    assert built.ABI_VERSION == 9 and handle.cm3_abi_version() == 9
    assert re.search(r"#define\s+CM3_ABI_VERSION\s+9\b", text)
    assert "cm3_qmix_mixer_checkers_packed_bytes / _pack / _rows_f32" in raw            # the ABI-9 comment names the addition
    # anonymous struct tags, like cm3_qmix_rows
    for name in ("cm3_qmix_mixer_checkers_desc", "cm3_qmix_mixer_checkers_weights", "cm3_qmix_mixer_checkers_rows"):
        assert re.search(r"\}\s*%s\s*;" % name, text) and not re.search(r"typedef struct %s\b" % name, text), name


def test_struct_layouts_match_the_header(built, tmp_path):
    structs = {"cm3_qmix_mixer_checkers_desc": built.QmixMixerCheckersDesc, "cm3_qmix_mixer_checkers_weights": built.QmixMixerCheckersWeights,
               "cm3_qmix_mixer_checkers_rows": built.QmixMixerCheckersRows}
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
    assert [f for f, _ in built.QmixMixerCheckersDesc._fields_] == ["n_agents", "embed_dim", "grid_h", "grid_w", "grid_c", "conv_f", "conv_kh",
                                                                     "conv_kw"]
    assert [f for f, _ in built.QmixMixerCheckersWeights._fields_] == WEIGHTS + ["packed"]
    assert [f for f, _ in built.QmixMixerCheckersRows._fields_] == ["grid_f64", "goals_onehot", "reward_f64", "reserved", "grid", "vec", "goals",
                                                                     "agent_qs", "reward", "done", "gamma", "q_tot", "q_tot64", "td", "n_steps"]


def test_packed_bytes(built):
    fn = built.lib().cm3_qmix_mixer_checkers_packed_bytes
    for n in range(1, 9):
        assert fn(n) > 0 and fn(n) % 16 == 0
    # the Toeplitz matrix [64 x 128] as 8 column tiles x 4 k groups of [64 lanes][4], its 128 bias values, N + 3 column blocks of
    # 8 column tiles x KG k groups (K = 108 + 6 N zero-padded to whole groups of 16) and the 128 weights of hyper_b_final:
    # N = 1: K = 114 -> 128, 8 groups;  N = 4: K = 132 -> 144, 9 groups;  N = 8: K = 156 -> 160, 10 groups
    conv = 8 * 4 * 256 + 128
    assert fn(1) == 4 * (conv + 4 * 8 * 8 * 256 + 128)
    assert fn(2) == 4 * (conv + 5 * 8 * 8 * 256 + 128)
    assert fn(4) == 4 * (conv + 7 * 8 * 9 * 256 + 128)
    assert fn(8) == 4 * (conv + 11 * 8 * 10 * 256 + 128)
    for n in (0, 9, 10, -1):
        assert fn(n) == 0


def _desc(built, **kw):
    d = built.QmixMixerCheckersDesc()
    d.n_agents, d.embed_dim = 3, 128
    d.grid_h, d.grid_w, d.grid_c = 3, 9, 2
    d.conv_f, d.conv_kh, d.conv_kw = 4, 3, 5
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _weights(built, **kw):
    w = built.QmixMixerCheckersWeights()
    for f, _ in built.QmixMixerCheckersWeights._fields_:
        setattr(w, f, FAKE)
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def _rows(built, **kw):
    r = built.QmixMixerCheckersRows()
    r.grid, r.vec, r.goals, r.agent_qs, r.q_tot, r.n_steps, r.gamma = FAKE, FAKE, FAKE, FAKE, FAKE, 100, 0.99
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _refused(built, needle, desc="default", weights="default", rows="default"):
    handle = built.lib()
    d = _desc(built) if desc == "default" else desc
    w = _weights(built) if weights == "default" else weights
    r = _rows(built) if rows == "default" else rows
    ref = lambda x: None if x is None else ctypes.byref(x)      # noqa: E731
    rc = handle.cm3_qmix_mixer_checkers_rows_f32(ref(d), ref(w), ref(r), None)
    assert rc == -1                                              # CM3_ERR_INVALID
    assert needle in handle.cm3_last_error(), handle.cm3_last_error()


def test_null_arguments_are_refused(built):
    _refused(built, b"null desc", desc=None)
    _refused(built, b"null weights", weights=None)
    _refused(built, b"null rows", rows=None)
    _refused(built, b"packed weights are NULL", weights=_weights(built, packed=None))


@pytest.mark.parametrize("kw,needle", [
    ({"n_agents": 0}, b"n_agents must be in 1..8"), ({"n_agents": 9}, b"n_agents must be in 1..8"), ({"n_agents": -3}, b"n_agents must be in 1..8"),
    ({"embed_dim": 64}, b"embedding width"), ({"embed_dim": 0}, b"embedding width"),
    ({"grid_h": 4}, b"3x9x2 grid"), ({"grid_w": 8}, b"3x9x2 grid"), ({"grid_c": 3}, b"3x9x2 grid"),
    ({"conv_f": 6}, b"4 filters of 3x5"), ({"conv_kh": 5}, b"4 filters of 3x5"), ({"conv_kw": 3}, b"4 filters of 3x5")])
def test_invalid_descriptor_is_refused_without_a_gpu(built, kw, needle):
    _refused(built, needle, desc=_desc(built, **kw))
    handle = built.lib()
    assert handle.cm3_qmix_mixer_checkers_pack(ctypes.byref(_desc(built, **kw)), ctypes.byref(_weights(built)), FAKE, None) == -1
    assert needle in handle.cm3_last_error()


@pytest.mark.parametrize("n_steps", [0, -5, 2 ** 31, 2 ** 40])
def test_row_count_out_of_range_is_refused(built, n_steps):
    _refused(built, b"n_steps", rows=_rows(built, n_steps=n_steps))


def test_missing_inputs_and_outputs_are_refused(built):
    for name in ("grid", "vec", "goals", "agent_qs"):
        _refused(built, b"missing inputs: grid, vec, goals and agent_qs", rows=_rows(built, **{name: None}))
    _refused(built, b"no output requested", rows=_rows(built, q_tot=None))
    _refused(built, b"td needs reward and done", rows=_rows(built, td=FAKE, done=FAKE))
    _refused(built, b"td needs reward and done", rows=_rows(built, td=FAKE, reward=FAKE))
    # each output alone passes the output check and fails a later one
    _refused(built, b"misaligned", rows=_rows(built, q_tot=None, q_tot64=FAKE + 4))
    _refused(built, b"misaligned", rows=_rows(built, q_tot=None, td=FAKE + 4, reward=FAKE, done=FAKE))


@pytest.mark.parametrize("kw,needle", [
    ({"vec": FAKE + 4}, b"misaligned inputs"), ({"agent_qs": FAKE + 2}, b"misaligned inputs"),
    ({"grid": FAKE + 4, "grid_f64": 1}, b"misaligned inputs"), ({"goals": FAKE + 4, "goals_onehot": 1}, b"misaligned inputs"),
    ({"td": FAKE, "done": FAKE, "reward": FAKE + 4, "reward_f64": 1}, b"misaligned reward"),
    ({"td": FAKE, "done": FAKE, "reward": FAKE + 2}, b"misaligned reward"),
    ({"q_tot": FAKE + 2}, b"misaligned outputs"), ({"q_tot64": FAKE + 4}, b"misaligned outputs"),
    ({"td": FAKE + 4, "done": FAKE, "reward": FAKE}, b"misaligned outputs")])
def test_misaligned_pointer_is_refused(built, kw, needle):
    _refused(built, needle, rows=_rows(built, **kw))
    _refused(built, b"misaligned packed", weights=_weights(built, packed=FAKE + 8))


def test_byte_columns_need_no_alignment(built):
    """an int8 grid and uint8 index goals at odd addresses pass the alignment check (the next refusal is the one seen)"""
    _refused(built, b"no output requested", rows=_rows(built, grid=FAKE + 1, goals=FAKE + 3, q_tot=None))


def test_pack_validates_before_launching(built):
    handle = built.lib()
    fn = handle.cm3_qmix_mixer_checkers_pack
    d = _desc(built)
    assert fn(None, ctypes.byref(_weights(built)), FAKE, None) == -1 and b"null desc" in handle.cm3_last_error()
    assert fn(ctypes.byref(d), None, FAKE, None) == -1 and b"null weights" in handle.cm3_last_error()
    assert fn(ctypes.byref(d), ctypes.byref(_weights(built)), None, None) == -1 and b"packed is NULL" in handle.cm3_last_error()
    for name in WEIGHTS:
        assert fn(ctypes.byref(d), ctypes.byref(_weights(built, **{name: None})), FAKE, None) == -1
        assert b"missing weights" in handle.cm3_last_error(), name
    assert fn(ctypes.byref(d), ctypes.byref(_weights(built)), FAKE + 4, None) == -1 and b"misaligned packed" in handle.cm3_last_error()


# ---- qmix_train_step_feeds: a target_mixer it cannot use (no GPU: bare objects, the refusal comes before any launch) ----
def _bare(cls_name, n):
    from cm3_amd import qmix
    cls = getattr(qmix, cls_name)
    m = cls.__new__(cls)
    m.n = n
    return m


def _host_cols(B=3, N=2):
    from tests.critic_checkers_feeds import make_cols
    return make_cols(B, N, 1)


class _Untouchable(dict):
    """columns that must not be read"""

    def __getitem__(self, key):
        raise AssertionError("cols[%r] was read: the refusal must come first" % (key,))


def _never(ops, feed):
    raise AssertionError("run was called: the refusal must come first")


def test_train_step_feeds_refuses_a_target_mixer_it_cannot_use():
    from cm3_amd.batch import qmix_train_step_feeds
    cols = _host_cols()
    agent, mixer = _bare("CheckersQmixAgent", 2), _bare("CheckersQmixMixer", 2)
    # what needs no column: the type (a particle mixer, any other object), the missing target agent
    for wrong, name in ((_bare("ParticleQmixMixer", 2), "ParticleQmixMixer"), (object(), "object"), (agent, "CheckersQmixAgent")):
        with pytest.raises(ValueError, match="env='checkers' takes a CheckersQmixMixer as target_mixer, got %s: the Checkers mixer is not built "
                                             "from another network's weights; build a CheckersQmixMixer" % name):
            qmix_train_step_feeds(_Untouchable(), _never, 0.99, env="checkers", target_agent=agent, target_mixer=wrong)
    with pytest.raises(ValueError, match="pass target_agent .a CheckersQmixAgent holding the Agent_target weights."):
        qmix_train_step_feeds(_Untouchable(), _never, 0.99, env="checkers", target_mixer=mixer)
    with pytest.raises(ValueError, match="mixer_q_agent names the agent .* pass target_mixer as well"):
        qmix_train_step_feeds(_Untouchable(), _never, 0.99, env="checkers", target_agent=agent, mixer_q_agent=agent)
    # what reads the batch's shape and device
    with pytest.raises(ValueError, match=re.escape("target_mixer takes a CheckersQmixMixer for 2 agents (the batch's count), got one for 4")):
        qmix_train_step_feeds(cols, _never, 0.99, env="checkers", target_agent=agent, target_mixer=_bare("CheckersQmixMixer", 4))
    with pytest.raises(ValueError, match="target_mixer evaluates device columns; call without it"):
        qmix_train_step_feeds(cols, _never, 0.99, env="checkers", target_agent=agent, target_mixer=mixer)
    # under env="particle" a Checkers mixer is no ParticleQmixMixer
    from tests.test_qmix_mixer_abi import _bare_agent, _host_cols as particle_cols
    with pytest.raises(ValueError, match=re.escape("target_mixer takes a ParticleQmixMixer for 2 agents (the batch's count), got CheckersQmixMixer")):
        qmix_train_step_feeds(particle_cols(), _never, 0.99, target_agent=_bare_agent(2), target_mixer=mixer)
    with pytest.raises(ValueError, match="mixer_q_agent belongs to env='checkers'"):
        qmix_train_step_feeds(_Untouchable(), _never, 0.99, target_agent=_bare_agent(2), mixer_q_agent=_bare_agent(2))


def test_the_class_is_exported():
    import cm3_amd
    from cm3_amd.qmix import CheckersQmixMixer
    assert cm3_amd.CheckersQmixMixer is CheckersQmixMixer
