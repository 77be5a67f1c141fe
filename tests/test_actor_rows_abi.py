"""CPU: the C ABI of the CM3 actor over transition rows (part of ABI 9, additive) -- cm3_actor_particle_rows_f32 declared,
exported, bound; the cm3_actor_rows layout as a C compiler sees it; every invalid argument refused with a readable error before
anything touches a GPU; the restated rows draw is a stream of its own."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import actor_oracle as AO
from tests import actor_rows_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "cm3_actor_particle_rows_f32"
FAKE = 0x1000                                      # 16-byte aligned, never dereferenced: validation fails first
FIELDS = ["obs_others", "v_obs", "goals", "probs", "actions", "onehot", "epsilon_dev", "n_rows", "row_id_base", "draw", "_pad"]


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
    """sizeof and every field offset of cm3_actor_rows (an anonymous-tag struct), as a C compiler sees include/cm3_amd.h, against
    the ctypes mirror."""
    cls = built.ActorRows
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cm3_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(cm3_actor_rows));']
    for fname, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(cm3_actor_rows, %s));' % (fname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert ctypes.sizeof(cls) == got["size"] == 80 and got["size"] % 8 == 0
    assert [f for f, _ in cls._fields_] == FIELDS
    for fname, _ in cls._fields_:
        assert getattr(cls, fname).offset == got[fname], fname
    text = open(os.path.join(ROOT, "include", "cm3_amd.h")).read()
    assert not re.search(r"typedef struct cm3_actor_rows", text)         # (anonymous tag: tests/test_abi.py's table stays as it is)


def _desc(built, **kw):
    d = built.ActorParticleDesc()
    d.n_envs, d.n_agents, d.stage = 0, 4, 2                              # n_envs and env_id_base: not read
    d.n_h1_self, d.n_h1_others, d.n_h2, d.n_actions = 64, 128, 64, 5
    d.epsilon, d.precision, d.seed = 0.25, 0, 12341
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _weights(built, packed=FAKE):
    w = built.ActorParticleWeights()
    w.packed = packed
    return w


def _rows(built, **kw):
    r = built.ActorRows()
    r.obs_others, r.v_obs, r.goals, r.actions, r.n_rows = FAKE, FAKE, FAKE, FAKE, 100
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
    ("n_agents", 0, b"n_agents"), ("n_agents", 11, b"n_agents"), ("n_h1_self", 128, b"64/128/64/5"), ("n_h1_others", 64, b"64/128/64/5"),
    ("n_h2", 32, b"64/128/64/5"), ("n_actions", 4, b"64/128/64/5"), ("precision", 3, b"precision"), ("precision", -1, b"precision"),
    ("epsilon", 1.5, b"epsilon"), ("epsilon", -0.1, b"epsilon")])
def test_rows_invalid_descriptor_is_refused_without_a_gpu(built, field, value, needle):
    _refused(built, needle, desc=_desc(built, **{field: value}))


def test_rows_null_arguments_are_refused(built):
    _refused(built, b"null desc", desc=None)
    _refused(built, b"null weights", weights=None)
    _refused(built, b"null rows", rows=None)


def test_rows_without_packed_weights_are_refused(built):
    _refused(built, b"weights->packed is NULL", weights=_weights(built, packed=None))


@pytest.mark.parametrize("name", ["obs_others", "v_obs", "goals"])
def test_rows_missing_input_is_refused(built, name):
    _refused(built, b"missing inputs", rows=_rows(built, **{name: None}))


def test_rows_without_an_output_are_refused(built):
    _refused(built, b"no output requested", rows=_rows(built, actions=None))
    for name in ("probs", "onehot"):                                       # any single output is enough to pass THIS check
        _refused(built, b"n_rows", rows=_rows(built, actions=None, n_rows=0, **{name: FAKE}))


@pytest.mark.parametrize("n_rows", [0, -1, 64 * (2 ** 31 - 1) + 1])
def test_rows_count_out_of_range_is_refused(built, n_rows):
    _refused(built, b"n_rows", rows=_rows(built, n_rows=n_rows))


@pytest.mark.parametrize("name,value,needle", [
    ("obs_others", FAKE + 8, b"misaligned inputs"), ("v_obs", FAKE + 4, b"misaligned inputs"), ("goals", FAKE + 4, b"misaligned inputs"),
    ("onehot", FAKE + 8, b"misaligned onehot")])
def test_rows_misaligned_pointer_is_refused(built, name, value, needle):
    _refused(built, needle, rows=_rows(built, **{name: value}))


@pytest.mark.parametrize("desc_kw,weights,rows_kw,needle", [
    ({"n_h2": 32}, None, {}, b"64/128/64/5"),
    ({}, None, None, b"null weights"),
    ({"epsilon": 1.5}, "default", None, b"null rows"),
    ({"epsilon": 1.5, "precision": 3}, "default", {}, b"epsilon must be"),
    ({"precision": 3}, "unpacked", {}, b"precision must be"),
    ({}, "unpacked", {"goals": None}, b"weights->packed is NULL"),
    ({}, "default", {"goals": None, "actions": None}, b"missing inputs"),
    ({}, "default", {"actions": None, "n_rows": 0}, b"no output requested"),
    ({}, "default", {"n_rows": 0, "v_obs": FAKE + 4}, b"n_rows must be positive"),
    ({}, "default", {"n_rows": 64 * (2 ** 31 - 1) + 1, "v_obs": FAKE + 4}, b"more than a grid"),
    ({}, "default", {"v_obs": FAKE + 4, "onehot": FAKE + 8}, b"misaligned inputs")])
def test_rows_checks_fire_in_their_order(built, desc_kw, weights, rows_kw, needle):
    """Two consecutive checks violated at once: the earlier one's message is the one reported."""
    w = {None: None, "default": _weights(built), "unpacked": _weights(built, packed=None)}[weights]
    _refused(built, needle, desc=_desc(built, **desc_kw), weights=w, rows=None if rows_kw is None else _rows(built, **rows_kw))


def test_the_actor_has_the_rows_methods():
    from cm3_amd.actor import ParticleActor
    for name in ("enqueue_rows", "probs_rows", "sample_rows", "soft_update_from"):
        assert callable(getattr(ParticleActor, name)), name


@pytest.mark.parametrize("which", ["target_actor", "actor"])
def test_train_step_feeds_refuses_device_actors_on_host_columns(which):
    import torch
    from cm3_amd.batch import train_step_feeds
    B, N = 3, 2
    z = lambda *s: torch.zeros(*s)                                          # noqa: E731
    cols = {"v_global": z(B, N, 4), "obs_others": z(B, N, 4), "v_local": z(B, N, 4), "actions": z(B, N).long(), "reward": z(B),
            "reward_local": z(B, N), "v_global_next": z(B, N, 4), "obs_others_next": z(B, N, 4), "v_local_next": z(B, N, 4),
            "done": z(B).bool(), "goals": z(B, N, 2)}

    def run(ops, feed):
        raise AssertionError("run must not be reached: %s" % (ops,))
    with pytest.raises(ValueError, match="device columns"):
        train_step_feeds(cols, run, 0.99, 0.1, **{which: object()})
    with pytest.raises(ValueError, match="Checkers"):
        train_step_feeds(cols, run, 0.99, 0.1, env="checkers", **{which: object()})


def test_restated_uniforms_lie_in_the_open_unit_interval():
    for seed, draw, base in ((12341, 0, 0), (2 ** 63 + 5, 7, 2 ** 40), (77, 2 ** 32 - 1, 2 ** 64 - 2000)):
        u = RR.rows_uniforms(seed, 4096, draw, row_id_base=base)
        assert u.dtype == np.float32 and u.shape == (4096,)
        assert (u > 0).all() and (u < 1).all()
        assert abs(float(u.mean()) - 0.5) < 0.03                            # (4096 uniforms: sigma of the mean 0.0045)
    a, b = RR.rows_uniforms(5, 1000, 0), RR.rows_uniforms(5, 1000, 1)
    assert (a != b).mean() > 0.99                                            # the launch counter moves every draw
    assert np.array_equal(RR.rows_uniforms(5, 10, 3, row_id_base=990), RR.rows_uniforms(5, 1000, 3)[990:])


@pytest.mark.parametrize("N", [1, 4, 10])
def test_rows_draw_is_not_the_policy_stream(N):
    """the same ids as global env ids of the collection stream (episode 0, step 0, which leave counter word 2 at the rows stream's
    draw 0): a purpose collision would make whole columns equal."""
    seed, E = 12341, 512
    pol = AO.policy_uniforms(seed, np.arange(E), 0, 0, N)
    rows = RR.rows_uniforms(seed, E, 0)
    assert RR.PURPOSE_ROWS == 1 << 28 and RR.PURPOSE_ROWS & (AO.PURPOSE_POLICY | 0x20000000 | 0x80000000 | (0xF << 24)) == 0
    for i in range(N):
        assert (pol[:, i] == rows).mean() < 0.01, i
    blocks = RR.rows_words(seed, np.arange(E), 0)
    from oracle import philox
    for call in range((N + 3) // 4):
        for word in philox.action_block(seed, np.arange(E), call):
            assert (word == blocks).mean() < 0.01


def test_row_id_base_field_widths_are_the_headers():
    """cm3_actor_rows.row_id_base is int64_t, cm3_actor_checkers_rows.row_id_base uint64_t: the ctypes mirrors hold the same types,
    draw is 32 bits in both, and a 64-bit seed fits every descriptor that carries one."""
    from cm3_amd import _lib
    text = open(os.path.join(ROOT, "include", "cm3_amd.h")).read()
    for struct, ctype, cls in (("cm3_actor_rows", "int64_t", _lib.ActorRows), ("cm3_actor_checkers_rows", "uint64_t", _lib.ActorCheckersRows)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % struct, text).group(1)
        assert re.search(r"\b%s\s+row_id_base;" % ctype, body), struct
        assert re.search(r"\buint32_t\s+draw;", body), struct
        fields = dict(cls._fields_)
        assert fields["row_id_base"] is (ctypes.c_int64 if ctype == "int64_t" else ctypes.c_uint64), struct
        assert fields["draw"] is ctypes.c_uint32 and fields["n_rows"] is ctypes.c_int64, struct
    for cls in (_lib.ParticleDesc, _lib.CheckersDesc, _lib.ActorParticleDesc, _lib.ActorCheckersDesc):
        fields = dict(cls._fields_)
        assert fields["seed"] is ctypes.c_uint64 and fields["env_id_base"] is ctypes.c_int64, cls.__name__
        d = cls()
        d.seed, d.env_id_base = 0x9E3779B97F4A7C15, (5 << 32) - 19
        assert (d.seed, d.env_id_base) == (0x9E3779B97F4A7C15, (5 << 32) - 19), cls.__name__


def test_particle_rows_wrapper_refuses_a_base_outside_int64():
    """The wrapper hands row_id_base to an int64_t field: every value of that type passes unchanged (the kernel reads it as the
    64-bit pattern, as tests/actor_rows_ref.py does), a value from 2^63 on is refused instead of being wrapped without a word."""
    from cm3_amd import Cm3Error
    from cm3_amd import _lib
    from cm3_amd.actor import rows_id_base_i64
    for ok in (0, 5, (5 << 32) - 19, (1 << 63) - 1, -1, -(1 << 63)):
        r = _lib.ActorRows()
        r.row_id_base = rows_id_base_i64(ok)
        assert r.row_id_base == ok
        assert np.array_equal(RR.rows_uniforms(7, 3, 0, row_id_base=ok), RR.rows_uniforms(7, 3, 0, row_id_base=ok & ((1 << 64) - 1)))
    for bad in (1 << 63, (1 << 63) + 11, (1 << 64) - 1, -(1 << 63) - 1):
        with pytest.raises(Cm3Error, match="row_id_base"):
            rows_id_base_i64(bad)
    c = _lib.ActorCheckersRows()
    c.row_id_base = (1 << 63) + 11                                           # the Checkers twin is unsigned: nothing to refuse
    assert c.row_id_base == (1 << 63) + 11
