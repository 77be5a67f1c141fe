"""CPU: the C ABI of the QMIX train-step data side (part of ABI 9, additive) -- cm3_qmix_particle_rows_f32 and
cm3_qmix_td_target_f64 declared, exported, bound; the cm3_qmix_rows layout as a C compiler sees it; every invalid argument
refused with a readable error before anything touches a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cm3_qmix_particle_rows_f32", "cm3_qmix_td_target_f64")
FAKE = 0x1000                                      # 16-byte aligned, never dereferenced: validation fails first


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


def test_rows_struct_layout_matches_the_header(built, tmp_path):
    """sizeof and every field offset of cm3_qmix_rows (an anonymous-tag struct), as a C compiler sees include/cm3_amd.h, against
    the ctypes mirror."""
    cls = built.QmixRows
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cm3_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(cm3_qmix_rows));']
    for fname, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(cm3_qmix_rows, %s));' % (fname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert ctypes.sizeof(cls) == got["size"] == 64
    assert [f for f, _ in cls._fields_] == ["obs_others", "v_obs", "goals", "q", "argmax", "onehot", "q_max", "n_rows"]
    for fname, _ in cls._fields_:
        assert getattr(cls, fname).offset == got[fname], fname
    text = open(os.path.join(ROOT, "include", "cm3_amd.h")).read()
    assert not re.search(r"typedef struct cm3_qmix_rows", text)          # (anonymous tag: tests/test_abi.py's table stays as it is)


def _desc(built, **kw):
    d = built.ActorParticleDesc()
    d.n_envs, d.n_agents, d.stage = 0, 4, 2                              # n_envs, epsilon, seed, env_id_base: not read
    d.n_h1_self, d.n_h1_others, d.n_h2, d.n_actions = 64, 0, 64, 5
    d.epsilon, d.precision = 7.0, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _rows(built, **kw):
    r = built.QmixRows()
    r.obs_others, r.v_obs, r.goals, r.argmax, r.n_rows = FAKE, FAKE, FAKE, FAKE, 100
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _refused(built, needle, desc="default", packed=FAKE, rows="default"):
    handle = built.lib()
    d = _desc(built) if desc == "default" else desc
    r = _rows(built) if rows == "default" else rows
    rc = handle.cm3_qmix_particle_rows_f32(None if d is None else ctypes.byref(d), packed, None if r is None else ctypes.byref(r), None)
    assert rc == -1
    assert needle in handle.cm3_last_error(), handle.cm3_last_error()


@pytest.mark.parametrize("field,value,needle", [
    ("n_agents", 0, b"n_agents"), ("n_agents", 11, b"n_agents"), ("n_h1_self", 128, b"64/64/5"), ("n_h2", 32, b"64/64/5"),
    ("n_actions", 4, b"64/64/5"), ("precision", 2, b"precision")])
def test_rows_invalid_descriptor_is_refused_without_a_gpu(built, field, value, needle):
    _refused(built, needle, desc=_desc(built, **{field: value}))


def test_rows_null_arguments_are_refused(built):
    _refused(built, b"null desc", desc=None)
    _refused(built, b"packed", packed=None)
    _refused(built, b"null rows", rows=None)


@pytest.mark.parametrize("name", ["obs_others", "v_obs", "goals"])
def test_rows_missing_input_is_refused(built, name):
    _refused(built, b"missing inputs", rows=_rows(built, **{name: None}))


def test_rows_without_an_output_are_refused(built):
    _refused(built, b"no output requested", rows=_rows(built, argmax=None))
    for name in ("q", "onehot", "q_max"):                                  # any single output is enough to pass THIS check
        handle = built.lib()
        r = _rows(built, argmax=None, n_rows=0, **{name: FAKE})
        assert handle.cm3_qmix_particle_rows_f32(ctypes.byref(_desc(built)), FAKE, ctypes.byref(r), None) == -1
        assert b"n_rows" in handle.cm3_last_error()


@pytest.mark.parametrize("n_rows", [0, -1, 64 * (2 ** 31 - 1) + 1])
def test_rows_count_out_of_range_is_refused(built, n_rows):
    _refused(built, b"n_rows", rows=_rows(built, n_rows=n_rows))


@pytest.mark.parametrize("name,value,needle", [
    ("obs_others", FAKE + 8, b"misaligned inputs"), ("v_obs", FAKE + 4, b"misaligned inputs"), ("goals", FAKE + 4, b"misaligned inputs"),
    ("onehot", FAKE + 8, b"misaligned onehot")])
def test_rows_misaligned_pointer_is_refused(built, name, value, needle):
    _refused(built, needle, rows=_rows(built, **{name: value}))


@pytest.mark.parametrize("desc_kw,packed,rows_kw,needle", [
    ({"n_h2": 32, "precision": 2}, FAKE, {}, b"64/64/5"),
    ({"precision": 2}, None, {}, b"precision must be 0"),
    ({}, None, None, b"packed weights are NULL"),
    ({}, FAKE, {"goals": None, "argmax": None}, b"missing inputs"),
    ({}, FAKE, {"argmax": None, "n_rows": 0}, b"no output requested"),
    ({}, FAKE, {"n_rows": 0, "v_obs": FAKE + 4}, b"n_rows must be positive"),
    ({}, FAKE, {"n_rows": 64 * (2 ** 31 - 1) + 1, "v_obs": FAKE + 4}, b"more than a grid"),
    ({}, FAKE, {"v_obs": FAKE + 4, "onehot": FAKE + 8}, b"misaligned inputs")])
def test_rows_checks_fire_in_their_order(built, desc_kw, packed, rows_kw, needle):
    """Two consecutive checks violated at once: the earlier one's message is the one reported."""
    _refused(built, needle, desc=_desc(built, **desc_kw), packed=packed, rows=None if rows_kw is None else _rows(built, **rows_kw))


def test_td_target_validates_before_launching(built):
    handle = built.lib()
    fn = handle.cm3_qmix_td_target_f64
    assert fn(FAKE, 0, 4, FAKE, 0, FAKE, 0.99, FAKE, -1, None) == -1
    assert b"n must be" in handle.cm3_last_error()
    for n_agents in (0, 11):
        assert fn(FAKE, 0, n_agents, FAKE, 0, FAKE, 0.99, FAKE, 8, None) == -1
        assert b"n_agents" in handle.cm3_last_error()
    for hole in (0, 3, 5, 7):
        args = [FAKE, 0, 4, FAKE, 0, FAKE, 0.99, FAKE, 8, None]
        args[hole] = None
        assert fn(*args) == -1, hole
        assert b"null argument" in handle.cm3_last_error()
    assert fn(None, 0, 4, None, 0, None, 0.99, None, 0, None) == 0          # nothing to do: no launch, no error


def test_soft_update_and_greedy_rows_exist_on_the_agent():
    from cm3_amd.qmix import ParticleQmixAgent
    assert callable(ParticleQmixAgent.greedy_rows) and callable(ParticleQmixAgent.soft_update_from)
