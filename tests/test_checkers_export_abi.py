"""CPU: the C ABI of the one-launch Checkers transition export (cm3_checkers_transitions_gather, additive in ABI 9) -- declared,
exported, bound, its struct laid out as a C compiler sees it, and every invalid argument refused with a readable error before
anything touches a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "cm3_checkers_transitions_gather"
FAKE = 0x1000                                   # never dereferenced: validation fails first
COLUMNS = ("grid", "vec", "obs_others", "obs_self_t", "obs_self_v", "actions_prev", "actions", "reward", "local_rewards",
           "next_grid", "next_vec", "next_obs_others", "next_obs_self_t", "next_obs_self_v", "done", "goals")


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
    assert "cm3_checkers_transition_cols" in text
    assert hasattr(handle, ENTRY)
    assert ENTRY in built.SYMBOLS
    assert built.ABI_VERSION == 9 and handle.cm3_abi_version() == 9


def test_struct_is_sixteen_pointers_and_two_int64_in_the_order_of_the_columns(built, tmp_path):
    cls = built.CheckersTransitionCols
    assert ctypes.sizeof(cls) == 16 * ctypes.sizeof(ctypes.c_void_p) + 2 * 8
    from cm3_amd.rollout import CheckersRollout
    assert tuple(n for n, _ in cls._fields_) == COLUMNS + ("ring_start", "ring_size") and CheckersRollout.ORDER == COLUMNS
    # sizeof and every field offset as a C compiler sees the header
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cm3_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(cm3_checkers_transition_cols));']
    for name, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(cm3_checkers_transition_cols, %s));' % (name, name))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for name, _ in cls._fields_:
        assert getattr(cls, name).offset == int(got[name]), name


def _desc(built, **kw):
    d = built.CheckersDesc()
    d.n_envs, d.n_agents, d.n_rows, d.n_columns, d.n_obs, d.max_steps = 16, 2, 3, 8, 2, 33
    d.grid_stride, d.obs_self_t_stride = 56, 152
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _traj(built, **kw):
    t = built.CheckersTraj()
    for name, kind in t._fields_:
        setattr(t, name, FAKE if kind is ctypes.c_void_p else 1024)
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _cols(built, **kw):
    c = built.CheckersTransitionCols()
    for name in COLUMNS:
        setattr(c, name, FAKE)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _call(built, desc="ok", traj="ok", prev0=FAKE, tt=None, ee=None, n=4, cols="ok"):
    handle = built.lib()
    byref = lambda x, make: ctypes.byref(make(built)) if isinstance(x, str) else (None if x is None else ctypes.byref(x))  # noqa: E731
    rc = handle.cm3_checkers_transitions_gather(byref(desc, _desc), byref(traj, _traj), prev0, tt, ee, n, byref(cols, _cols), None)
    return rc, handle.cm3_last_error()


@pytest.mark.parametrize("kw,needle", [
    (dict(desc=None), b"null desc"), (dict(traj=None), b"null traj"), (dict(cols=None), b"null out"),
    (dict(tt=FAKE), b"tt and ee"), (dict(ee=FAKE), b"tt and ee"),
    (dict(n=-1), b"n must be >= 0")])
def test_null_and_count_arguments_are_refused_without_a_gpu(built, kw, needle):
    rc, err = _call(built, **kw)
    assert rc == -1 and needle in err, err


def test_ring_arguments_are_refused_without_a_gpu(built):
    for ring in (dict(ring_size=-1), dict(ring_size=3, ring_start=0), dict(ring_size=8, ring_start=8), dict(ring_size=8, ring_start=-1),
                 dict(ring_size=0, ring_start=-1)):
        rc, err = _call(built, n=4, cols=_cols(built, **ring))
        assert rc == -1 and b"ring_start / ring_size" in err, (ring, err)


@pytest.mark.parametrize("name", COLUMNS)
def test_a_missing_column_is_refused_by_name(built, name):
    rc, err = _call(built, cols=_cols(built, **{name: None}))
    assert rc == -1 and b"column %s is missing" % name.encode() in err, err


def test_trajectory_and_geometry_are_checked_before_the_launch(built):
    for field in ("actions", "grid", "vec", "obs_others", "obs_self_t", "obs_self_v", "local_rewards", "reward", "done"):
        rc, err = _call(built, traj=_traj(built, **{field: None}))
        assert rc == -1 and b"trajectory base pointers" in err, (field, err)
    rc, err = _call(built, traj=_traj(built, goals=None, goals_slots=None))
    assert rc == -1 and b"trajectory base pointers" in err
    rc, err = _call(built, traj=_traj(built, term_vec=None))
    assert rc == -1 and b"all five" in err
    rc, err = _call(built, prev0=None)
    assert rc == -1 and b"prev0" in err
    for kw, needle in ((dict(n_agents=0), b"n_agents"), (dict(n_agents=9), b"n_agents"), (dict(n_envs=0), b"n_envs"),
                       (dict(n_obs=9), b"n_obs"), (dict(grid_stride=50), b"record strides"), (dict(obs_self_t_stride=149), b"record strides")):
        rc, err = _call(built, desc=_desc(built, **kw))
        assert rc == -1 and needle in err, (kw, err)
    rc, err = _call(built, cols=_cols(built, grid=FAKE + 8))
    assert rc == -1 and b"not aligned" in err


def test_an_empty_batch_touches_nothing(built):
    empty = built.CheckersTransitionCols()                  # (the columns of an empty batch are null)
    rc, _ = _call(built, n=0, cols=empty, traj=built.CheckersTraj(), prev0=None)
    assert rc == 0
    rc, _ = _call(built, n=0, tt=FAKE, ee=FAKE, cols=empty)
    assert rc == 0


def test_rollout_and_buffer_carry_the_surface():
    from cm3_amd.replay import DeviceReplayBuffer
    from cm3_amd.rollout import CheckersRollout, ParticleRollout
    for name in ("export_into", "sample_batch", "on_policy_minibatches", "as_reference_batch_torch", "last_sample_positions"):
        assert hasattr(CheckersRollout, name), name
    # one implementation of the sampling side for both env families
    for name in ("_sample_positions", "_phase_export", "sample_batch", "on_policy_minibatches"):
        assert getattr(CheckersRollout, name) is getattr(ParticleRollout, name), name
    assert hasattr(DeviceReplayBuffer, "add_rollout")
