"""CPU: the C ABI of the compact Checkers replay ring (cm3_checkers_transitions_pack / cm3_checkers_ring_expand, additive in ABI 9) --
declared, exported, bound, the new struct laid out as a C compiler sees it, and every invalid argument refused with a readable error
before anything touches a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACK, EXPAND = "cm3_checkers_transitions_pack", "cm3_checkers_ring_expand"
FAKE = 0x1000                                   # never dereferenced: validation fails first
COLUMNS = ("grid", "vec", "obs_others", "obs_self_t", "obs_self_v", "actions_prev", "actions", "reward", "local_rewards",
           "next_grid", "next_vec", "next_obs_others", "next_obs_self_t", "next_obs_self_v", "done", "goals")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    return _lib


def test_header_declares_and_library_exports_both_entries(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cm3_amd.h")).read(), flags=re.S)
    handle = built.lib()
    for entry in (PACK, EXPAND):
        assert re.search(r"\b%s\s*\(" % entry, text), entry
        assert hasattr(handle, entry), entry
        assert entry in built.SYMBOLS, entry
    assert "cm3_checkers_compact_cols" in text
    assert built.ABI_VERSION == 9 and handle.cm3_abi_version() == 9


def test_compact_struct_is_sixteen_pointers_and_two_int64_in_the_order_of_the_columns(built, tmp_path):
    cls = built.CheckersCompactCols
    assert ctypes.sizeof(cls) == 16 * ctypes.sizeof(ctypes.c_void_p) + 2 * 8
    from cm3_amd.rollout import CheckersRollout
    assert tuple(n for n, _ in cls._fields_) == COLUMNS + ("ring_start", "ring_size") and CheckersRollout.ORDER == COLUMNS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cm3_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(cm3_checkers_compact_cols));']
    for name, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(cm3_checkers_compact_cols, %s));' % (name, name))
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
    d.n_envs, d.n_agents, d.n_rows, d.n_columns, d.n_obs, d.max_steps = 4, 2, 3, 8, 2, 33
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


def _compact(built, **kw):
    c = built.CheckersCompactCols()
    for name in COLUMNS:
        setattr(c, name, FAKE)
    c.ring_start, c.ring_size = 0, 8
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _wide(built, **kw):
    c = built.CheckersTransitionCols()
    for name in COLUMNS:
        setattr(c, name, FAKE)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _ref(x, make, built):
    return ctypes.byref(make(built)) if isinstance(x, str) else (None if x is None else ctypes.byref(x))


def _pack(built, desc="ok", traj="ok", prev0=FAKE, n=4, cols="ok"):
    handle = built.lib()
    rc = handle.cm3_checkers_transitions_pack(_ref(desc, _desc, built), _ref(traj, _traj, built), prev0, n, _ref(cols, _compact, built), None)
    return rc, handle.cm3_last_error()


def _expand(built, desc="ok", ring="ok", index=None, n=4, out="ok"):
    handle = built.lib()
    rc = handle.cm3_checkers_ring_expand(_ref(desc, _desc, built), _ref(ring, _compact, built), index, n, _ref(out, _wide, built), None)
    return rc, handle.cm3_last_error()


@pytest.mark.parametrize("kw,needle", [
    (dict(desc=None), b"null desc"), (dict(traj=None), b"null traj"), (dict(cols=None), b"null compact columns"),
    (dict(n=-1), b"n must be >= 0")])
def test_pack_refuses_null_and_count_arguments_without_a_gpu(built, kw, needle):
    rc, err = _pack(built, **kw)
    assert rc == -1 and needle in err, err


@pytest.mark.parametrize("kw,needle", [
    (dict(desc=None), b"null desc"), (dict(ring=None), b"null compact columns"), (dict(out=None), b"null out"),
    (dict(n=-1), b"n must be >= 0")])
def test_expand_refuses_null_and_count_arguments_without_a_gpu(built, kw, needle):
    rc, err = _expand(built, **kw)
    assert rc == -1 and needle in err, err


RINGS = (dict(ring_size=0), dict(ring_size=-1), dict(ring_size=3, ring_start=0), dict(ring_size=8, ring_start=8),
         dict(ring_size=8, ring_start=-1))


def test_ring_arguments_are_refused_without_a_gpu(built):
    for ring in RINGS:                             # (ring_size 3 < n = 4: more transitions than the ring holds)
        rc, err = _pack(built, n=4, cols=_compact(built, **ring))
        assert rc == -1 and b"ring_start / ring_size" in err, (ring, err)
        rc, err = _expand(built, n=4, ring=_compact(built, **ring))
        assert rc == -1 and b"ring_start / ring_size" in err, (ring, err)
    rc, err = _expand(built, n=4, out=_wide(built, ring_size=3))
    assert rc == -1 and b"ring_start / ring_size" in err, err


@pytest.mark.parametrize("name", COLUMNS)
def test_a_missing_column_is_refused_by_name(built, name):
    needle = b"column %s is missing" % name.encode()
    rc, err = _pack(built, cols=_compact(built, **{name: None}))
    assert rc == -1 and needle in err and b"compact" in err, err
    rc, err = _expand(built, ring=_compact(built, **{name: None}))
    assert rc == -1 and needle in err and b"compact" in err, err
    rc, err = _expand(built, out=_wide(built, **{name: None}))
    assert rc == -1 and needle in err and b"compact" not in err, err


def test_alignment_is_checked_by_name(built):
    for name in COLUMNS:                           # the pack kernel stores aligned 16-byte pieces of every column
        rc, err = _pack(built, cols=_compact(built, **{name: FAKE + 8}))
        assert rc == -1 and b"column %s is not aligned" % name.encode() in err, err
    rc, err = _expand(built, out=_wide(built, grid=FAKE + 8))
    assert rc == -1 and b"column grid is not aligned" in err, err
    # the expansion loads vec two int32 at a time, the float64 rows 16 bytes at a time, reward 8, actions 4
    for name, off in (("vec", 4), ("next_vec", 4), ("obs_others", 8), ("next_obs_self_v", 8), ("reward", 4), ("actions", 2), ("actions_prev", 2)):
        rc, err = _expand(built, ring=_compact(built, **{name: FAKE + off}))
        assert rc == -1 and b"%s is not aligned" % name.encode() in err, (name, err)


def test_trajectory_and_geometry_are_checked_before_the_launch(built):
    for field in ("actions", "grid", "vec", "obs_others", "obs_self_t", "obs_self_v", "local_rewards", "reward", "done"):
        rc, err = _pack(built, traj=_traj(built, **{field: None}))
        assert rc == -1 and b"trajectory base pointers" in err, (field, err)
    rc, err = _pack(built, traj=_traj(built, goals=None, goals_slots=None))
    assert rc == -1 and b"trajectory base pointers" in err
    rc, err = _pack(built, traj=_traj(built, term_vec=None))
    assert rc == -1 and b"all five" in err
    rc, err = _pack(built, prev0=None)
    assert rc == -1 and b"prev0" in err
    for kw, needle in ((dict(n_agents=0), b"n_agents"), (dict(n_agents=9), b"n_agents"), (dict(n_obs=9), b"n_obs"),
                       (dict(grid_stride=50), b"record strides"), (dict(obs_self_t_stride=149), b"record strides"),
                       (dict(grid_stride=-1), b"record strides")):
        rc, err = _pack(built, desc=_desc(built, **kw))
        assert rc == -1 and needle in err, (kw, err)
        rc, err = _expand(built, desc=_desc(built, **kw))
        assert rc == -1 and needle in err, (kw, err)
    rc, err = _pack(built, desc=_desc(built, n_envs=0))
    assert rc == -1 and b"n_envs" in err


def test_an_empty_batch_touches_nothing(built):
    empty, out = built.CheckersCompactCols(), built.CheckersTransitionCols()      # (null columns)
    empty.ring_size = 8
    rc, _ = _pack(built, n=0, cols=empty, traj=built.CheckersTraj(), prev0=None)
    assert rc == 0
    rc, _ = _expand(built, n=0, ring=empty, out=out)
    assert rc == 0
    rc, _ = _expand(built, n=0, ring=empty, out=out, index=FAKE)
    assert rc == 0


def test_rollout_and_buffer_carry_the_surface():
    from cm3_amd.replay import CompactCheckersReplayBuffer, DeviceReplayBuffer
    from cm3_amd.rollout import CheckersRollout
    for name in ("compact_column_specs", "pack_into", "column_specs", "export_into"):
        assert hasattr(CheckersRollout, name), name
    for name in ("maxsize", "idx", "len", "__len__", "add_rollout", "add", "sample_batch", "sample_n", "all"):
        assert hasattr(CompactCheckersReplayBuffer, name) and hasattr(DeviceReplayBuffer, name), name
    import inspect
    assert list(inspect.signature(CompactCheckersReplayBuffer.sample_batch).parameters) == ["self", "size", "generator", "out"]


def test_compact_specs_keep_the_dtypes_of_the_trajectory():
    import torch
    from cm3_amd.rollout import compact_specs
    f64 = torch.float64
    wide = dict(grid=((3, 9, 2), f64), vec=((2, 4), f64), obs_others=((2, 2), f64), obs_self_t=((2, 5, 5, 3), f64),
                obs_self_v=((2, 4), f64), actions_prev=((2,), torch.int32), actions=((2,), torch.int32), reward=((), f64),
                local_rewards=((2,), f64), done=((), torch.bool), goals=((2, 2), torch.int64))
    wide.update({"next_" + k: wide[k] for k in ("grid", "vec", "obs_others", "obs_self_t", "obs_self_v")})
    got = compact_specs({k: wide[k] for k in COLUMNS})
    assert tuple(got) == COLUMNS
    assert got["grid"] == got["next_grid"] == ((3, 9, 2), torch.int8)
    assert got["obs_self_t"] == got["next_obs_self_t"] == ((2, 5, 5, 3), torch.int8)
    assert got["vec"] == got["next_vec"] == ((2, 4), torch.int32) and got["goals"] == ((2,), torch.uint8)
    for name in ("obs_others", "obs_self_v", "actions_prev", "actions", "reward", "local_rewards", "done", "next_obs_others"):
        assert got[name] == wide[name], name
    row = sum(torch.empty(s, dtype=d).numel() * torch.empty((), dtype=d).element_size() for s, d in got.values())
    assert row == 707                              # bytes per transition at the reference geometry, N = 2
