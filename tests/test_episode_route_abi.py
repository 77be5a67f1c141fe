"""CPU: the C ABI of the whole-episode dual replay path (cm3_episode_route_plan / _scratch_bytes / _plan_host and
cm3_transitions_route_f32, additive in ABI 9) -- declared, exported, bound, the descriptor laid out as a C compiler sees it, every
invalid argument refused with a readable error before anything touches a GPU, and the host entry equal to the model."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.dual_ref import DualModel, crafted_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cm3_episode_route_scratch_bytes", "cm3_episode_route_plan", "cm3_episode_route_plan_host", "cm3_transitions_route_f32")
FAKE = 0x1000                                   # never dereferenced: validation fails first
FIELDS = ("done", "collisions", "valid", "done_stride", "collisions_stride", "valid_stride", "n_ticks", "n_envs", "pending_depth",
          "synchronous", "ring_idx", "ring_size")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    return _lib


def test_header_declares_and_library_exports_the_entries(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cm3_amd.h")).read(), flags=re.S)
    handle = built.lib()
    for entry in ENTRIES:
        assert re.search(r"\b%s\s*\(" % entry, text), entry
        assert hasattr(handle, entry) and entry in built.SYMBOLS, entry
    assert "cm3_episode_route_desc" in text and not re.search(r"struct\s+cm3_episode_route_desc", text)      # untagged
    assert built.ABI_VERSION == 9 and handle.cm3_abi_version() == 9
    assert (built.ROUTE_BAD, built.ROUTE_GOOD, built.ROUTE_PENDING, built.ROUTE_SKIP) == tuple(
        int(re.search(r"#define CM3_ROUTE_%s (\d+)" % n, text).group(1)) for n in ("BAD", "GOOD", "PENDING", "SKIP"))


def test_descriptor_layout_is_the_c_compilers(built, tmp_path):
    cls = built.EpisodeRouteDesc
    assert tuple(n for n, _ in cls._fields_) == FIELDS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cm3_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(cm3_episode_route_desc));']
    for name in FIELDS:
        lines.append('  printf("%s %%zu\\n", offsetof(cm3_episode_route_desc, %s));' % (name, name))
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for name in FIELDS:
        assert getattr(cls, name).offset == int(got[name]), name


def _desc(built, **kw):
    d = built.EpisodeRouteDesc()
    d.done, d.collisions, d.done_stride, d.collisions_stride = FAKE, FAKE, 70, 280
    d.n_ticks, d.n_envs, d.pending_depth, d.synchronous = 7, 70, 5, 0
    d.ring_idx[0], d.ring_idx[1], d.ring_size[0], d.ring_size[1] = 3, 0, 37, 600
    for k, v in kw.items():
        if k in ("ring_idx", "ring_size"):
            getattr(d, k)[0], getattr(d, k)[1] = v
        else:
            setattr(d, k, v)
    return d


def _plan(built, desc="ok", scratch=FAKE, scratch_bytes=1 << 20, **ptrs):
    a = dict(pend_in=FAKE, pend_out=FAKE, sel=FAKE, row=FAKE, flush_row=FAKE, counts=FAKE)
    a.update(ptrs)
    d = _desc(built) if isinstance(desc, str) else desc
    handle = built.lib()
    rc = handle.cm3_episode_route_plan(None if d is None else ctypes.byref(d), a["pend_in"], a["pend_out"], a["sel"], a["row"],
                                       a["flush_row"], a["counts"], scratch, scratch_bytes, None)
    return rc, handle.cm3_last_error()


def test_plan_refuses_null_negative_and_oversize_arguments_without_a_gpu(built):
    cases = [
        (dict(desc=None), b"null desc"),
        (dict(desc=_desc(built, done=None)), b"done and collisions"), (dict(desc=_desc(built, collisions=None)), b"done and collisions"),
        (dict(desc=_desc(built, n_ticks=0)), b"below 2^31"), (dict(desc=_desc(built, n_envs=-1)), b"below 2^31"),
        (dict(desc=_desc(built, pending_depth=-1)), b"below 2^31"),
        (dict(desc=_desc(built, n_ticks=1 << 16, n_envs=1 << 15, done_stride=1 << 15, collisions_stride=1 << 17)), b"below 2^31"),
        (dict(desc=_desc(built, n_envs=1 << 20, pending_depth=2041, done_stride=1 << 20, collisions_stride=1 << 22)), b"below 2^31"),
        (dict(desc=_desc(built, done_stride=69)), b"tick stride"), (dict(desc=_desc(built, collisions_stride=276)), b"tick stride"),
        (dict(desc=_desc(built, valid=FAKE, valid_stride=10)), b"tick stride"),
        (dict(desc=_desc(built, ring_size=(0, 600))), b"ring 0"), (dict(desc=_desc(built, ring_idx=(37, 0))), b"ring 0"),
        (dict(desc=_desc(built, ring_idx=(0, -1))), b"ring 1"),
        (dict(sel=None), b"sel, row and counts"), (dict(row=None), b"sel, row and counts"), (dict(counts=None), b"sel, row and counts"),
        (dict(flush_row=None), b"flush_row"), (dict(pend_in=None), b"pend_len"), (dict(pend_out=None), b"pend_len"),
        (dict(scratch=None), b"scratch"), (dict(scratch=FAKE + 4), b"scratch"), (dict(scratch_bytes=7 * 70 * 16), b"scratch"),
    ]
    for kw, needle in cases:
        rc, err = _plan(built, **kw)
        assert rc == -1 and needle in err, (kw, err)
    handle = built.lib()
    assert handle.cm3_episode_route_scratch_bytes(7, 70) == (2 * 490 + 1) * 8
    assert handle.cm3_episode_route_scratch_bytes(0, 70) == 0 and handle.cm3_episode_route_scratch_bytes(1 << 16, 1 << 15) == 0


def _route(built, n=140, n_sets=3, sel=FAKE, row=FAKE, desc="ok", traj="ok", sets="ok"):
    handle = built.lib()
    d = built.ParticleDesc()
    d.n_envs, d.n_agents = 70, 4
    t = built.ParticleTraj()
    for name, kind in t._fields_:
        setattr(t, name, FAKE if kind is ctypes.c_void_p else 1024)
    s = (built.TransitionCols * 3)()
    for k in range(3):
        for name, kind in s[k]._fields_:
            if kind is ctypes.c_void_p:
                setattr(s[k], name, FAKE)
    if callable(desc):
        desc(d)
    if callable(traj):
        traj(t)
    if callable(sets):
        sets(s)
    rc = handle.cm3_transitions_route_f32(None if desc is None else ctypes.byref(d), None if traj is None else ctypes.byref(t), None, 0,
                                          n, sel, row, None if sets is None else s, n_sets, None)
    return rc, handle.cm3_last_error()


def test_routed_export_refuses_bad_arguments_without_a_gpu(built):
    for kw, needle in [
            (dict(desc=None), b"null argument"), (dict(traj=None), b"null argument"), (dict(sets=None), b"null argument"),
            (dict(n=-1), b"n must be >= 0"), (dict(n_sets=0), b"1..3 column sets"), (dict(n_sets=4), b"1..3 column sets"),
            (dict(sel=None), b"sel and row"), (dict(row=None), b"sel and row"), (dict(n=141), b"whole ticks"),
            (dict(desc=lambda d: setattr(d, "n_agents", 11)), b"n_agents"),
            (dict(traj=lambda t: setattr(t, "state", None)), b"trajectory base pointers"),
            (dict(traj=lambda t: setattr(t, "term_state", None)), b"both or neither"),
            (dict(sets=lambda s: setattr(s[2], "goals", None)), b"column set 2"),
            (dict(sets=lambda s: setattr(s[1], "state", FAKE + 8)), b"column set 1 is not aligned")]:
        rc, err = _route(built, **kw)
        assert rc == -1 and needle in err, (kw, err)
    assert _route(built, n=0, sel=None, row=None)[0] == 0                   # an empty chunk touches nothing


def test_host_entry_equals_the_model(built):
    """cm3_episode_route_plan_host: the header's sequential function behind the library's validation, on host arrays."""
    E, T, P, sizes = 70, 7, 12, (37, 600)
    done, coll = crafted_chunks(E, T, P, 3, seed=12)
    model = DualModel(sizes, E, P)
    pend = np.zeros(E, np.int32)
    handle = built.lib()
    for c in range(3):
        d_, c_ = np.ascontiguousarray(done[c * T:(c + 1) * T]), np.ascontiguousarray(coll[c * T:(c + 1) * T])
        want = model.add_chunk(d_, c_)
        desc = _desc(built, done=d_.ctypes.data, collisions=c_.ctypes.data, pending_depth=P, ring_idx=tuple(want["idx"]), ring_size=sizes)
        sel, row = np.empty(T * E, np.uint8), np.empty(T * E, np.int64)
        flush, counts = np.empty((2, P * E), np.int64), np.empty(2, np.int64)
        rc = handle.cm3_episode_route_plan_host(ctypes.byref(desc), pend.ctypes.data, pend.ctypes.data, sel.ctypes.data, row.ctypes.data,
                                                flush.ctypes.data, counts.ctypes.data)
        assert rc == 0, handle.cm3_last_error()
        for k, got in (("sel", sel), ("row", row), ("flush_row", flush), ("counts", counts), ("pend_len", pend)):
            assert np.array_equal(got, want[k]), (c, k)


def test_classes_carry_the_surface():
    from cm3_amd.replay import DeviceDualReplayBuffer, off_policy_batches
    from cm3_amd.rollout import ParticleRollout
    import inspect
    for name in ("add_rollout", "pending", "drop_pending", "add", "sample_batch"):
        assert hasattr(DeviceDualReplayBuffer, name), name
    assert hasattr(ParticleRollout, "route_into")
    assert inspect.signature(off_policy_batches).parameters["whole_episodes"].default is False
