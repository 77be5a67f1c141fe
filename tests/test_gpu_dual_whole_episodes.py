"""GPU: whole episodes into the dual replay buffer -- the routing plan kernels (csrc/episode_route.hip) against the header's host
function and the host model of tests/dual_ref.py, the routed export launch (cm3_transitions_route_f32) on a synthetic trajectory, and
DeviceDualReplayBuffer.add_rollout end to end in both collection modes."""
import ctypes

import numpy as np
import pytest
import torch

from tests.dual_ref import DualModel, crafted_chunks, crafted_sync
from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E70, T7 = 70, 7


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _plan_both(done, coll, valid, pend, P, sync, idx, sizes):
    """One chunk through cm3_episode_route_plan (device tensors) and cm3_episode_route_plan_host (host arrays) -> (device, host)"""
    from cm3_amd import _lib
    handle = _lib.lib()
    T, E = done.shape
    done, coll = np.ascontiguousarray(done, np.uint8), np.ascontiguousarray(coll, np.int32)
    valid = None if valid is None else np.ascontiguousarray(valid, np.uint8)

    def desc(d_ptr, c_ptr, v_ptr):
        d = _lib.EpisodeRouteDesc()
        d.done, d.collisions, d.valid = d_ptr, c_ptr, v_ptr
        d.done_stride, d.collisions_stride, d.valid_stride = E, 4 * E, E
        d.n_ticks, d.n_envs, d.pending_depth, d.synchronous = T, E, P, int(sync)
        d.ring_idx[0], d.ring_idx[1], d.ring_size[0], d.ring_size[1] = idx[0], idx[1], sizes[0], sizes[1]
        return d
    # host
    h = dict(sel=np.empty(T * E, np.uint8), row=np.empty(T * E, np.int64), flush_row=np.full((2, max(P, 1) * E), -1, np.int64),
             counts=np.empty(2, np.int64), pend_len=np.array(pend, np.int32))
    hd = desc(done.ctypes.data, coll.ctypes.data, None if valid is None else valid.ctypes.data)
    rc = handle.cm3_episode_route_plan_host(ctypes.byref(hd), h["pend_len"].ctypes.data, h["pend_len"].ctypes.data, h["sel"].ctypes.data,
                                            h["row"].ctypes.data, h["flush_row"].ctypes.data, h["counts"].ctypes.data)
    assert rc == 0, handle.cm3_last_error()
    # device: pend_in and pend_out apart, as DeviceDualReplayBuffer passes them
    g = dict(done=_dev(done), coll=_dev(coll), valid=None if valid is None else _dev(valid), pend_in=_dev(np.array(pend, np.int32)),
             pend_len=torch.zeros(E, dtype=torch.int32, device=DEV), sel=torch.empty(T * E, dtype=torch.uint8, device=DEV),
             row=torch.empty(T * E, dtype=torch.int64, device=DEV), flush_row=torch.full((2, max(P, 1) * E), -1, dtype=torch.int64, device=DEV),
             counts=torch.empty(2, dtype=torch.int64, device=DEV))
    nbytes = handle.cm3_episode_route_scratch_bytes(T, E)
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    gd = desc(g["done"].data_ptr(), g["coll"].data_ptr(), _lib.ptr(g["valid"]))
    _lib.check(handle.cm3_episode_route_plan(ctypes.byref(gd), g["pend_in"].data_ptr(), g["pend_len"].data_ptr(), g["sel"].data_ptr(),
                                             g["row"].data_ptr(), g["flush_row"].data_ptr(), g["counts"].data_ptr(), scratch.data_ptr(),
                                             nbytes, torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return {k: g[k].cpu().numpy() for k in h}, h


@pytest.mark.parametrize("P", [5, 12])
def test_plan_kernels_equal_the_host_function_on_three_chained_chunks(P):
    sizes = (37, 600)
    done, coll = crafted_chunks(E70, T7, P, 3, seed=P)
    model = DualModel(sizes, E70, P)
    pend = np.zeros(E70, np.int32)
    for c in range(3):
        sl = slice(c * T7, (c + 1) * T7)
        want = model.add_chunk(done[sl], coll[sl])
        dev, host = _plan_both(done[sl], coll[sl], None, pend, P, False, want["idx"], sizes)
        for k in ("sel", "row", "flush_row", "counts", "pend_len"):
            assert np.array_equal(dev[k], host[k]), (c, k)          # element for element
            assert np.array_equal(dev[k], want[k]), (c, k, "model")
        pend = dev["pend_len"]
    assert {"several ends of both classes at one tick", "one boundary", "two ends in one chunk", "wrap", "more than a ring holds",
            "pending row overwritten by the call that flushes it"} <= model.seen
    assert ("two boundaries" in model.seen) == (P == 12)


def test_plan_kernels_synchronous_and_more_than_one_scan_block():
    done, coll, valid = crafted_sync(E70, T7, seed=3)
    model = DualModel((50, 1000), E70, 0)
    model.rings[0].plan_add(45)
    want = model.add_chunk(done, coll, valid, sync=True)
    dev, host = _plan_both(done, coll, valid, np.zeros(E70), 0, True, want["idx"], (50, 1000))
    for k in ("sel", "row", "counts"):
        assert np.array_equal(dev[k], host[k]) and np.array_equal(dev[k], want[k]), k
    # 9 x 333 = 2997 cells: three workgroups of the scan launches, the last one partly filled, 6 waves of walkers
    E, T, P, sizes = 333, 9, 9, (700, 5000)
    done, coll = crafted_chunks(E, T, P, 2, seed=1)
    model, pend = DualModel(sizes, E, P), np.zeros(E, np.int32)
    for c in range(2):
        sl = slice(c * T, (c + 1) * T)
        want = model.add_chunk(done[sl], coll[sl])
        dev, host = _plan_both(done[sl], coll[sl], None, pend, P, False, want["idx"], sizes)
        for k in ("sel", "row", "flush_row", "counts", "pend_len"):
            assert np.array_equal(dev[k], host[k]) and np.array_equal(dev[k], want[k]), (c, k)
        pend = dev["pend_len"]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_holds(cols, tokens, wants, what):
    """cols: the columns of a ring / the pending store; tokens int64 [rows] (-1: never written); wants: the reference rows of
    all chunks back to back (token = its row there).  Bit for bit; rows never written are zero."""
    tok = _dev(tokens.reshape(-1))
    for name, have in cols.items():
        w = wants[name][tok.clamp(min=0)]
        mask = (tok >= 0).view((-1,) + (1,) * (w.dim() - 1))
        w = torch.where(mask, w, torch.zeros_like(w))
        assert have.dtype == w.dtype and torch.equal(_bits(have), _bits(w)), (what, name)


def _env(E, n=4, max_steps=33, auto_reset=True, seed=11):
    from cm3_amd.particle import VecParticleEnv
    return VecParticleEnv(load_cfg("particle_stage2_cross.json"), n, 0.2, max_steps, E, device=DEV, dtype=torch.float32,
                          auto_reset=auto_reset, seed=seed)


@pytest.mark.parametrize("N", [1, 2, 4])
def test_routed_export_of_a_synthetic_trajectory(N):
    """Every float of the trajectory a distinct integer (chunk, array, position): terminal capture and sparse goal slots on; after
    three chunks both rings and the pending store hold exactly what the model holds."""
    from cm3_amd.replay import DeviceDualReplayBuffer
    from cm3_amd.rollout import ParticleRollout
    P, sizes = 12, (37, 1200)            # (the bad ring wraps and overflows; the good ring keeps rows that are never written)
    env = _env(E70, N, max_steps=P)
    ro = ParticleRollout(env, n_ticks=T7, use_graph=False)
    assert ro.term_state is not None
    done, coll = crafted_chunks(E70, T7, P, 3, seed=12)
    dual = DeviceDualReplayBuffer(size=sizes[1], device=DEV)
    dual.mem1 = type(dual.mem1)(sizes[0], DEV)
    model = DualModel(sizes, E70, P)
    wants = []
    tt = torch.arange(T7, device=DEV).repeat_interleave(E70)
    ee = torch.arange(E70, device=DEV).repeat(T7)
    for c in range(3):
        for k, name in enumerate(("state", "obs_others", "reward", "reward_n", "term_state", "term_obs_others", "_goals_buf")):
            a = getattr(ro, name)
            a.copy_((torch.arange(a.numel(), device=DEV) + (10 * c + k) * (1 << 19)).to(torch.float32).view_as(a))
            assert a.numel() < (1 << 19)
        ro.actions.copy_(torch.arange(ro.actions.numel(), device=DEV).view_as(ro.actions) * 3 + c)
        ro.done.copy_(_dev(done[c * T7:(c + 1) * T7]))
        ro.collisions.copy_(_dev(coll[c * T7:(c + 1) * T7]))
        ro._goals_sparse, ro._goal_src, ro._goal_src32, ro.collected = True, None, None, True
        model.add_chunk(done[c * T7:(c + 1) * T7], coll[c * T7:(c + 1) * T7])
        wants.append(ro.as_reference_batch_torch(tt, ee, numpy=False))
        dual.add_rollout(ro)
        assert (dual.mem1.idx, dual.mem1.len, dual.mem2.idx, dual.mem2.len) == (
            model.rings[0].idx, model.rings[0].len, model.rings[1].idx, model.rings[1].len)
        assert dual.pending == model.pending
    wants = {k: torch.cat([w[k] for w in wants]).contiguous() for k in wants[0]}
    _assert_holds(dual.mem1.cols, model.mem[0], wants, "memory_1")
    _assert_holds(dual.mem2.cols, model.mem[1], wants, "memory_2")
    _assert_holds(dual._carry["store"], model.pend, wants, "pending store")
    assert (model.mem[1] < 0).any() and (model.pend < 0).any()            # (rows never written exist, and stayed zero)
    assert dual.mem1.cols["v_local"].data_ptr() == dual.mem1.cols["v_global"].data_ptr()


def _contiguous_in_time_order(model, c):
    """every episode of class c whose transitions are all still in the ring lies on consecutive rows (mod size), oldest first"""
    size, pos = model.rings[c].maxsize, {int(tok): r for r, tok in enumerate(model.mem[c]) if tok >= 0}
    n = 0
    for cls, toks in model.episodes:
        if cls != c or not all(t in pos for t in toks):
            continue
        rows = [pos[t] for t in toks]
        assert all((rows[k + 1] - rows[k]) % size == 1 for k in range(len(rows) - 1)), toks
        n += 1
    return n


@pytest.mark.parametrize("size", [40 * 128 * 4, 1500])
def test_off_policy_batches_whole_episodes_end_to_end(size):
    """Three chunks of a real continuous collection (the env of tests/test_gpu_replay.py's dual test) through
    off_policy_batches(..., whole_episodes=True): both rings equal the model, with rings large enough and with rings that wrap."""
    from cm3_amd.replay import DeviceDualReplayBuffer, off_policy_batches
    from cm3_amd.rollout import ParticleRollout
    E, T = 128, 40
    env = _env(E)
    env.reset()
    ro = ParticleRollout(env, n_ticks=T, use_graph=False)
    dual = DeviceDualReplayBuffer(size=size, device=DEV)
    model = DualModel((size, size), E, 33)
    tt, ee = torch.arange(T, device=DEV).repeat_interleave(E), torch.arange(E, device=DEV).repeat(T)
    wants = []
    gen = torch.Generator(device=DEV).manual_seed(0)
    for batch in off_policy_batches(ro, dual, 3, batch_size=64, generator=gen, whole_episodes=True):
        assert batch["reward"].shape[0] == 64
        model.add_chunk(ro.done.cpu().numpy(), ro.collisions.cpu().numpy())
        wants.append(ro.as_reference_batch_torch(tt, ee, numpy=False))
        assert len(dual.mem1) + len(dual.mem2) + dual.pending == model.rings[0].len + model.rings[1].len + model.pending
    wants = {k: torch.cat([w[k] for w in wants]).contiguous() for k in wants[0]}
    _assert_holds(dual.mem1.cols, model.mem[0], wants, "memory_1")
    _assert_holds(dual.mem2.cols, model.mem[1], wants, "memory_2")
    assert (dual.mem1.idx, dual.mem2.idx) == (model.rings[0].idx, model.rings[1].idx)
    assert {cls for cls, _ in model.episodes} == {0, 1} and "one boundary" in model.seen      # asserted, not skipped
    total = sum(len(toks) for _, toks in model.episodes) + model.pending
    assert total == 3 * T * E
    if size >= total:
        assert len(dual.mem1) + len(dual.mem2) + dual.pending == total
    else:
        assert "wrap" in model.seen and len(dual.mem1) + len(dual.mem2) < total
    assert _contiguous_in_time_order(model, 0) > 0 and _contiguous_in_time_order(model, 1) > 0


def _sync_rollout(E=200, max_steps=33):
    from cm3_amd.rollout import ParticleRollout
    env = _env(E, max_steps=max_steps, auto_reset=False, seed=5)
    return ParticleRollout(env, use_graph=False).collect()


def test_episode_synchronous_rollout_equals_the_model():
    """auto_reset=False, T = max_steps: the mode the on-policy trainer uses, for which the flag path has no working route."""
    from cm3_amd.replay import DeviceDualReplayBuffer
    ro = _sync_rollout()
    T, E = ro.T, ro.env.E
    dual = DeviceDualReplayBuffer(size=8000, device=DEV)
    model = DualModel((8000, 8000), E, 0)
    valid = ro.valid.cpu().numpy()
    model.add_chunk(ro.done.cpu().numpy(), ro.collisions.cpu().numpy(), valid, sync=True)
    n1, n2 = dual.add_rollout(ro)
    assert (n1, n2) == (model.rings[0].len, model.rings[1].len) and n1 + n2 == int(valid.sum()) and dual.pending == 0
    assert (dual.mem1.len, dual.mem2.len, dual.mem1.idx, dual.mem2.idx) == (n1, n2, n1 % 8000, n2 % 8000)
    tt, ee = torch.arange(T, device=DEV).repeat_interleave(E), torch.arange(E, device=DEV).repeat(T)
    wants = ro.as_reference_batch_torch(tt, ee, numpy=False)
    _assert_holds(dual.mem1.cols, model.mem[0], wants, "memory_1")
    _assert_holds(dual.mem2.cols, model.mem[1], wants, "memory_2")
    bad = ro.episode_is_bad().cpu().numpy()
    assert sorted(e for cls, toks in model.episodes if cls == 0 for e in {toks[0] % E}) == sorted(np.nonzero(bad & valid.any(0))[0])


def _row_set(cols, n):
    names = sorted(k for k in cols if k not in ("v_local", "v_local_next"))
    m = torch.cat([cols[k][:n].reshape(n, -1).to(torch.float64) for k in names], dim=1)
    return torch.unique(m, dim=0, return_counts=True)


def test_a_chunk_of_whole_episodes_equals_add_with_flags_as_sets():
    """Every episode of an episode-synchronous chunk starts and ends in it: add_rollout and the existing add(cols, flags) put the same
    transitions into each memory; the order differs by design (episode by episode instead of tick by tick)."""
    from cm3_amd.replay import DeviceDualReplayBuffer
    ro = _sync_rollout()
    a, b = DeviceDualReplayBuffer(size=8000, device=DEV), DeviceDualReplayBuffer(size=8000, device=DEV)
    a.add_rollout(ro)
    tt, ee = ro.valid_indices()
    cols = ro.as_reference_batch(tt, ee, numpy=False)
    b.add({k: v.contiguous() for k, v in cols.items()}, ro.episode_is_bad()[ee])
    assert (len(a.mem1), len(a.mem2)) == (len(b.mem1), len(b.mem2)) and len(a.mem1) > 0 and len(a.mem2) > 0
    for ma, mb in ((a.mem1, b.mem1), (a.mem2, b.mem2)):
        (ra, ca), (rb, cb) = _row_set(ma.cols, len(ma)), _row_set(mb.cols, len(mb))
        assert torch.equal(ra, rb) and torch.equal(ca, cb)


def test_add_rollout_refuses_what_it_cannot_route_and_leaves_the_buffer_as_it_was():
    from cm3_amd import Cm3Error
    from cm3_amd.replay import DeviceDualReplayBuffer
    from cm3_amd.rollout import ParticleRollout
    env = _env(64)
    env.reset()
    ro = ParticleRollout(env, n_ticks=10, use_graph=False).collect()
    dual = DeviceDualReplayBuffer(size=500, device=DEV)
    dual.add_rollout(ro)
    state = (dual.mem1.idx, dual.mem1.len, dual.mem2.idx, dual.mem2.len, dual.pending)
    other = _env(64, seed=12)
    other.reset()
    with pytest.raises(Cm3Error, match="another env batch"):
        dual.add_rollout(ParticleRollout(other, n_ticks=10, use_graph=False).collect())
    with pytest.raises(Cm3Error, match="record_collisions"):
        dual.add_rollout(ParticleRollout(env, n_ticks=10, use_graph=False, record_collisions=False).collect(reset=False))
    assert (dual.mem1.idx, dual.mem1.len, dual.mem2.idx, dual.mem2.len, dual.pending) == state
    dual.drop_pending()
    assert dual.pending == 0
    dual.add_rollout(ParticleRollout(other, n_ticks=10, use_graph=False).collect(reset=False))
