"""GPU: the one-launch Checkers transition export (cm3_checkers_transitions_gather, csrc/batch.hip) and what stands on it --
CheckersRollout.as_reference_batch / export_into / sample_batch / on_policy_minibatches, DeviceReplayBuffer.add_rollout and
off_policy_batches -- against the torch composition it replaces (CheckersRollout.as_reference_batch_torch).  Every value is a copy
or an exact integer -> double conversion: all comparisons are torch.equal, dtype and shape included."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import actor_checkers_oracle as AO
from tests import qmix_checkers_ref as QC
from tests.helpers import band_init, load_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRY = "cm3_checkers_transitions_gather"
GENERIC = dict(n_agents=3, init=dict(n_rows=5, n_columns=6, n_obs=1, agents_r=[0, 2, 4], agents_c=[6, 6, 6]))   # 81-byte windows: 8-byte units
BAND_N4 = dict(n_agents=4, init=band_init(4, 44))     # 3 x 8 band, in-band start cells, 4-byte padded 300-byte windows: the fast kernels above two agents


def _same(a, b, names=None):
    from cm3_amd.rollout import CheckersRollout
    assert tuple(a) == tuple(b) == CheckersRollout.ORDER
    for name in names or a:
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, name
        assert torch.equal(a[name], b[name]), name


def _env(case, E, auto_reset, seed=12341, max_steps=7):
    from cm3_amd.checkers import VecCheckersEnv
    cfg = {"generic": GENERIC, "band_n4": BAND_N4}.get(case) or load_cfg("checkers_stage%d.json" % (1 if case == "n1" else 2))
    env = VecCheckersEnv(cfg["init"], cfg["n_agents"], max_steps, E, device=DEV, seed=seed, auto_reset=auto_reset,
                         padded_records=(False if case == "generic" else None))
    N = cfg["n_agents"]
    goals = np.array([[0, 1]]) if N == 1 else np.eye(2)[np.arange(N) % 2]
    return env, N, goals


def _policy(kind, N, seed=12341):
    if kind == "random":
        return None
    from cm3_amd.actor import CheckersActor
    stage = 1 if N == 1 else 2
    return CheckersActor(AO.init_weights(np.random.default_rng(40 + N), N, stage=stage), N, stage=stage, device=DEV, seed=seed,
                         precision="f16x3")


class _Spy(object):
    """The library handle with the calls of some entry points counted."""

    def __init__(self, handle, names):
        self._handle, self.calls = handle, {n: 0 for n in names}

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if name not in self.calls:
            return fn

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


@pytest.fixture
def spy(monkeypatch):
    from cm3_amd import _lib
    s = _Spy(_lib.lib(), (ENTRY, "cm3_rows_scatter"))
    monkeypatch.setattr(_lib, "_lib", s)          # (objects built from here on hold the counting handle)
    return s


CASES = [(c, a, p) for c in ("n1", "n2") for a in (False, True) for p in ("random", "tick", "auto")] + \
        [("generic", False, "random"), ("generic", True, "random"), ("band_n4", False, "random"), ("band_n4", True, "random")]


@pytest.mark.parametrize("case,auto_reset,policy", CASES)
def test_kernel_equals_the_torch_composition(case, auto_reset, policy):
    from cm3_amd.rollout import CheckersRollout
    E, T = 150, 10
    env, N, goals = _env(case, E, auto_reset)
    actor = _policy(policy, N)
    ro = CheckersRollout(env, n_ticks=T, policy_mode="tick" if policy == "tick" else "auto")
    gen = torch.Generator(device=DEV).manual_seed(5)
    seen = dict(term=False, zeroed=False, goal_change=False)
    for chunk in range(3):                               # (prev0 is carried from chunk to chunk in continuous mode)
        ro.collect(goals=goals, policy=actor, epsilon=0.3)
        if policy == "auto":
            assert ro._rolled is not None                # the one-launch policy rollout ran: prev0 comes through the spare buffer
        if chunk and auto_reset:
            assert ro.prev0.data_ptr() != ro._prev_bufs[0].data_ptr()
        done = ro.done.bool()
        assert bool(done.any())
        if auto_reset:
            assert bool(done.any(0).all())               # max_steps < n_ticks: every env ends an episode in every chunk
            t, e = done.nonzero(as_tuple=True)
            seen["term"] |= bool((ro.term_grid[t, e] != ro.grid[t + 1, e]).any())
            seen["zeroed"] |= bool((done[:-1].unsqueeze(2) & (ro.actions[:-1] != 0)).any())
            if N == 1:
                seen["goal_change"] |= bool((ro.goal_slots[1:] != ro.goal_slots[:-1]).any())
        # the whole trajectory / all valid transitions
        whole = ro.as_reference_batch(numpy=False)
        _same(whole, ro.as_reference_batch_torch(None, None, numpy=False))
        tt, ee = ro.valid_indices()
        assert whole["reward"].shape[0] == tt.numel() and (tt.numel() == T * E) == auto_reset
        _same(ro.as_reference_batch(tt, ee, numpy=False), ro.as_reference_batch_torch(tt, ee, numpy=False))
        # random pairs with duplicates, first and last tick included
        rt = torch.randint(0, T, (700,), generator=gen, device=DEV)
        re_ = torch.randint(0, E, (700,), generator=gen, device=DEV)
        rt[:40], rt[40:80] = 0, T - 1
        rt[80:90], re_[80:90] = rt[0], re_[0]
        _same(ro.as_reference_batch(rt, re_, numpy=False), ro.as_reference_batch_torch(rt, re_, numpy=False))
        # the numpy form and an empty selection
        got = ro.as_reference_batch(rt[:9], re_[:9])
        want = ro.as_reference_batch_torch(rt[:9], re_[:9])
        for name in want:
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
        empty = ro.as_reference_batch(rt[:0], re_[:0], numpy=False)
        assert all(v.shape[0] == 0 for v in empty.values())
    if auto_reset:
        assert seen["term"] and seen["zeroed"] and (N != 1 or seen["goal_change"]), seen
    ro.close()


def test_odd_record_strides_take_the_byte_loads():
    """Records whose stride is odd (nothing in cm3_amd allocates them; the C ABI accepts any stride >= the record) cannot be read
    two bytes at a time: the same columns through single-byte loads, against NumPy indexing of a synthetic trajectory."""
    from cm3_amd import _lib
    T, E, N, R, C, K = 3, 37, 2, 3, 8, 5
    gs, os_ = 55, 151
    rng = np.random.default_rng(3)
    dev = torch.device(DEV)
    t_ = lambda a: torch.as_tensor(a, device=dev)    # noqa: E731
    grid = t_(rng.integers(-128, 128, (T + 1, E, gs), dtype=np.int8))
    obst = t_(rng.integers(-128, 128, (T + 1, E, os_), dtype=np.int8))
    vec = t_(rng.integers(-2 ** 31, 2 ** 31, (T + 1, E, N, 4)).astype(np.int32))
    oo, ov = t_(rng.standard_normal((T + 1, E, N, 2))), t_(rng.standard_normal((T + 1, E, N, 4)))
    actions = t_(rng.integers(0, 5, (T, E, N)).astype(np.int32))
    lr, rew = t_(rng.standard_normal((T, E, N))), t_(rng.standard_normal((T, E)))
    done = t_(rng.integers(0, 2, (T, E)).astype(np.uint8))
    goals = t_(rng.integers(0, 2, (E, N)).astype(np.uint8))
    prev0 = t_(rng.integers(0, 5, (E, N)).astype(np.int32))
    d = _lib.CheckersDesc()
    d.n_envs, d.n_agents, d.n_rows, d.n_columns, d.n_obs, d.max_steps, d.grid_stride, d.obs_self_t_stride = E, N, R, C, 2, 33, gs, os_
    tr = _lib.CheckersTraj()
    for name, x in (("actions", actions), ("grid", grid), ("vec", vec), ("obs_others", oo), ("obs_self_t", obst), ("obs_self_v", ov),
                    ("local_rewards", lr), ("reward", rew), ("done", done)):
        setattr(tr, name, x.data_ptr())
        stride = name + ("_slot_stride" if name in ("grid", "obs_self_t") else "_stride")
        setattr(tr, stride, x[0].numel() * x.element_size())
    tr.goals = goals.data_ptr()
    B = 200
    tt, ee = t_(rng.integers(0, T, B)), t_(rng.integers(0, E, B))
    shapes = dict(grid=(R, C + 1, 2), vec=(N, 4), obs_others=(N, 2), obs_self_t=(N, K, K, 3), obs_self_v=(N, 4), actions_prev=(N,),
                  actions=(N,), reward=(), local_rewards=(N,), done=(), goals=(N, 2))
    dts = dict(actions_prev=torch.int32, actions=torch.int32, done=torch.bool, goals=torch.int64)
    out, cols = _lib.CheckersTransitionCols(), {}
    for name, _ in out._fields_[:16]:
        base = name[5:] if name.startswith("next_") else name
        cols[name] = torch.empty((B,) + shapes[base], dtype=dts.get(base, torch.float64), device=dev)
        setattr(out, name, cols[name].data_ptr())
    _lib.check(_lib.lib().cm3_checkers_transitions_gather(ctypes.byref(d), ctypes.byref(tr), prev0.data_ptr(), tt.data_ptr(), ee.data_ptr(),
                                                          B, ctypes.byref(out), torch.cuda.current_stream(dev).cuda_stream))
    f = lambda x: x.to(torch.float64)      # noqa: E731
    assert torch.equal(cols["grid"], f(grid[tt, ee, :54]).view(B, R, C + 1, 2))
    assert torch.equal(cols["next_grid"], f(grid[tt + 1, ee, :54]).view(B, R, C + 1, 2))
    assert torch.equal(cols["obs_self_t"], f(obst[tt, ee, :150]).view(B, N, K, K, 3))
    assert torch.equal(cols["next_obs_self_t"], f(obst[tt + 1, ee, :150]).view(B, N, K, K, 3))
    assert torch.equal(cols["vec"], f(vec[tt, ee])) and torch.equal(cols["next_obs_self_v"], ov[tt + 1, ee])
    assert torch.equal(cols["goals"], torch.nn.functional.one_hot(goals[ee].long(), 2))
    # no terminal capture: actions_prev is not zeroed behind a done
    assert torch.equal(cols["actions_prev"], torch.where((tt > 0).view(-1, 1), actions[(tt - 1).clamp(min=0), ee], prev0[ee]))
    assert torch.equal(cols["done"], done[tt, ee].bool()) and torch.equal(cols["reward"], rew[tt, ee])


def _continuous(E=96, T=10, case="n2", seed=12341):
    from cm3_amd.rollout import CheckersRollout
    env, N, goals = _env(case, E, True, seed=seed)
    return env, CheckersRollout(env, n_ticks=T), goals


def _ring_equal(a, b):
    assert (a.len, a.idx) == (b.len, b.idx) and set(a.cols) == set(b.cols)
    for name in a.cols:
        assert a.cols[name].dtype == b.cols[name].dtype and torch.equal(a.cols[name], b.cols[name]), name


@pytest.mark.parametrize("case", ["n2", "n1"])
def test_add_rollout_is_export_plus_add_in_one_launch(case, spy):
    from cm3_amd.replay import DeviceReplayBuffer
    env, ro, goals = _continuous(case=case)
    a, b = DeviceReplayBuffer(size=2500, device=DEV), DeviceReplayBuffer(size=2500, device=DEV)    # 960 per chunk: the third wraps
    small_a, small_b = DeviceReplayBuffer(size=500, device=DEV), DeviceReplayBuffer(size=500, device=DEV)
    for chunk in range(4):
        ro.collect(goals=goals)
        before = dict(spy.calls)
        a.add_rollout(ro)
        assert spy.calls[ENTRY] == before[ENTRY] + 1 and spy.calls["cm3_rows_scatter"] == before["cm3_rows_scatter"]
        b.add({k: v.contiguous() for k, v in ro.as_reference_batch_torch(None, None, numpy=False).items()})
        _ring_equal(a, b)
        assert a.len == min(960 * (chunk + 1), 2500) and a.idx == 960 * (chunk + 1) % 2500
        # a chunk larger than the ring: the newest transitions survive, as sequential adds leave them
        small_a.add_rollout(ro)
        small_b.add({k: v.contiguous() for k, v in ro.as_reference_batch_torch(None, None, numpy=False).items()})
        _ring_equal(small_a, small_b)
        assert small_a.len == 500
    # a ring that add() allocated takes add_rollout as well (same columns, same dtypes)
    b.add_rollout(ro)
    a.add_rollout(ro)
    _ring_equal(a, b)
    ro.close()


def test_export_into_refuses_every_wrong_column():
    from cm3_amd import Cm3Error
    from cm3_amd.replay import DeviceReplayBuffer
    env, ro, goals = _continuous()
    ro.collect(goals=goals)
    ring = 2000
    good = ro.empty_columns(ring, zero=True)
    assert ro.export_into(good, 1500, ring) == 960
    ref = ro.as_reference_batch_torch(None, None, numpy=False)
    rows = (1500 + torch.arange(960, device=DEV)) % ring
    for name in good:
        assert torch.equal(good[name][rows], ref[name]), name
    N = env.n
    wrong = dict(
        dtype=dict(good, grid=good["grid"].float()),
        int_dtype=dict(good, actions=good["actions"].long()),
        row_shape=dict(good, obs_self_t=torch.zeros(ring, N, 5, 5, 2, dtype=torch.float64, device=DEV)),
        row_count=dict(good, reward=torch.zeros(ring - 1, dtype=torch.float64, device=DEV)),
        non_contiguous=dict(good, actions_prev=torch.zeros(ring, 2 * N, dtype=torch.int32, device=DEV)[:, ::2]),
        missing={k: v for k, v in good.items() if k != "goals"},
        host=dict(good, done=torch.zeros(ring, dtype=torch.bool)))
    for what, cols in wrong.items():
        with pytest.raises(Cm3Error):
            ro.export_into(cols, 0, ring)
    for start, size in ((-1, ring), (ring, ring), (0, 900)):
        with pytest.raises(Cm3Error):
            ro.export_into(good, start, size)
    buf = DeviceReplayBuffer(size=ring, device=DEV)
    buf.add_rollout(ro)
    assert (buf.len, buf.idx) == (960, 960)
    buf.cols = wrong["dtype"]
    with pytest.raises(Cm3Error):
        buf.add_rollout(ro)
    assert (buf.len, buf.idx) == (960, 960)             # the ring advances only after the export was accepted
    # an episode-synchronous collection has invalid transitions: no whole-trajectory export
    env2, N2, goals2 = _env("n2", 32, False)
    from cm3_amd.rollout import CheckersRollout
    ro2 = CheckersRollout(env2, n_ticks=10).collect(goals=goals2)
    with pytest.raises(Cm3Error):
        ro2.export_into(ro2.empty_columns(ring), 0, ring)
    with pytest.raises(Cm3Error):
        DeviceReplayBuffer(size=ring, device=DEV).add_rollout(ro2)
    ro.close()
    ro2.close()


@pytest.mark.parametrize("auto_reset", [False, True])
def test_on_policy_minibatches_cost_one_export_launch(auto_reset, spy):
    from cm3_amd.rollout import CheckersRollout
    E, T = 1024, 10                                       # 10240 transitions (fewer valid ones in episode-synchronous mode) >= 64 * 128
    env, N, goals = _env("n2", E, auto_reset)
    ro = CheckersRollout(env, n_ticks=T).collect(goals=goals)
    gen = torch.Generator(device=DEV).manual_seed(9)
    tt, ee = ro.valid_indices()
    n = tt.numel()
    assert (n == T * E) == auto_reset and n > 128
    before = spy.calls[ENTRY]
    mbs = list(ro.on_policy_minibatches(24, 128, generator=gen))
    assert spy.calls[ENTRY] == before + 1 and len(mbs) == 24
    pos = ro.last_sample_positions
    assert pos.shape == (24, 128) and int(pos.min()) >= 0 and int(pos.max()) < n
    assert all(torch.unique(row).numel() == 128 for row in pos)
    flat = pos.reshape(-1)
    want = ro.as_reference_batch_torch(tt[flat], ee[flat], numpy=False)
    for m, mb in enumerate(mbs):
        assert tuple(mb) == CheckersRollout.ORDER
        for name, v in mb.items():
            assert v.dtype == want[name].dtype and torch.equal(v, want[name][m * 128:(m + 1) * 128]), (m, name)
    # sample_batch: `size` distinct valid transitions, or all of them
    one = ro.sample_batch(128, generator=gen, numpy=False)
    assert one["reward"].shape == (128,) and one["obs_self_t"].dtype == torch.float64
    everything = ro.sample_batch(10 ** 6, generator=gen, numpy=False)
    _same(everything, ro.as_reference_batch_torch(tt, ee, numpy=False))
    ro.close()


@pytest.mark.parametrize("policy", ["random", "qmix"])
def test_off_policy_batches_take_the_one_launch_route(policy, spy):
    from cm3_amd.qmix import CheckersQmixAgent
    from cm3_amd.replay import DeviceReplayBuffer, off_policy_batches
    from cm3_amd.rollout import CheckersRollout
    env, ro, goals = _continuous()
    kw = dict(goals=goals)
    if policy == "qmix":
        kw.update(policy=CheckersQmixAgent(QC.init_weights(np.random.default_rng(202), 2), 2, device=DEV, seed=12341), epsilon=0.2)
    buf = DeviceReplayBuffer(size=100000, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(11)
    n = 0
    for batch in off_policy_batches(ro, buf, 3, batch_size=128, generator=gen, **kw):
        n += 960
        assert spy.calls[ENTRY] == n // 960 and spy.calls["cm3_rows_scatter"] == 0
        assert len(buf) == n and tuple(batch) == CheckersRollout.ORDER and batch["grid"].shape[0] == 128
        want = ro.as_reference_batch_torch(None, None, numpy=False)
        for name, v in want.items():
            assert buf.cols[name].dtype == v.dtype and torch.equal(buf.all()[name][n - 960:n], v), name
    assert bool(ro.done.any())
    ro.close()


def test_out_keeps_the_addresses():
    from cm3_amd import Cm3Error
    env, ro, goals = _continuous()
    ro.collect(goals=goals)
    tt = torch.arange(10, device=DEV).repeat_interleave(5)
    ee = torch.arange(50, device=DEV)
    first = ro.as_reference_batch(tt, ee, numpy=False)
    ptrs = {k: v.data_ptr() for k, v in first.items()}
    ro.collect()
    again = ro.as_reference_batch(tt, ee, numpy=False, out=first)
    assert {k: v.data_ptr() for k, v in again.items()} == ptrs
    _same(again, ro.as_reference_batch_torch(tt, ee, numpy=False))
    with pytest.raises(Cm3Error):
        ro.as_reference_batch(tt[:49], ee[:49], numpy=False, out=first)
    with pytest.raises(Cm3Error):
        ro.as_reference_batch(tt, ee, numpy=True, out=first)
    ro.close()
