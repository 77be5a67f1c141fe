"""GPU: the compact Checkers replay ring -- cm3_checkers_transitions_pack / cm3_checkers_ring_expand (csrc/batch.hip),
CheckersRollout.pack_into and replay.CompactCheckersReplayBuffer -- against the wide float64 ring (DeviceReplayBuffer) it stands in
for.  int8 -> float64 and int32 -> float64 are exact: every comparison is torch.equal over all rows and columns, dtype and shape
included; there are no tolerances."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import actor_checkers_oracle as AO
from tests import qmix_checkers_ref as QC
from tests.helpers import band_init, load_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PACK, EXPAND, GATHER, SCATTER = ("cm3_checkers_transitions_pack", "cm3_checkers_ring_expand", "cm3_checkers_transitions_gather",
                                 "cm3_rows_scatter")
GENERIC = dict(n_agents=3, init=dict(n_rows=5, n_columns=6, n_obs=1, agents_r=[0, 2, 4], agents_c=[6, 6, 6]))   # 81-byte windows, unpadded
BAND_N4 = dict(n_agents=4, init=band_init(4, 44))     # 3 x 8 band, in-band start cells, 4-byte padded 300-byte windows: the fast kernels above two agents


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
    s = _Spy(_lib.lib(), (PACK, EXPAND, GATHER, SCATTER))
    monkeypatch.setattr(_lib, "_lib", s)          # (objects built from here on hold the counting handle)
    return s


def _continuous(E=96, T=10, case="n2", seed=12341):
    from cm3_amd.rollout import CheckersRollout
    env, N, goals = _env(case, E, True, seed=seed)
    return env, CheckersRollout(env, n_ticks=T), goals, N


def _widen(name, v):
    """A compact column cast to the dtype of the wide ring's column."""
    base = name[5:] if name.startswith("next_") else name
    if base in ("grid", "obs_self_t", "vec"):
        return v.to(torch.float64)
    if base == "goals":
        return torch.nn.functional.one_hot(v.long(), 2)
    return v


def _rings_equal(compact, wide):
    from cm3_amd.rollout import CheckersRollout
    assert (compact.len, compact.idx) == (wide.len, wide.idx)
    assert tuple(compact.cols) == CheckersRollout.ORDER and set(wide.cols) == set(CheckersRollout.ORDER)
    for name in CheckersRollout.ORDER:
        got, want = _widen(name, compact.cols[name]), wide.cols[name]
        assert got.dtype == want.dtype and got.shape == want.shape, name
        if name == "goals":
            # rows never written hold zeros in both rings: a zero goal INDEX widens to the pair [1, 0], the wide ring's zeros are
            # [0, 0] -- the stored rows are compared through one_hot, the others must be untouched zeros on both sides
            n = compact.len
            assert not bool(compact.cols[name][n:].any()) and not bool(want[n:].any()), name
            got, want = got[:n], want[:n]
        assert torch.equal(got, want), name


def _same(a, b):
    from cm3_amd.rollout import CheckersRollout
    assert tuple(a) == tuple(b) == CheckersRollout.ORDER
    for name in a:
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, name
        assert torch.equal(a[name], b[name]), name


def _gens(seed):
    return torch.Generator(device=DEV).manual_seed(seed), torch.Generator(device=DEV).manual_seed(seed)


# (policy-driven collection for n1 and n2: the CM3 Checkers actor is built for the reference geometry's 5 x 5 windows, not for the
# generic case's 3 x 3 ones.  What the pack kernel reads does not depend on who chose the actions: the generic case covers the
# 3-agent, unpadded 81-byte records, the policy cases the carried prev0 and the one-launch rollout's buffers.)
@pytest.mark.parametrize("case,policy", [(c, p) for c in ("n1", "n2") for p in ("random", "auto")] + [("generic", "random"), ("band_n4", "random")])
def test_compact_ring_equals_the_wide_ring(case, policy, spy):
    """Four chunks of 960 transitions into rings of 2500 (the third wraps) and of 500 (every chunk exceeds the ring): after every
    add the compact ring, widened, IS the wide ring; sampling from both with generators seeded alike returns the same 16 columns."""
    from cm3_amd.replay import CompactCheckersReplayBuffer, DeviceReplayBuffer
    env, ro, goals, N = _continuous(case=case)
    actor = _policy(policy, N)
    compact, wide = CompactCheckersReplayBuffer(size=2500, device=DEV), DeviceReplayBuffer(size=2500, device=DEV)
    small_c, small_w = CompactCheckersReplayBuffer(size=500, device=DEV), DeviceReplayBuffer(size=500, device=DEV)
    seen_done = False
    for chunk in range(4):
        ro.collect(goals=goals, policy=actor, epsilon=0.3)
        seen_done |= bool(ro.done.any())
        before = dict(spy.calls)
        compact.add_rollout(ro)
        assert spy.calls[PACK] == before[PACK] + 1
        assert spy.calls[GATHER] == before[GATHER] and spy.calls[SCATTER] == before[SCATTER]
        wide.add_rollout(ro)
        _rings_equal(compact, wide)
        assert compact.len == min(960 * (chunk + 1), 2500) and compact.idx == 960 * (chunk + 1) % 2500 and len(compact) == compact.len
        small_c.add_rollout(ro)
        small_w.add_rollout(ro)
        _rings_equal(small_c, small_w)
        assert small_c.len == 500
        # sampling: below len == size on the first chunk of the large ring (everything, in storage order), above it afterwards
        for c, w, size in ((compact, wide, 128 if chunk else 1000), (small_c, small_w, 128), (small_c, small_w, 500)):
            ga, gb = _gens(100 + chunk)
            before = spy.calls[EXPAND]
            got = c.sample_batch(size, generator=ga)
            assert spy.calls[EXPAND] == before + 1
            want = w.sample_batch(size, generator=gb)
            _same(got, want)
            assert got["grid"].shape[0] == min(size, c.len)
            assert torch.equal(torch.rand(3, generator=ga, device=DEV), torch.rand(3, generator=gb, device=DEV))   # the same draws were made
    assert seen_done
    assert compact.cols["grid"].dtype == torch.int8 and compact.cols["vec"].dtype == torch.int32 and compact.cols["goals"].dtype == torch.uint8
    row = sum(v[0].numel() * v.element_size() for v in compact.cols.values())
    wide_row = sum(v[0].numel() * v.element_size() for v in wide.cols.values())
    assert row * 3 < wide_row                      # (the float64 columns stay: 3.7 x at the generic geometry, 5.2 x at the reference one)
    if case == "n2":
        assert (row, wide_row) == (707, 3657)
    _same(compact.all(), {k: wide.all()[k] for k in ro.ORDER})
    _same(compact.sample_n(64, generator=_gens(7)[0]), wide.sample_n(64, generator=_gens(7)[1]))
    ro.close()


def test_batches_share_no_storage_with_the_ring():
    from cm3_amd.replay import CompactCheckersReplayBuffer
    env, ro, goals, N = _continuous()
    buf = CompactCheckersReplayBuffer(size=960, device=DEV)
    ro.collect(goals=goals)
    buf.add_rollout(ro)
    ring_ptrs = {v.data_ptr() for v in buf.cols.values()}
    for size in (128, 5000):                       # sampled rows; everything (len <= size)
        batch = buf.sample_batch(size, generator=torch.Generator(device=DEV).manual_seed(3))
        assert not ring_ptrs & {v.data_ptr() for v in batch.values()}
        kept = {k: v.clone() for k, v in batch.items()}
        ro.collect()
        buf.add_rollout(ro)                        # overwrites every row of the ring
        for k in kept:
            assert torch.equal(batch[k], kept[k]), k
    everything = buf.all()
    kept = {k: v.clone() for k, v in everything.items()}
    ro.collect()
    buf.add_rollout(ro)
    assert all(torch.equal(everything[k], kept[k]) for k in kept)
    assert not all(torch.equal(buf.all()[k], kept[k]) for k in kept)
    ro.close()


def test_out_keeps_the_addresses_and_refuses_wrong_columns():
    from cm3_amd import Cm3Error
    from cm3_amd.replay import CompactCheckersReplayBuffer, DeviceReplayBuffer
    env, ro, goals, N = _continuous()
    compact, wide = CompactCheckersReplayBuffer(size=3000, device=DEV), DeviceReplayBuffer(size=3000, device=DEV)
    for _ in range(2):
        ro.collect(goals=goals)
        compact.add_rollout(ro)
        wide.add_rollout(ro)
    ga, gb = _gens(21)
    first = compact.sample_batch(128, generator=ga)
    wide.sample_batch(128, generator=gb)
    ptrs = {k: v.data_ptr() for k, v in first.items()}
    again = compact.sample_batch(128, generator=ga, out=first)
    assert {k: v.data_ptr() for k, v in again.items()} == ptrs
    _same(again, wide.sample_batch(128, generator=gb))
    _same(compact.sample_n(128, generator=ga, out=first), wide.sample_n(128, generator=gb))
    assert {k: v.data_ptr() for k, v in first.items()} == ptrs
    wrong = dict(
        dtype=("grid", dict(first, grid=first["grid"].float())),
        int_dtype=("actions", dict(first, actions=first["actions"].long())),
        row_shape=("obs_self_t", dict(first, obs_self_t=torch.zeros(128, N, 5, 5, 2, dtype=torch.float64, device=DEV))),
        row_count=("reward", dict(first, reward=torch.zeros(127, dtype=torch.float64, device=DEV))),
        non_contiguous=("actions_prev", dict(first, actions_prev=torch.zeros(128, 2 * N, dtype=torch.int32, device=DEV)[:, ::2])),
        missing=("goals", {k: v for k, v in first.items() if k != "goals"}),
        host=("done", dict(first, done=torch.zeros(128, dtype=torch.bool))))
    for what, (name, cols) in wrong.items():
        with pytest.raises(Cm3Error, match="column %s " % name):
            compact.sample_batch(128, generator=ga, out=cols)
    with pytest.raises(Cm3Error):
        compact.sample_batch(64, generator=ga, out=first)         # another row count
    ro.close()


def test_add_narrows_the_wide_columns_and_refuses_what_does_not_survive():
    from cm3_amd import Cm3Error
    from cm3_amd.replay import CompactCheckersReplayBuffer, DeviceReplayBuffer
    env, ro, goals, N = _continuous()
    ro.collect(goals=goals)
    cols = ro.as_reference_batch(numpy=False)
    for size in (2000, 700):                       # in the ring; more than the ring holds
        compact, wide = CompactCheckersReplayBuffer(size=size, device=DEV), DeviceReplayBuffer(size=size, device=DEV)
        for _ in range(2):
            compact.add(cols)
            wide.add(cols)
            _rings_equal(compact, wide)
        _same(compact.all(), {k: wide.all()[k] for k in ro.ORDER})
    one = CompactCheckersReplayBuffer(size=960, device=DEV)
    one.add(cols)
    _same(one.all(), cols)                         # the round trip, bit for bit
    state = (one.len, one.idx, {k: v.clone() for k, v in one.cols.items()})
    bad_grid = dict(cols, grid=cols["grid"].clone())
    bad_grid["grid"][5, 0, 0, 0] = 0.5
    bad_goals = dict(cols, goals=cols["goals"].clone())
    bad_goals["goals"][7, 0] = 1
    for bad in (bad_grid, bad_goals, dict(cols, vec=cols["vec"] + 2.0 ** 31), {k: v for k, v in cols.items() if k != "reward"}):
        with pytest.raises(Cm3Error):
            one.add(bad)
        assert (one.len, one.idx) == state[:2] and all(torch.equal(one.cols[k], state[2][k]) for k in state[2])
    # a ring that add() allocated takes add_rollout as well, and the other way round
    one.add_rollout(ro)
    wide = DeviceReplayBuffer(size=960, device=DEV)
    wide.add_rollout(ro)
    _rings_equal(one, wide)
    ro.close()


def test_pack_into_refuses_every_wrong_column():
    from cm3_amd import Cm3Error
    from cm3_amd.replay import CompactCheckersReplayBuffer
    from cm3_amd.rollout import CheckersRollout
    env, ro, goals, N = _continuous()
    ro.collect(goals=goals)
    ring = 2000
    good = {k: torch.zeros((ring,) + shape, dtype=dt, device=DEV) for k, (shape, dt) in ro.compact_column_specs().items()}
    assert ro.pack_into(good, 1500, ring) == 960
    ref = ro.as_reference_batch_torch(None, None, numpy=False)
    rows = (1500 + torch.arange(960, device=DEV)) % ring
    untouched = torch.ones(ring, dtype=torch.bool, device=DEV)
    untouched[rows] = False
    for name in good:
        assert torch.equal(_widen(name, good[name][rows]), ref[name]), name
        assert not bool(good[name][untouched].any()), name          # nothing outside the chunk's rows was written
    wrong = dict(
        wide=ro.empty_columns(ring),
        dtype=dict(good, vec=good["vec"].long()),
        row_shape=dict(good, goals=torch.zeros(ring, N, 2, dtype=torch.uint8, device=DEV)),
        row_count=dict(good, reward=torch.zeros(ring - 1, dtype=torch.float64, device=DEV)),
        non_contiguous=dict(good, actions_prev=torch.zeros(ring, 2 * N, dtype=torch.int32, device=DEV)[:, ::2]),
        missing={k: v for k, v in good.items() if k != "goals"},
        host=dict(good, done=torch.zeros(ring, dtype=torch.bool)))
    for what, cols in wrong.items():
        with pytest.raises(Cm3Error):
            ro.pack_into(cols, 0, ring)
    for start, size in ((-1, ring), (ring, ring), (0, 900)):
        with pytest.raises(Cm3Error):
            ro.pack_into(good, start, size)
    buf = CompactCheckersReplayBuffer(size=ring, device=DEV)
    buf.add_rollout(ro)
    assert (buf.len, buf.idx) == (960, 960)
    buf.cols = wrong["dtype"]
    with pytest.raises(Cm3Error):
        buf.add_rollout(ro)
    assert (buf.len, buf.idx) == (960, 960)             # the ring advances only after the pack was accepted
    env2, N2, goals2 = _env("n2", 32, False)
    ro2 = CheckersRollout(env2, n_ticks=10).collect(goals=goals2)
    with pytest.raises(Cm3Error):                        # an episode-synchronous collection has invalid transitions
        CompactCheckersReplayBuffer(size=ring, device=DEV).add_rollout(ro2)
    ro.close()
    ro2.close()


@pytest.mark.parametrize("term", [False, True])
def test_odd_record_strides_and_full_range_values_through_the_raw_abi(term):
    """A synthetic trajectory with odd record strides (55 / 151: byte granules) and full-range int8 / int32 values, packed into a
    wrapping ring and expanded again, against NumPy-style indexing of the source.  Negative bytes must survive."""
    from cm3_amd import _lib
    T, E, N, R, C, K = 3, 37, 2, 3, 8, 5
    gs, os_ = 55, 151
    rng = np.random.default_rng(3)
    dev = torch.device(DEV)
    t_ = lambda a: torch.as_tensor(a, device=dev)    # noqa: E731
    i8 = lambda *s: t_(rng.integers(-128, 128, s, dtype=np.int8))    # noqa: E731
    grid, obst = i8(T + 1, E, gs), i8(T + 1, E, os_)
    vec = t_(rng.integers(-2 ** 31, 2 ** 31, (T + 1, E, N, 4)).astype(np.int32))
    oo, ov = t_(rng.standard_normal((T + 1, E, N, 2))), t_(rng.standard_normal((T + 1, E, N, 4)))
    actions = t_(rng.integers(0, 5, (T, E, N)).astype(np.int32))
    lr, rew = t_(rng.standard_normal((T, E, N))), t_(rng.standard_normal((T, E)))
    done = t_((rng.integers(0, 2, (T, E)) * rng.integers(1, 256, (T, E))).astype(np.uint8))      # any non-zero byte is "done"
    goals = t_(rng.integers(0, 2, (E, N)).astype(np.uint8))
    gslots = t_(rng.integers(0, 2, (T + 1, E, N)).astype(np.uint8))
    prev0 = t_(rng.integers(0, 5, (E, N)).astype(np.int32))
    tgrid, tobst = i8(T, E, gs), i8(T, E, os_)
    tvec = t_(rng.integers(-2 ** 31, 2 ** 31, (T, E, N, 4)).astype(np.int32))
    too, tov = t_(rng.standard_normal((T, E, N, 2))), t_(rng.standard_normal((T, E, N, 4)))
    assert bool((grid < 0).any()) and bool((obst == -128).any()) and bool((vec < 0).any())
    d = _lib.CheckersDesc()
    d.n_envs, d.n_agents, d.n_rows, d.n_columns, d.n_obs, d.max_steps, d.grid_stride, d.obs_self_t_stride = E, N, R, C, 2, 33, gs, os_
    tr = _lib.CheckersTraj()
    fields = [("actions", actions), ("grid", grid), ("vec", vec), ("obs_others", oo), ("obs_self_t", obst), ("obs_self_v", ov),
              ("local_rewards", lr), ("reward", rew), ("done", done)]
    if term:
        fields += [("term_grid", tgrid), ("term_vec", tvec), ("term_obs_others", too), ("term_obs_self_t", tobst),
                   ("term_obs_self_v", tov), ("goals_slots", gslots)]
    for name, x in fields:
        setattr(tr, name, x.data_ptr())
        stride = name + ("_slot_stride" if name.endswith(("grid", "obs_self_t")) else "_stride")
        setattr(tr, stride, x[0].numel() * x.element_size())
    tr.goals = goals.data_ptr()
    B, ring, start = T * E, 150, 97                  # 111 transitions from row 97 of 150: wraps
    shapes = dict(grid=(R, C + 1, 2), vec=(N, 4), obs_others=(N, 2), obs_self_t=(N, K, K, 3), obs_self_v=(N, 4), actions_prev=(N,),
                  actions=(N,), reward=(), local_rewards=(N,), done=(), goals=(N,))
    cdt = dict(grid=torch.int8, obs_self_t=torch.int8, vec=torch.int32, actions_prev=torch.int32, actions=torch.int32, done=torch.bool,
               goals=torch.uint8)
    wdt = dict(actions_prev=torch.int32, actions=torch.int32, done=torch.bool, goals=torch.int64)
    comp, ccols = _lib.CheckersCompactCols(), {}
    for name, _ in comp._fields_[:16]:
        base = name[5:] if name.startswith("next_") else name
        ccols[name] = torch.full((ring,) + shapes[base], 77, dtype=cdt.get(base, torch.float64), device=dev)
        setattr(comp, name, ccols[name].data_ptr())
    comp.ring_start, comp.ring_size = start, ring
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.lib().cm3_checkers_transitions_pack(ctypes.byref(d), ctypes.byref(tr), prev0.data_ptr(), B, ctypes.byref(comp), stream))
    tt, ee = torch.arange(T, device=dev).repeat_interleave(E), torch.arange(E, device=dev).repeat(T)
    dn = (done[tt, ee] != 0)

    def nxt(x, tx, width=None):
        a, b = x[tt + 1, ee], tx[tt, ee]
        if width:
            a, b = a[:, :width], b[:, :width]
        return torch.where(dn.view(-1, *([1] * (a.dim() - 1))), b, a) if term else a
    prev = actions[(tt - 1).clamp(min=0), ee]
    if term:
        prev = torch.where((done[(tt - 1).clamp(min=0), ee] != 0).view(-1, 1), torch.zeros_like(prev), prev)
    prev = torch.where((tt > 0).view(-1, 1), prev, prev0[ee])
    want = dict(grid=grid[tt, ee, :54].reshape(B, R, C + 1, 2), vec=vec[tt, ee], obs_others=oo[tt, ee],
                obs_self_t=obst[tt, ee, :150].reshape(B, N, K, K, 3), obs_self_v=ov[tt, ee], actions_prev=prev, actions=actions[tt, ee],
                reward=rew[tt, ee], local_rewards=lr[tt, ee], next_grid=nxt(grid, tgrid, 54).reshape(B, R, C + 1, 2),
                next_vec=nxt(vec, tvec), next_obs_others=nxt(oo, too), next_obs_self_t=nxt(obst, tobst, 150).reshape(B, N, K, K, 3),
                next_obs_self_v=nxt(ov, tov), done=dn, goals=gslots[tt, ee] if term else goals[ee])
    rows = (start + torch.arange(B, device=dev)) % ring
    untouched = torch.ones(ring, dtype=torch.bool, device=dev)
    untouched[rows] = False
    for name, v in want.items():
        assert ccols[name].dtype == v.dtype and torch.equal(ccols[name][rows], v), name
        rest = ccols[name][untouched]
        assert torch.equal(rest, torch.full_like(rest, 77)), name          # the bytes around the chunk's rows stay
    # ... and expanded again: sampled rows (with repeats, first and last ring row of the chunk included), then rows 0 .. n - 1
    f = lambda x: x.to(torch.float64)      # noqa: E731
    wide_of = lambda c: {k: (f(v) if k.endswith(("grid", "obs_self_t", "vec")) else    # noqa: E731
                             torch.nn.functional.one_hot(v.long(), 2) if k == "goals" else v) for k, v in c.items()}
    pos = t_(rng.integers(0, B, 120))
    pos[0], pos[1], pos[2] = 0, B - 1, 0
    head = ring - start                               # transitions before the wrap: ring rows 0 .. hold b = head ..
    for index, n, ref in ((rows[pos].contiguous(), 120, {k: v[pos] for k, v in want.items()}),
                          (None, B - head, {k: v[head:] for k, v in want.items()})):
        out, wcols = _lib.CheckersTransitionCols(), {}
        for name, _ in out._fields_[:16]:
            base = name[5:] if name.startswith("next_") else name
            shape = shapes[base] + ((2,) if base == "goals" else ())
            wcols[name] = torch.empty((n,) + shape, dtype=wdt.get(base, torch.float64), device=dev)
            setattr(out, name, wcols[name].data_ptr())
        _lib.check(_lib.lib().cm3_checkers_ring_expand(ctypes.byref(d), ctypes.byref(comp), _lib.ptr(index), n, ctypes.byref(out), stream))
        for name, v in wide_of(ref).items():
            assert wcols[name].dtype == v.dtype and wcols[name].shape == v.shape and torch.equal(wcols[name], v), name
        assert bool((wcols["grid"] < 0).any()) and bool((wcols["next_obs_self_t"] < 0).any()) and bool((wcols["vec"] < 0).any())


@pytest.mark.parametrize("policy", ["random", "qmix"])
def test_off_policy_batches_are_those_of_the_wide_ring(policy, spy):
    from cm3_amd.qmix import CheckersQmixAgent
    from cm3_amd.replay import CompactCheckersReplayBuffer, DeviceReplayBuffer, off_policy_batches
    from cm3_amd.rollout import CheckersRollout
    batches = []
    for cls in (CompactCheckersReplayBuffer, DeviceReplayBuffer):
        env, ro, goals, N = _continuous()
        kw = dict(goals=goals)
        if policy == "qmix":
            kw.update(policy=CheckersQmixAgent(QC.init_weights(np.random.default_rng(202), 2), 2, device=DEV, seed=12341), epsilon=0.2)
        buf = cls(size=2000, device=DEV)              # the third chunk wraps
        gen = torch.Generator(device=DEV).manual_seed(11)
        before = dict(spy.calls)
        got = [{k: v.clone() for k, v in b.items()} for b in off_policy_batches(ro, buf, 3, batch_size=128, generator=gen, **kw)]
        if cls is CompactCheckersReplayBuffer:
            assert spy.calls[PACK] == before[PACK] + 3 and spy.calls[EXPAND] == before[EXPAND] + 3
            assert spy.calls[GATHER] == before[GATHER] and spy.calls[SCATTER] == before[SCATTER]
        assert len(got) == 3 and len(buf) == 2000 and all(tuple(b) == CheckersRollout.ORDER and b["grid"].shape[0] == 128 for b in got)
        batches.append(got)
        assert bool(ro.done.any())
        ro.close()
    for a, b in zip(*batches):
        _same(a, b)
