"""GPU: the Checkers kernels at 3..8 agents on the reference geometry (3 x 8 band, n_obs 2), where 4-byte padded records select the
multi-lane fast kernels -- CkPlanTab<N>'s lane plans (NQ cell quads, 4N + 2N(N-1) normalised values, the k-th-other-agent rule),
ckf_emit<N> of the reset kernel, the second table emit of an auto-reset for N >= 3 (CkFresh<N>::kOn is N <= 2), the pairwise total
at N == 8, the fused-ticks and the non-temporal builds -- and the generic kernel on the same layouts (unpadded records).  The other
Checkers tests reach the fast kernels with one and two agents only.

Integer grid world: every comparison is bit-exact (np.array_equal on float64 / torch.equal) against VecCheckersOracle, which
tests/test_oracle_checkers.py holds to the dense restatement of env/checkers.py and to fixtures recorded from the reference at
these agent counts.  Start cells: the first N of a seeded permutation of the 27 cells of band plus start column."""
import functools

import numpy as np
import pytest
import torch

from oracle import philox
from oracle.checkers_oracle import VecCheckersOracle
from tests.helpers import band_init, left_biased_actions, load_cfg

pytestmark = pytest.mark.gpu
MB128 = 128 << 20          # ck_rollout (csrc/checkers.hip): observation slots of a rollout from here on are a stream


def _env(init, N, E, max_steps=33, **kw):
    from cm3_amd.checkers import VecCheckersEnv
    return VecCheckersEnv(init, N, max_steps, E, device="cuda:0", **kw)


def _oracle(init, N, E, max_steps=33):
    return VecCheckersOracle(init["n_rows"], init["n_columns"], init["n_obs"], init["agents_r"], init["agents_c"], N, max_steps, E)


def _variant():
    from cm3_amd import _lib
    return _lib.last_kernel_variant()


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _check_obs(got, want, sel=slice(None), what=None):
    (grid, vec), oo, ot, ov = got
    for name, x, w in zip(("grid", "vec", "obs_others", "obs_self_t", "obs_self_v"), (grid, vec, oo, ot, ov), want):
        assert np.array_equal(_f64(x)[sel], w[sel]), (name, what)


def _check_step(out, w, what=None):
    gs, oo, ot, ov, total, local, done = out
    _check_obs((gs, oo, ot, ov), w[:5], what=what)
    assert np.array_equal(_f64(total), w[5]), ("total", what)
    assert np.array_equal(_f64(local), w[6]), ("local_rewards", what)
    assert np.array_equal(done.cpu().numpy(), w[7]), ("done", what)


def _check_state(env, orc):
    st = env.get_state()
    i64 = lambda x: x.cpu().numpy().astype(np.int64)      # noqa: E731
    assert np.array_equal(i64(st["mask"]), orc.mask.astype(np.int64))
    assert np.array_equal(i64(st["r"]), orc.loc[:, :, 0]) and np.array_equal(i64(st["c"]), orc.loc[:, :, 1])
    assert np.array_equal(i64(st["n_green"]), orc.count[:, :, 0]) and np.array_equal(i64(st["n_orange"]), orc.count[:, :, 1])
    assert np.array_equal(i64(st["steps"]), orc.steps) and np.array_equal(i64(st["goals"]), orc.goal)


# ---- a. step and reset, every output, every tick --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _reference_episode(N, E):
    """(init, goal_index, reset outputs, [(actions, step outputs)] of 33 ticks) of the oracle: computed once per (N, E), shared by the
    padded and the unpadded case, never written to."""
    init = band_init(N, 10 * N + E % 7)
    rng = np.random.default_rng(1000 * N + E)
    goal_idx = rng.integers(0, 2, (E, N))
    orc = _oracle(init, N, E)
    first = orc.reset(goal_idx)
    ticks = []
    for t in range(33):
        acts = left_biased_actions(rng, (E, N))
        ticks.append((acts, orc.step(acts)))
    return init, goal_idx, first, ticks


# E: 8 lanes per env = 8 envs per wave, 32 per workgroup -- 1: seven eighths of a wave idle; 33: one env in a second workgroup;
# 300: ragged waves and ragged blocks.  (N, E) outermost, so the two record layouts share one reference episode.
@pytest.mark.parametrize("N,E,padded", [(N, E, p) for N in range(3, 9) for E in (1, 33, 300) for p in (True, False)])
def test_step_and_reset_bit_exact_vs_oracle(N, E, padded):
    init, goal_idx, first, ticks = _reference_episode(N, E)
    env = _env(init, N, E, padded_records=padded)
    out = env.reset(goal_index=torch.as_tensor(goal_idx))
    # a dispatch change must not quietly move these cases off the kernels they are here for
    assert _variant().startswith("%s<-,N=%d," % ("k_checkers_reset_fast" if padded else "k_checkers_reset", N)), _variant()
    _check_obs(out[:4], first, what="reset")
    assert not bool(out[4].any())
    for t, (acts, want) in enumerate(ticks):
        got = env.step(torch.as_tensor(acts))
        assert _variant().startswith("%s<-,N=%d," % ("k_checkers_step_fast" if padded else "k_checkers_step", N)), _variant()
        _check_step(got, want, what=t)
    assert bool(got[6].all())


# ---- b. scripted sweeps ---------------------------------------------------------------------------------------------------------
S, U, D, L, R = 0, 1, 2, 3, 4


def _run_script(script, E=9, extra_seed=0):
    """N = 3 on the start column, padded records: `script` ([T][3] actions, the same in every env; goals random per env and agent)
    through the oracle and the device, tick for tick.  -> the oracle and the per-tick oracle outputs."""
    N = 3
    init = band_init(N)
    assert init["agents_c"] == [8, 8, 8] and init["agents_r"] == [0, 1, 2]
    goal_idx = np.random.default_rng(50 + extra_seed).integers(0, 2, (E, N))
    orc = _oracle(init, N, E)
    want0 = orc.reset(goal_idx)
    wants = [orc.step(np.tile(np.array(a), (E, 1))) for a in script]
    env = _env(init, N, E, padded_records=True)
    out = env.reset(goal_index=torch.as_tensor(goal_idx))
    _check_obs(out[:4], want0, what="reset")
    for t, a in enumerate(script):
        got = env.step(torch.as_tensor(np.tile(np.array(a), (E, 1))))
        assert _variant().startswith("k_checkers_step_fast<-,N=3,"), _variant()
        _check_step(got, wants[t], what=t)
    _check_state(env, orc)
    return orc, wants


def test_serpentine_sweep_reaches_the_last_count_entry():
    """Agent 0 walks row 0 leftwards, down, row 1 rightwards to column 7, down, row 2 leftwards; the others stay.  It ends with
    n_green = n_orange = 12 -- the last entry of the count table norm[20..32], which random walks do not reach -- and the episode
    ends on tick 24, before max_steps = 33; two more ticks follow the done."""
    sweep = [L] * 8 + [D] + [R] * 7 + [D] + [L] * 7
    script = [[a, S, S] for a in sweep] + [[S, S, S]] * 2
    orc, wants = _run_script(script)
    done = np.array([w[7] for w in wants])
    assert not done[:23].any() and done[23:].all()                  # conditions on the oracle: the sweep does what it is here for
    assert np.array_equal(orc.count[:, 0], np.full((9, 2), 12)) and not orc.count[:, 1:].any()
    assert np.array_equal(wants[23][4][:, 0, 2:], np.ones((9, 2)))   # obs_self_v counts: 12 / 12


def test_three_agents_sweep_their_rows_and_end_early():
    """All agents "left" for nine ticks: each sweeps its own row, all 24 cells are collected on tick 8 (done before max_steps), the
    ninth "left" runs into the wall."""
    orc, wants = _run_script([[L, L, L]] * 9, extra_seed=1)
    done = np.array([w[7] for w in wants])
    assert not done[:7].any() and done[7:].all()
    assert np.array_equal(orc.count.sum(axis=2), np.full((9, 3), 8))
    assert np.array_equal(wants[8][6], np.full((9, 3), -0.1))


# ---- c. auto-reset for N >= 3 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,padded", [(3, True), (5, True), (8, True), (5, False)])
@pytest.mark.parametrize("capture", [True, False])
def test_auto_reset_above_two_agents(N, padded, capture):
    """auto_reset, max_steps = 5, in-kernel actions, 16 ticks, 257 envs: the !kFresh branch of the fast step kernel (a finished env
    gets a second table emit instead of the fresh-record copy), with and without terminal capture; the generic kernel once."""
    E, seed, T = 257, 29, 16
    init = band_init(N, 300 + N)
    goal_idx = np.random.default_rng(N).integers(0, 2, (E, N))
    orc = _oracle(init, N, E, max_steps=5)
    want = orc.reset(goal_idx)
    env = _env(init, N, E, max_steps=5, seed=seed, auto_reset=True, padded_records=padded)
    if capture:
        env.enable_terminal_capture()
    out = env.reset(goal_index=torch.as_tensor(goal_idx))
    _check_obs(out[:4], want, what="reset")
    ids = np.arange(E)
    episode, steps = np.ones(E, np.int64), np.zeros(E, np.int64)       # reset() made this episode 1
    n_done = 0
    for t in range(T):
        gs, oo, ot, ov, total, local, done = env.step()
        assert _variant().startswith("%s<-,N=%d," % ("k_checkers_step_fast" if padded else "k_checkers_step", N)), _variant()
        acts = env.last_actions.cpu().numpy()
        for ep, st in sorted(set(zip(episode.tolist(), steps.tolist()))):
            m = (episode == ep) & (steps == st)
            assert np.array_equal(acts[m], philox.expected_actions(seed, ids[m], ep, st, N, checkers=True)), t
        w = orc.step(acts)
        d = w[7]
        assert np.array_equal(_f64(total), w[5]) and np.array_equal(_f64(local), w[6]), t
        assert np.array_equal(done.cpu().numpy(), d), t
        if d.any():
            n_done += int(d.sum())
            if capture:
                _check_obs(env.terminal_obs(), w[:5], sel=d, what=("terminal", t))
            else:
                assert env.terminal_obs() is None
            fresh = orc.reset_envs(d)      # the fresh episode where done, the step output elsewhere
            _check_obs((gs, oo, ot, ov), fresh, what=("slot", t))
        else:
            _check_obs((gs, oo, ot, ov), w[:5], what=("slot", t))
        episode, steps = episode + d, np.where(d, 0, steps + 1)
        assert np.array_equal(env._episode.cpu().numpy(), episode), t
    _check_state(env, orc)
    assert n_done == 3 * E


# ---- d. fused ticks and the non-temporal build ------------------------------------------------------------------------------------
TRAJ = ("grid", "vec", "obs_others", "obs_self_t", "obs_self_v", "actions", "local_rewards", "reward", "done", "term_grid", "term_vec",
        "term_obs_others", "term_obs_self_t", "term_obs_self_v", "goal_slots")


def _onehot_goals(N, seed):
    return np.eye(2)[np.random.default_rng(seed).integers(0, 2, N)]


@pytest.mark.parametrize("N", [3, 8])
def test_fused_rollout_equals_per_tick(N):
    from cm3_amd.rollout import CheckersRollout
    E, T = 333, 40
    init, goals = band_init(N, 400 + N), _onehot_goals(N, N)
    outs = []
    for fused, graph in ((False, False), (False, True), (True, False)):
        env = _env(init, N, E, max_steps=9, seed=6, auto_reset=True)
        ro = CheckersRollout(env, n_ticks=T, use_graph=graph, fused=fused).collect(goals)
        assert _variant().startswith("k_checkers_step_fast<-,N=%d,waves=4,fused=%d,sp=plain," % (N, fused)), _variant()
        outs.append((ro, env))
    a, env_a = outs[0]
    for ro, env in outs[1:]:
        for name in TRAJ:
            assert torch.equal(getattr(a, name), getattr(ro, name)), name
        assert torch.equal(env_a.steps, env.steps) and torch.equal(env_a._mask, env._mask) and torch.equal(env_a._agents, env._agents)
        assert torch.equal(env_a._episode, env._episode) and torch.equal(env_a._goals, env._goals)
        ro.close()
    assert int(a.done.sum()) >= 4 * E            # episodes of 9 ticks: four auto-resets inside the 40-tick rollout
    a.close()


@pytest.mark.parametrize("mode", ["graph", "fused"])
def test_streaming_rollout_at_eight_agents_equals_stepwise(mode):
    """The smallest rollout of 2048 eight-agent envs whose observation slots are a stream (1936 bytes per env and tick: 34 ticks
    pass 128 MB) reports the non-temporal build -- one tick fewer the plain one -- and equals the same envs stepped by env.step()."""
    from cm3_amd.rollout import CheckersRollout
    N, E = 8, 2048
    init, goals = band_init(N, 408), _onehot_goals(N, 8)
    mk = lambda: _env(init, N, E, max_steps=9, seed=23, auto_reset=True)      # noqa: E731
    env, ref = mk(), mk()
    per_env = env.grid_stride + env.obst_stride + N * 4 * 4 + N * env.Lo * 8 + N * 4 * 8
    assert per_env == 1936
    T = -(-MB128 // (per_env * E))
    assert per_env * E * T >= MB128 > per_env * E * (T - 1)
    kw = dict(use_graph=(mode == "graph"), fused=(mode == "fused"))
    below = CheckersRollout(mk(), n_ticks=T - 1, **kw).collect(goals)
    assert _variant().startswith("k_checkers_step_fast<-,N=8,waves=4,fused=%d,sp=plain," % (mode == "fused")), _variant()
    below.close()
    del below
    ref.enable_terminal_capture()
    ref.reset(goals)
    ro = CheckersRollout(env, n_ticks=T, **kw).collect(goals)
    assert _variant().startswith("k_checkers_step_fast<-,N=8,waves=4,fused=%d,sp=nt," % (mode == "fused")), _variant()
    n_done = 0
    for t in range(T):
        (g, v), oo, ot, ov, rew, local, done = ref.step()
        assert torch.equal(ref.last_actions, ro.actions[t]), t
        assert torch.equal(rew, ro.reward[t]) and torch.equal(local, ro.local_rewards[t]) and torch.equal(done, ro.done[t].bool()), t
        assert torch.equal(g, ro.grid[t + 1]) and torch.equal(v, ro.vec[t + 1]) and torch.equal(oo, ro.obs_others[t + 1]), t
        assert torch.equal(ot, ro.obs_self_t[t + 1]) and torch.equal(ov, ro.obs_self_v[t + 1]), t
        assert torch.equal(ref._goals, ro.goal_slots[t + 1]), t
        if bool(done.any()):
            n_done += int(done.sum())
            (tg, tv), too, tot, tov = ref.terminal_obs()
            assert torch.equal(tg[done], ro.term_grid[t][done]) and torch.equal(tv[done], ro.term_vec[t][done]), t
            assert torch.equal(too[done], ro.term_obs_others[t][done]) and torch.equal(tot[done], ro.term_obs_self_t[t][done]), t
            assert torch.equal(tov[done], ro.term_obs_self_v[t][done]), t
    assert n_done >= 3 * E
    ro.close()


# ---- e. masked reset ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("padded", [True, False])
def test_masked_reset(N, padded):
    """reset(goal_index=..., mask=m) after seven ticks, m random at about one half: selected envs restart with their new goals (the
    oracle's reset_envs), the others keep state, goals and observation; one more tick shows the state both kinds continue from."""
    E = 300
    init = load_cfg("checkers_stage2.json")["init"] if N == 2 else band_init(N, 500 + N)
    rng = np.random.default_rng(60 + N)
    goal_idx = rng.integers(0, 2, (E, N))
    orc = _oracle(init, N, E)
    orc.reset(goal_idx)
    env = _env(init, N, E, padded_records=padded)
    env.reset(goal_index=torch.as_tensor(goal_idx))
    for t in range(7):
        acts = left_biased_actions(rng, (E, N))
        want = orc.step(acts)
        got = env.step(torch.as_tensor(acts))
    _check_step(got, want, what="before")
    m = rng.random(E) < 0.5
    assert 0 < m.sum() < E
    new_goals = rng.integers(0, 2, (E, N))
    kept = [x.copy() for x in want[:5]]
    want = orc.reset_envs(m, new_goals)
    for x, y in zip(want, kept):
        assert np.array_equal(x[~m], y[~m])                          # (the oracle itself leaves the unselected envs alone)
    out = env.reset(goal_index=torch.as_tensor(new_goals), mask=torch.as_tensor(m))
    assert _variant().startswith("%s<-,N=%d," % ("k_checkers_reset_fast" if padded else "k_checkers_reset", N)), _variant()
    _check_obs(out[:4], want, what="masked reset")
    assert not bool(out[4].any())
    _check_state(env, orc)
    assert np.array_equal(orc.goal[m], new_goals[m]) and np.array_equal(orc.goal[~m], goal_idx[~m])
    acts = left_biased_actions(rng, (E, N))
    _check_step(env.step(torch.as_tensor(acts)), orc.step(acts), what="after")
