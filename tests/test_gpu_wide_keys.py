"""GPU: every device random stream under full-width keys -- a 64-bit seed with both key words live (and one whose LOW word is zero),
global ids whose high word is non-zero and whose low word carries out inside the batch (tests/wide_keys.py: SEEDS, BASE, E = 37,
CARRY = 19).  Every other test of the suite runs with seeds and id bases below 2^16, where key word 1 and counter word 1 are zero on
the device and a kernel, wrapper or packed record that kept 32 bits of either would pass.  tests/test_wide_keys_oracle.py proves that
the oracle's output changes under each such loss at every point compared here, so these equalities can fail.

  A  particle reset + generated actions through VecParticleEnv.reset() / .step(): the three step kernels, N = 2 and 5 (second Philox
     call), float64 and float32, same-launch resets at episodes 2 and 3
  B  the same through ParticleRollout: packed live records (rec=1), live state, slot-chained, fused ticks
  C  Checkers generated actions (action-block table; N = 5 draws agent 4's block in-kernel) through VecCheckersEnv and
     CheckersRollout (graph, fused), and the goal bit of a one-agent env over episodes 2 .. 4
  D  the policy uniform: ParticleActor.act / CheckersActor.act and the collectors in launch pairs and in one launch
  E  the exploration words: ParticleQmixAgent.act / CheckersQmixAgent.act and the collectors in launch pairs and in one launch
  F  the rows stream: ParticleActor / CheckersActor rows at explicit draws (0xFFFFFFFF included) and under the device-side counter
     started at 0xFFFFFFFE, so that it wraps within three launches; Checkers also at a row id base with bit 63 set

Integer outputs are compared for exact equality over all entries, entries 18 and 19 (the two sides of the carry) once more by name.
Policy and QMIX launches run at epsilon = 1: the mixed probabilities are then exactly uniform and a QMIX agent always explores, so
the action is a function of the stream alone; one case per class runs at epsilon = 0.3 on the device's own probabilities / greedy
actions.  Inverse-CDF picks leave out rows whose uniform lies within 1e-4 of a CDF boundary, at most 1 row in 50 of a case (one
launch, or the launches of one collect; tests/test_wide_keys_oracle.py confirms on the oracle's uniforms that the cases stay within
that); the rows stream at epsilon 0.3 is compared on every row, as its own tests do.  Reset positions keep the bounds of
tests/test_gpu_particle.py (1e-12 float64 positions, 1e-15 goals, 5e-7 float32).  Every case is 37 envs or rows and one launch or
one 8-tick collect; the whole file runs in a few seconds.

Entry points that do not exist, and what stands in for them: the one-launch Checkers kernels cover one and two agents (N = 5 runs
as launch pairs here); the one-launch particle QMIX rollout covers N in {1, 2, 4, 8} (N = 5: act() and launch pairs); the goal bit
is drawn for one agent only (N = 1 there, not 2 / 5); ParticleActor / ParticleQmixAgent collectors take the env's env_id_base, so
for them only unequal SEEDS are a key mismatch -- a base that differs on the agent is never read, which the case asserts instead.
"""
import numpy as np
import pytest
import torch

from oracle import actor_checkers_oracle as CO
from oracle import actor_oracle as AO
from oracle import philox
from tests import actor_rows_ref as RR
from tests import qmix_checkers_ref as QC
from tests import qmix_ref as QR
from tests import wide_keys as WK
from tests.helpers import band_init, load_cfg
from tests.test_gpu_actor_rows_counted import _Checkers as CkRows
from tests.test_gpu_actor_rows_counted import _Particle as PtRows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E, BASE, CARRY, T, MAX_STEPS = WK.E, WK.BASE, WK.CARRY, WK.TICKS, WK.MAX_STEPS
M32 = 0xFFFFFFFF
STEP_KERNEL = {"env": "k_particle_step<", "pair": "k_particle_step_pairs<", "agent": "k_particle_step_agents<"}


def _variant():
    from cm3_amd import _lib
    return _lib.last_kernel_variant()


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want, what):
    """exact equality over all entries (leading axis = env / row), the two sides of the carry once more by name"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0].tolist()
    if got.shape[0] > CARRY:
        assert np.array_equal(got[CARRY - 1], want[CARRY - 1]), (what, "entry 18", "wrong entries", bad)
        assert np.array_equal(got[CARRY], want[CARRY]), (what, "entry 19", "wrong entries", bad)
    assert not bad, (what, "wrong entries", bad)


def _per_env(fn, ids, episode, steps):
    """fn(ids[m], episode, step) over the envs m that share (episode, step), assembled per env"""
    out = None
    for ep, st in sorted(set(zip(episode.tolist(), steps.tolist()))):
        m = (episode == ep) & (steps == st)
        part = np.asarray(fn(ids[m], int(ep), int(st)))
        if out is None:
            out = np.zeros((len(ids),) + part.shape[1:], part.dtype)
        out[m] = part
    return out


def _inverse_cdf_same(actions, probs, u, what, left_out=None):
    """actions [E, N] against AO.sample_actions(probs [E * N, 5], u [E, N]) off the CDF boundaries.  At most 1 row in 50 of a case is
    left out: of this launch, or -- with a _LeftOut that the caller settles -- of the launches of one collect."""
    rows = u.size
    u = np.asarray(u, np.float32).reshape(rows)
    probs = np.asarray(probs, np.float32).reshape(rows, 5)
    safe = np.abs(np.cumsum(probs.astype(np.float64), axis=1)[:, :4] - u[:, None]).min(axis=1) > 1e-4
    tally = _LeftOut() if left_out is None else left_out
    tally.rows, tally.out = tally.rows + rows, tally.out + int((~safe).sum())
    want = np.where(safe, AO.sample_actions(probs, u), -1).reshape(np.shape(actions))
    got = np.where(safe.reshape(np.shape(actions)), np.asarray(actions), -1)
    _same(got, want, what)
    if left_out is None:
        tally.settle(what)


class _LeftOut(object):
    """rows of one case left out of the inverse-CDF comparison"""

    def __init__(self):
        self.rows = self.out = 0

    def settle(self, what):
        assert self.out * 50 <= self.rows, (what, self.out, self.rows)


UNIFORM = np.full((1, 5), 0.2, np.float32)          # the mixture at epsilon = 1: (1 - 1) p + 1 / 5, whatever the network says


class _Clock(object):
    """(episode, steps) of every env, advanced by the done flags of a trajectory: reset() makes episode 1, step 0"""

    def __init__(self, n):
        self.episode, self.steps = np.ones(n, np.int64), np.zeros(n, np.int64)

    def tick(self, done):
        done = np.asarray(done).astype(bool)
        self.episode, self.steps = self.episode + done, np.where(done, 0, self.steps + 1)
        return done


# ---- A. particle reset + generated actions, straight through the env -----------------------------------------------------------------
def _penv(seed, N, n=E, base=BASE, dtype=torch.float32, kernel="auto", **kw):
    from cm3_amd.particle import VecParticleEnv
    kw.setdefault("auto_reset", True)
    return VecParticleEnv(load_cfg(WK.RESET_CFG[N]), N, WK.P_RANDOM, MAX_STEPS, n, device=DEV, dtype=dtype, seed=seed, env_id_base=base,
                          kernel=kernel, **kw)


def _reset_same(state_en4, goals_en2, seed, ids, episode, N, dtype, sel, what):
    """positions / velocities / goals of the envs `sel` (state [E, N, 4] = vel, pos) against the reset stream at `episode`"""
    pos, lm, _ = philox.expected_reset(seed, ids[sel], int(episode), load_cfg(WK.RESET_CFG[N]), N, WK.P_RANDOM)
    st, gl = _np(state_en4).astype(np.float64)[sel], _np(goals_en2).astype(np.float64)[sel]
    tol_pos, tol_goal = (1e-12, 1e-15) if dtype == torch.float64 else (5e-7, 5e-7)
    err_pos, err_goal = np.abs(st[..., 2:4] - pos).max(axis=(1, 2)), np.abs(gl - lm).max(axis=(1, 2))
    where = np.nonzero(sel)[0]
    assert np.all(st[..., 0:2] == 0), what
    assert err_pos.max() < tol_pos, (what, float(err_pos.max()), "wrong entries", where[err_pos >= tol_pos].tolist())
    assert err_goal.max() < tol_goal, (what, float(err_goal.max()), "wrong entries", where[err_goal >= tol_goal].tolist())


def run_particle_env_case(seed, base, n, kernel, N, dtype):
    """reset() and TICKS steps of an auto-reset env (max_steps 3: same-launch resets at episodes 2 and 3) against the Philox
    specification under (seed, base); -> what a shard comparison needs"""
    ids = WK.ids(base, n)
    env = _penv(seed, N, n, base, dtype, kernel)
    env.reset()
    everyone = np.ones(n, bool)
    _reset_same(env.global_state, env.goals, seed, ids, 1, N, dtype, everyone, "reset()")
    clock, keep = _Clock(n), []
    for t in range(T):
        out = env.step()
        v = _variant()
        assert v.startswith(STEP_KERNEL[kernel]) and (",N=%d," % N) in v and ("<f64," in v) == (dtype == torch.float64), v
        want = _per_env(lambda i, ep, st: philox.expected_actions(seed, i, ep, st, N), ids, clock.episode, clock.steps)
        _same(_np(env.last_actions), want, ("actions", t))
        done = clock.tick(_np(out[5]))
        assert np.array_equal(_np(env.episode), clock.episode) and np.array_equal(_np(env.steps), clock.steps), t
        for ep in np.unique(clock.episode[done]):
            _reset_same(env.global_state, env.goals, seed, ids, ep, N, dtype, done & (clock.episode == ep), ("same-launch reset", t, int(ep)))
        keep.append((env.last_actions.clone(), env.global_state.clone(), env.goals.clone()))
    assert clock.episode.min() >= 3, "every env restarted at least twice"
    return keep


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("kernel", ["env", "pair", "agent"])
def test_particle_env_reset_and_actions(kernel, N, dtype, seed):
    run_particle_env_case(seed, BASE, E, kernel, N, dtype)


@pytest.mark.parametrize("kernel,N,dtype", [("pair", 2, torch.float32), ("env", 5, torch.float64)])
def test_particle_env_shard_equals_the_tail_of_the_full_run(kernel, N, dtype):
    """envs [19, 37) as their own object under env_id_base = BASE + 19, a base whose low word is zero"""
    full = run_particle_env_case(WK.SEEDS[0], BASE, E, kernel, N, dtype)
    tail = run_particle_env_case(WK.SEEDS[0], WK.SHARD_BASE, E - CARRY, kernel, N, dtype)
    for t, (a, b) in enumerate(zip(full, tail)):
        for x, y in zip(a, b):
            assert torch.equal(x[CARRY:], y), t


# ---- B. the same through the collectors ----------------------------------------------------------------------------------------------
COLLECT_MODES = {"record": dict(live_state=True), "slots": dict(live_state=False), "fused": dict(fused=True)}


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("N", [2, 4])
@pytest.mark.parametrize("mode", sorted(COLLECT_MODES))
def test_particle_collectors_reset_and_actions(mode, N, seed):
    from cm3_amd.rollout import ParticleRollout
    ids = WK.ids()
    env = _penv(seed, N)
    env.reset()
    ro = ParticleRollout(env, n_ticks=T, use_graph=True, **COLLECT_MODES[mode]).collect(reset=False)
    v = _variant()
    if mode == "record":
        assert ro._live and v.startswith("k_particle_step_pairs<f32,N=%d," % N) and ",live=1," in v and ",rec=1" in v, v
    elif mode == "slots":
        assert not ro._live and ",live=0," in v and ",rec=1" not in v and ",fused=0," in v, v
    else:
        assert ",fused=1," in v and ",rec=1" not in v, v
    state, goals = ro.state.permute(0, 2, 1, 3), ro.goals.permute(0, 2, 1, 3)            # [T + 1, E, N, .]
    _reset_same(state[0], goals[0], seed, ids, 1, N, torch.float32, np.ones(E, bool), "slot 0")
    clock = _Clock(E)
    for t in range(T):
        want = _per_env(lambda i, ep, st: philox.expected_actions(seed, i, ep, st, N), ids, clock.episode, clock.steps)
        _same(_np(ro.actions[t]), want, ("actions", t))
        done = clock.tick(_np(ro.done[t]))
        for ep in np.unique(clock.episode[done]):
            _reset_same(state[t + 1], goals[t + 1], seed, ids, ep, N, torch.float32, done & (clock.episode == ep), ("restart", t, int(ep)))
    assert clock.episode.min() >= 3
    assert np.array_equal(_np(env.episode), clock.episode) and np.array_equal(_np(env.steps), clock.steps)
    ro.close()


# ---- C. Checkers generated actions and the goal bit ----------------------------------------------------------------------------------
def _ck_init(N):
    return load_cfg("checkers_stage%d.json" % (1 if N == 1 else 2))["init"] if N <= 2 else band_init(N, 300 + N)


def _ckenv(seed, N, n=E, base=BASE, max_steps=MAX_STEPS, **kw):
    from cm3_amd.checkers import VecCheckersEnv
    kw.setdefault("auto_reset", True)
    return VecCheckersEnv(_ck_init(N), N, max_steps, n, device=DEV, seed=seed, env_id_base=base, **kw)


def _ck_goals(N):
    return np.random.default_rng(N).integers(0, 2, (E, N))


def run_checkers_env_case(seed, base, n, N, padded):
    ids = WK.ids(base, n)
    env = _ckenv(seed, N, n, base, padded_records=padded)
    # stage 1 of the action stream, the per-env table a step launch loads
    _same(_np(env._action_block).view(np.uint32), np.stack(philox.action_block(seed, ids, 0), axis=1), "action-block table")
    env.reset(goal_index=torch.as_tensor(_ck_goals(N)[E - n:]))          # (a shard takes the goals of its envs of the full batch)
    clock, keep = _Clock(n), []
    for t in range(T):
        out = env.step()
        v = _variant()
        assert v.startswith("%s<-,N=%d," % ("k_checkers_step_fast" if padded else "k_checkers_step", N)), v
        want = _per_env(lambda i, ep, st: philox.expected_actions(seed, i, ep, st, N, checkers=True), ids, clock.episode, clock.steps)
        _same(_np(env.last_actions), want, ("actions", t))
        clock.tick(_np(out[6]))
        assert np.array_equal(_np(env._episode), clock.episode), t
        keep.append((env.last_actions.clone(), out[0][0].clone(), out[0][1].clone(), out[4].clone()))
    assert clock.episode.min() >= 3
    return keep


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("N,padded", [(2, True), (2, False), (5, True), (5, False)])
def test_checkers_env_actions(N, padded, seed):
    """N = 5: agent 4 is the first word of Philox call 1, which the kernel draws itself (the table holds call 0)"""
    run_checkers_env_case(seed, BASE, E, N, padded)


def test_checkers_env_shard_equals_the_tail_of_the_full_run():
    full = run_checkers_env_case(WK.SEEDS[0], BASE, E, 5, True)
    tail = run_checkers_env_case(WK.SEEDS[0], WK.SHARD_BASE, E - CARRY, 5, True)
    for t, (a, b) in enumerate(zip(full, tail)):
        for x, y in zip(a, b):
            assert torch.equal(x[CARRY:], y), t


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("mode", ["graph", "fused"])
def test_checkers_collectors_actions(mode, N, seed):
    from cm3_amd.rollout import CheckersRollout
    ids = WK.ids()
    env = _ckenv(seed, N)
    goals = np.eye(2)[_ck_goals(N)]
    ro = CheckersRollout(env, n_ticks=T, use_graph=(mode == "graph"), fused=(mode == "fused")).collect(goals)
    v = _variant()
    assert v.startswith("k_checkers_step_fast<-,N=%d," % N) and (",fused=%d," % (mode == "fused")) in v, v
    clock = _Clock(E)
    for t in range(T):
        want = _per_env(lambda i, ep, st: philox.expected_actions(seed, i, ep, st, N, checkers=True), ids, clock.episode, clock.steps)
        _same(_np(ro.actions[t]), want, ("actions", t))
        clock.tick(_np(ro.done[t]))
    assert clock.episode.min() >= 3 and np.array_equal(_np(env._episode), clock.episode)
    ro.close()


def _goal_bits(seed, ids, episode):
    return _per_env(lambda i, ep, st: (philox.reset_words(seed, i, ep, 0)[0] & np.uint32(1)).astype(np.int64), ids, episode, np.zeros_like(episode))


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("how", ["env", "env-unpadded", "graph", "fused"])
def test_checkers_goal_bit_over_three_episodes(how, seed):
    """One agent: every same-launch restart draws the goal, word .x & 1 of the reset block (global env id, episode, call 0);
    max_steps 2, so seven ticks reach episodes 2, 3 and 4."""
    from cm3_amd.rollout import CheckersRollout
    ids, ticks = WK.ids(), 7
    env = _ckenv(seed, 1, max_steps=2, padded_records=(how != "env-unpadded"))
    first = torch.zeros(E, 1, dtype=torch.int64)
    clock, seen = _Clock(E), set()
    if how.startswith("env"):
        env.reset(goal_index=first)
        for t in range(ticks):
            done = clock.tick(_np(env.step()[6]))
            if done.any():
                got = _np(env.get_state()["goals"])[:, 0].astype(np.int64)
                want = _goal_bits(seed, ids, clock.episode)
                _same(np.where(done, got, -1), np.where(done, want, -1), ("goal", t))
                seen |= set(clock.episode[done].tolist())
    else:
        ro = CheckersRollout(env, n_ticks=ticks, use_graph=(how == "graph"), fused=(how == "fused")).collect(np.eye(2)[first.numpy()])
        assert (",fused=%d," % (how == "fused")) in _variant(), _variant()
        for t in range(ticks):
            done = clock.tick(_np(ro.done[t]))
            if done.any():
                got = _np(ro.goal_slots[t + 1])[:, 0].astype(np.int64)
                _same(np.where(done, got, -1), np.where(done, _goal_bits(seed, ids, clock.episode), -1), ("goal", t))
                seen |= set(clock.episode[done].tolist())
        ro.close()
    assert seen >= set(WK.GOAL_EPISODES), seen


# ---- D. the policy uniform -----------------------------------------------------------------------------------------------------------
def _pactor(seed, N, precision="f32", base=0):
    from cm3_amd.actor import ParticleActor
    stage = 1 if N == 1 else 2
    w = AO.init_weights(np.random.default_rng(100 + N), N, stage=stage)
    return ParticleActor(w, N, stage=stage, device=DEV, seed=seed, env_id_base=base, precision=precision)


def _cactor(seed, N, precision="f32", base=BASE):
    from cm3_amd.actor import CheckersActor
    stage = 1 if N == 1 else 2
    w = CO.init_weights(np.random.default_rng(100 + N), N, stage=stage)
    return CheckersActor(w, N, stage=stage, device=DEV, seed=seed, env_id_base=base, precision=precision)


def _policy_u(seed, ids, clock, N):
    return _per_env(lambda i, ep, st: AO.policy_uniforms(seed, i, ep, st, N), ids, clock.episode, clock.steps)


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("N", [2, 5])
def test_particle_actor_act(N, seed):
    ids = WK.ids()
    env = _penv(seed, N)
    env.reset()
    actor = _pactor(seed, N)                                      # (the actor's own base is 0: act() passes the env's on)
    clock = _Clock(E)
    for t in range(2):
        a, p = actor.act(env, 1.0, return_probs=True)
        assert _variant().startswith("k_actor_particle<f32,N=%d," % N), _variant()
        assert np.all(_np(p) == np.float32(0.2)), "epsilon = 1: the mixture is exactly uniform"
        _inverse_cdf_same(_np(a), _np(p), _policy_u(seed, ids, clock, N), ("eps 1", t))
        a3, p3 = actor.act(env, 0.3, return_probs=True)
        assert np.ptp(_np(p3), axis=-1).max() > 1e-3
        _inverse_cdf_same(_np(a3), _np(p3), _policy_u(seed, ids, clock, N), ("eps 0.3", t))
        clock.tick(_np(env.step(a)[5]))


def run_particle_policy_collect(seed, base, n, N, mode, actor_seed=None, actor_base=0, **kw):
    """collect(policy=actor, epsilon=1) -> (actions [T, n, N] checked against the policy stream under (actor seed, env base), variant)"""
    from cm3_amd.rollout import ParticleRollout
    ids = WK.ids(base, n)
    env = _penv(seed, N, n, base)
    env.reset()
    actor = _pactor(seed if actor_seed is None else actor_seed, N, "f16x3", actor_base)
    ro = ParticleRollout(env, n_ticks=T, policy_mode=mode, **kw).collect(policy=actor, epsilon=1.0, reset=False)
    v = _variant()
    clock, left_out = _Clock(n), _LeftOut()
    for t in range(T):
        _inverse_cdf_same(_np(ro.actions[t]), np.broadcast_to(UNIFORM, (n * N, 5)), _policy_u(actor.seed, ids, clock, N), ("actions", t), left_out)
        clock.tick(_np(ro.done[t]))
    left_out.settle("the collect")
    assert clock.episode.min() >= 3
    out = ro.actions.clone(), ro.state.clone()
    ro.close()
    return out, v


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("N,mode,kw,one_launch", [(2, "tick", {}, False), (2, "auto", {}, True), (5, "tick", {}, False),
                                                  (5, "episode", {"partial_tiles": True}, True)],
                         ids=["N2-pairs", "N2-episode", "N5-pairs", "N5-padded-tiles"])
def test_particle_policy_collectors(N, mode, kw, one_launch, seed):
    _, v = run_particle_policy_collect(seed, BASE, E, N, mode, **kw)
    assert v.startswith("k_policy_rollout<") == one_launch and (not one_launch or (",N=%d," % N) in v), v


def test_particle_policy_shard_equals_the_tail_of_the_full_run():
    (fa, fs), _ = run_particle_policy_collect(WK.SEEDS[0], BASE, E, 2, "auto")
    (ta, ts), _ = run_particle_policy_collect(WK.SEEDS[0], WK.SHARD_BASE, E - CARRY, 2, "auto")
    assert torch.equal(fa[:, CARRY:], ta) and torch.equal(fs[:, :, CARRY:], ts)


def test_particle_policy_key_mismatch():
    """agent on SEEDS[0], env on its low word: the one launch refuses, "auto" falls back to the launch pairs, whose actor launch
    draws under the AGENT's seed; the agent's own env_id_base is never read by a collector (the env's is passed on)."""
    from cm3_amd import Cm3Error
    with pytest.raises(Cm3Error, match="seed"):
        run_particle_policy_collect(WK.SEEDS[0] & M32, BASE, E, 2, "episode", actor_seed=WK.SEEDS[0])
    _, v = run_particle_policy_collect(WK.SEEDS[0] & M32, BASE, E, 2, "auto", actor_seed=WK.SEEDS[0])
    assert not v.startswith("k_policy_rollout"), v
    _, v = run_particle_policy_collect(WK.SEEDS[0], BASE, E, 2, "auto", actor_base=BASE & M32)
    assert v.startswith("k_policy_rollout<"), v


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("N", [2, 5])
def test_checkers_actor_act(N, seed):
    ids = WK.ids()
    env = _ckenv(seed, N)
    env.reset(goal_index=torch.as_tensor(_ck_goals(N)))
    actor = _cactor(seed, N, base=0)                              # (act() passes the env's base on)
    clock = _Clock(E)
    for t in range(2):
        a, p = actor.act(env, 1.0, return_probs=True)
        assert _variant().startswith("k_ck_actor<"), _variant()
        assert np.all(_np(p) == np.float32(0.2))
        _inverse_cdf_same(_np(a), _np(p), _policy_u(seed, ids, clock, N), ("eps 1", t))
        a3, p3 = actor.act(env, 0.3, actions_prev=_np(a), return_probs=True)
        _inverse_cdf_same(_np(a3), _np(p3), _policy_u(seed, ids, clock, N), ("eps 0.3", t))
        clock.tick(_np(env.step(a)[6]))


def run_checkers_policy_collect(make, stream, seed, base, n, N, mode, policy_seed=None, policy_base=None):
    """collect(goals, policy, epsilon=1) with record_probs; `stream(policy seed, ids, clock, actions, probs, what)` checks one tick"""
    from cm3_amd.rollout import CheckersRollout
    ids = WK.ids(base, n)
    env = _ckenv(seed, N, n, base)
    policy = make(seed if policy_seed is None else policy_seed, N, "f16x3", base if policy_base is None else policy_base)
    ro = CheckersRollout(env, n_ticks=T, policy_mode=mode, record_probs=True)
    ro.collect(np.eye(2)[_ck_goals(N)[E - n:]], policy=policy, epsilon=1.0)
    v = _variant()
    clock, left_out = _Clock(n), _LeftOut()
    for t in range(T):
        stream(policy.seed, ids, clock, _np(ro.actions[t]), _np(ro.probs[t]), ("actions", t), left_out)
        done = clock.tick(_np(ro.done[t]))
        if N == 1 and done.any():
            got = _np(ro.goal_slots[t + 1])[:, 0].astype(np.int64)
            _same(np.where(done, got, -1), np.where(done, _goal_bits(seed, ids, clock.episode), -1), ("goal", t))
    left_out.settle("the collect")
    assert clock.episode.min() >= 3 and np.array_equal(_np(env._episode), clock.episode)
    out = ro.actions.clone(), ro.grid.clone()
    ro.close()
    return out, v


def _policy_stream(seed, ids, clock, actions, probs, what, left_out):
    assert np.all(probs == np.float32(0.2)), what
    _inverse_cdf_same(actions, probs, _policy_u(seed, ids, clock, actions.shape[1]), what, left_out)


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("N,mode,one_launch", [(2, "tick", False), (2, "auto", True), (1, "auto", True), (5, "auto", False)],
                         ids=["N2-pairs", "N2-one-launch", "N1-one-launch-goal-bit", "N5-pairs"])
def test_checkers_policy_collectors(N, mode, one_launch, seed):
    _, v = run_checkers_policy_collect(_cactor, _policy_stream, seed, BASE, E, N, mode)
    assert v.startswith("k_ck_policy_rollout<") == one_launch and (not one_launch or (",N=%d," % N) in v), v


def test_checkers_policy_shard_equals_the_tail_of_the_full_run():
    (fa, fg), _ = run_checkers_policy_collect(_cactor, _policy_stream, WK.SEEDS[0], BASE, E, 2, "auto")
    (ta, tg), _ = run_checkers_policy_collect(_cactor, _policy_stream, WK.SEEDS[0], WK.SHARD_BASE, E - CARRY, 2, "auto")
    assert torch.equal(fa[:, CARRY:], ta) and torch.equal(fg[:, CARRY:], tg)


@pytest.mark.parametrize("make,stream_name", [(_cactor, "policy"), ("qmix", "explore")], ids=["actor", "qmix"])
def test_checkers_one_launch_key_mismatch(make, stream_name):
    """Unequal seeds that agree in the low word, and unequal bases that agree in the low word: policy_mode "episode" raises, and the
    actor's "auto" falls back to the launch pairs (which draw under the policy's seed and the env's base)."""
    from cm3_amd import Cm3Error
    make, stream = (_cqmix, _explore_stream) if make == "qmix" else (make, _policy_stream)
    lo_seed, lo_base = WK.SEEDS[0] & M32, BASE & M32
    with pytest.raises(Cm3Error, match="seed / env_id_base"):
        run_checkers_policy_collect(make, stream, lo_seed, BASE, E, 2, "episode", policy_seed=WK.SEEDS[0])
    with pytest.raises(Cm3Error, match="seed / env_id_base"):
        run_checkers_policy_collect(make, stream, WK.SEEDS[0], BASE, E, 2, "episode", policy_base=lo_base)
    for kw in (dict(seed=lo_seed, policy_seed=WK.SEEDS[0]), dict(seed=WK.SEEDS[0], policy_base=lo_base)):
        _, v = run_checkers_policy_collect(make, stream, kw.pop("seed"), BASE, E, 2, "auto", **kw)
        assert not v.startswith("k_ck_policy_rollout"), v


# ---- E. the exploration words --------------------------------------------------------------------------------------------------------
def _pqmix(seed, N, episode_kernel=False):
    from cm3_amd.qmix import ParticleQmixAgent
    return ParticleQmixAgent(QR.init_weights(np.random.default_rng(100 + N), N), N, device=DEV, seed=seed, episode_kernel=episode_kernel)


def _cqmix(seed, N, precision="f16x3", base=BASE):
    from cm3_amd.qmix import CheckersQmixAgent
    return CheckersQmixAgent(QC.init_weights(np.random.default_rng(200 + N), N), N, device=DEV, seed=seed, env_id_base=base, precision=precision)


def _explored(seed, ids, clock, greedy, eps):
    """QR.epsilon_greedy per env at the env's own (episode, step)"""
    out = np.zeros_like(greedy, dtype=np.int64)
    for ep, st in sorted(set(zip(clock.episode.tolist(), clock.steps.tolist()))):
        m = (clock.episode == ep) & (clock.steps == st)
        out[m] = QR.epsilon_greedy(greedy[m], seed, ids[m], int(ep), int(st), eps)
    return out


def _explore_stream(seed, ids, clock, actions, q, what, left_out):
    _same(actions, _explored(seed, ids, clock, np.zeros_like(actions), 1.0), what)          # epsilon = 1: every agent explores


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("N", [2, 5])
def test_particle_qmix_act(N, seed):
    ids = WK.ids()
    env = _penv(seed, N)
    env.reset()
    agent = _pqmix(seed, N)
    clock = _Clock(E)
    for t in range(2):
        a = _np(agent.act(env, 1.0))
        assert _variant().startswith("k_qmix_particle<f32,N=%d," % N), _variant()
        _same(a, _explored(seed, ids, clock, np.zeros_like(a), 1.0), ("eps 1", t))
        greedy = _np(agent.act(env, 0.0))
        _same(_np(agent.act(env, 0.3)), _explored(seed, ids, clock, greedy, 0.3), ("eps 0.3", t))
        clock.tick(_np(env.step(torch.as_tensor(a, device=DEV))[5]))


def run_particle_qmix_collect(seed, base, n, N, mode, agent_seed=None):
    from cm3_amd.rollout import ParticleRollout
    ids = WK.ids(base, n)
    env = _penv(seed, N, n, base)
    env.reset()
    agent = _pqmix(seed if agent_seed is None else agent_seed, N, episode_kernel=True)
    ro = ParticleRollout(env, n_ticks=T, policy_mode=mode).collect(policy=agent, epsilon=1.0, reset=False)
    v = _variant()
    clock = _Clock(n)
    for t in range(T):
        a = _np(ro.actions[t])
        _same(a, _explored(agent.seed, ids, clock, np.zeros_like(a), 1.0), ("actions", t))
        clock.tick(_np(ro.done[t]))
    assert clock.episode.min() >= 3
    out = ro.actions.clone(), ro.state.clone()
    ro.close()
    return out, v


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("N,mode,one_launch", [(2, "episode", True), (2, "tick", False), (5, "auto", False)],
                         ids=["N2-one-launch", "N2-pairs", "N5-pairs"])
def test_particle_qmix_collectors(N, mode, one_launch, seed):
    _, v = run_particle_qmix_collect(seed, BASE, E, N, mode)
    assert v.startswith("k_policy_rollout_qmix<f32,N=%d," % N) == one_launch, v


def test_particle_qmix_shard_and_key_mismatch():
    from cm3_amd import Cm3Error
    (fa, fs), _ = run_particle_qmix_collect(WK.SEEDS[0], BASE, E, 2, "episode")
    (ta, ts), _ = run_particle_qmix_collect(WK.SEEDS[0], WK.SHARD_BASE, E - CARRY, 2, "episode")
    assert torch.equal(fa[:, CARRY:], ta) and torch.equal(fs[:, :, CARRY:], ts)
    with pytest.raises(Cm3Error, match="seed"):
        run_particle_qmix_collect(WK.SEEDS[0] & M32, BASE, E, 2, "episode", agent_seed=WK.SEEDS[0])
    _, v = run_particle_qmix_collect(WK.SEEDS[0] & M32, BASE, E, 2, "auto", agent_seed=WK.SEEDS[0])
    assert not v.startswith("k_policy_rollout"), v


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("N", [2, 5])
def test_checkers_qmix_act(N, seed):
    ids = WK.ids()
    env = _ckenv(seed, N)
    env.reset(goal_index=torch.as_tensor(_ck_goals(N)))
    agent = _cqmix(seed, N, "f32", base=0)
    clock = _Clock(E)
    for t in range(2):
        a = _np(agent.act(env, 1.0))
        assert _variant().startswith("k_ck_qmix<"), _variant()
        _same(a, _explored(seed, ids, clock, np.zeros_like(a), 1.0), ("eps 1", t))
        greedy = _np(agent.act(env, 0.0, actions_prev=a))
        _same(_np(agent.act(env, 0.3, actions_prev=a)), _explored(seed, ids, clock, greedy, 0.3), ("eps 0.3", t))
        clock.tick(_np(env.step(torch.as_tensor(a, device=DEV))[6]))


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("N,mode,one_launch", [(2, "episode", True), (2, "tick", False), (5, "auto", False)],
                         ids=["N2-one-launch", "N2-pairs", "N5-pairs"])
def test_checkers_qmix_collectors(N, mode, one_launch, seed):
    _, v = run_checkers_policy_collect(_cqmix, _explore_stream, seed, BASE, E, N, mode)
    assert v.startswith("k_ck_policy_rollout_qmix<") == one_launch, v


def test_checkers_qmix_shard_equals_the_tail_of_the_full_run():
    (fa, fg), _ = run_checkers_policy_collect(_cqmix, _explore_stream, WK.SEEDS[0], BASE, E, 2, "episode")
    (ta, tg), _ = run_checkers_policy_collect(_cqmix, _explore_stream, WK.SEEDS[0], WK.SHARD_BASE, E - CARRY, 2, "episode")
    assert torch.equal(fa[:, CARRY:], ta) and torch.equal(fg[:, CARRY:], tg)


# ---- F. the rows stream --------------------------------------------------------------------------------------------------------------
ROWS = {"particle": (PtRows, 4, None, (BASE,)), "checkers": (CkRows, 2, "int8", (BASE, WK.ROWS_BASE_HIGH))}


def _rows_case(which, seed, precision="f32"):
    cls, N, form, bases = ROWS[which]
    actor = cls.actor(N, precision)
    actor.seed = seed                                           # (the helper builds its actors on a small seed)
    return cls, actor, cls.rows(N, E, form), bases


def _rows_launch(actor, rows, eps, base, draw):
    out = dict(probs=torch.empty(E, 5, dtype=torch.float32, device=DEV), actions=torch.full((E,), -7, dtype=torch.int32, device=DEV),
               onehot=torch.empty(E, 5, dtype=torch.int64, device=DEV))
    actor.enqueue_rows(E, *rows, eps, draw=draw, row_id_base=base, **out)
    torch.cuda.synchronize()
    assert torch.equal(out["onehot"], torch.nn.functional.one_hot(out["actions"].long(), 5))
    return _np(out["actions"]), _np(out["probs"])


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("which", sorted(ROWS))
def test_rows_stream_at_explicit_draws(which, seed):
    cls, actor, rows, bases = _rows_case(which, seed)
    for base in bases:
        for draw in (7, WK.DRAW_LAST):
            u = RR.rows_uniforms(seed, E, draw, base)
            a, p = _rows_launch(actor, rows, 1.0, base, draw)
            assert _variant().startswith(cls.kernel["f32"]) and not _variant().endswith(",counted>"), _variant()
            assert np.all(p == np.float32(0.2))
            _inverse_cdf_same(a[:, None], p, u[:, None], (hex(base), hex(draw), "eps 1"))
        # epsilon 0.3 on the device's own float32 probabilities: the pick is their float32 inverse CDF, every row, nothing left out
        # (as tests/test_gpu_actor_rows.py and tests/test_gpu_actor_checkers_rows.py compare it)
        a, p = _rows_launch(actor, rows, 0.3, base, WK.DRAW_LAST)
        assert np.ptp(p, axis=1).max() > 1e-3
        _same(a, cls.sample(p, RR.rows_uniforms(seed, E, WK.DRAW_LAST, base)), (hex(base), "eps 0.3"))


@pytest.mark.parametrize("seed", WK.SEEDS, ids=["seed-hi-lo", "seed-lo-zero"])
@pytest.mark.parametrize("which", sorted(ROWS))
def test_rows_stream_under_a_device_counter_that_wraps(which, seed):
    from cm3_amd.actor import RowsDrawCounter
    cls, actor, rows, bases = _rows_case(which, seed)
    for base in bases:
        counter = RowsDrawCounter(DEV, 0xFFFFFFFE)
        for k, draw in enumerate((0xFFFFFFFE, 0xFFFFFFFF, 0)):
            a, p = _rows_launch(actor, rows, 1.0, base, counter)
            assert _variant().startswith(cls.kernel["f32"]) and _variant().endswith(",counted>"), _variant()
            _inverse_cdf_same(a[:, None], p, RR.rows_uniforms(seed, E, draw, base)[:, None], (hex(base), k))
        assert counter.value() == 1 and counter.arrivals() == 0


def test_particle_rows_refuse_a_base_the_abi_field_cannot_hold():
    """cm3_actor_rows.row_id_base is an int64_t: a base from 2^63 on is refused by the wrapper, before any launch; the same bits as
    a negative int64 are accepted and draw the stream of the 64-bit pattern."""
    from cm3_amd import Cm3Error
    cls, actor, rows, _ = _rows_case("particle", WK.SEEDS[0])
    out = torch.full((E,), -7, dtype=torch.int32, device=DEV)
    with pytest.raises(Cm3Error, match="row_id_base"):
        actor.enqueue_rows(E, *rows, 1.0, actions=out, draw=0, row_id_base=WK.ROWS_BASE_HIGH)
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    a, p = _rows_launch(actor, rows, 1.0, WK.ROWS_BASE_HIGH - (1 << 64), 3)
    _inverse_cdf_same(a[:, None], p, RR.rows_uniforms(WK.SEEDS[0], E, 3, WK.ROWS_BASE_HIGH)[:, None], "negative int64 base")
