"""GPU: the Checkers QMIX agent's whole rollout in ONE launch (cm3_policy_rollout_checkers_qmix, CheckersRollout(env,
policy_mode="episode")) -- bit for bit what the agent + step launch pairs write (restarts inside the launch, a ragged and a lone
partial workgroup, both agent counts, a second collect() that continues the first), teacher-forced against the float64
restatement with the exploration stream recomputed on the host, which kernel a collection runs, what is refused, replay and
determinism."""
import numpy as np
import pytest
import torch

from tests import qmix_checkers_ref as QC
from tests import qmix_ref as QR
from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu

_TRAJ = ("actions", "probs", "grid", "vec", "obs_others", "obs_self_t", "obs_self_v", "local_rewards", "reward", "done")
_TERM = ("term_grid", "term_vec", "term_obs_others", "term_obs_self_t", "term_obs_self_v", "goal_slots")
_CUR = ("grid_raw", "obs_self_t_raw", "vec", "obs_others", "obs_self_v", "actions")


def _agent(N, precision="f16x3", seed=12341, **kw):
    from cm3_amd.qmix import CheckersQmixAgent
    w = QC.init_weights(np.random.default_rng(200 + N), N)
    return CheckersQmixAgent(w, N, device="cuda:0", seed=seed, precision=precision, **kw), w


def _env(E, N, seed=12341, max_steps=33, **kw):
    from cm3_amd.checkers import VecCheckersEnv
    cfg = load_cfg("checkers_stage%d.json" % (1 if N == 1 else 2))
    init = cfg["init"]
    if N > 2:                                  # (only the refusal test: any distinct start cells inside the band)
        init = dict(init, agents_r=[k % 3 for k in range(N)], agents_c=[8 - k // 3 for k in range(N)])
    return VecCheckersEnv(init, N, max_steps, E, device="cuda:0", seed=seed, **kw)


def _goals(rng, E, N):
    return np.eye(2)[rng.integers(0, 2, (E, N))] if N == 1 else np.broadcast_to(np.eye(N), (E, N, 2)).copy()


def _snapshot(ro, env):
    snap = {k: getattr(ro, k).clone() for k in _TRAJ}
    if ro.auto_reset:
        snap.update({k: getattr(ro, k).clone() for k in _TERM})
    cur = env._slots[env._cur]
    snap.update({"cur_" + k: cur[k].clone() for k in _CUR})
    snap.update(mask=env._mask.clone(), agents=env._agents.clone(), steps=env._steps.clone(), episode=env._episode.clone(),
                goals=env._goals.clone(), prev0=ro.prev0.clone())
    return snap


def _collect(N, E, auto_reset, max_steps, T, mode, eps=0.2, seed=31, collects=2):
    """-> (one snapshot of every array per collect(), the last kernel variant)"""
    from cm3_amd import _lib
    from cm3_amd.rollout import CheckersRollout
    env = _env(E, N, seed=seed, max_steps=max_steps, auto_reset=auto_reset)
    agent, _ = _agent(N, seed=seed)
    ro = CheckersRollout(env, n_ticks=T, policy_mode=mode, record_probs=True)
    if eps == "device":
        eps = torch.full((1,), 0.2, dtype=torch.float32, device="cuda:0")
    rng = np.random.default_rng(1)
    snaps = []
    for _ in range(collects):
        ro.collect(_goals(rng, E, N), policy=agent, epsilon=eps)
        torch.cuda.synchronize()
        snaps.append(_snapshot(ro, env))
    name = _lib.last_kernel_variant()
    ro.close()
    return snaps, name


def _assert_equal(got, want):
    for k, (a, b) in enumerate(zip(got, want)):
        assert set(a) == set(b)
        for name in a:
            assert torch.equal(a[name], b[name]), "collect %d: %s differs" % (k, name)


# ---- 1. bit-equal to the launch pairs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E,auto_reset,max_steps,T", [
    (2, 200, False, 33, 33),          # seven workgroups of 32 envs, the last one ragged; one reference episode per env and collect()
    (2, 200, True, 9, 33),            # restarts inside the launch: terminal capture, fresh record, actions_prev = zeros
    (1, 150, False, 33, 33),          # one agent (64 envs per workgroup, ragged): the others table row is the agent's OWN cell
    (1, 150, True, 7, 20),            # ... with restarts: a fresh random goal per episode picks the start row
    (2, 5, True, 9, 20),              # fewer envs than one workgroup
])
def test_one_launch_rollout_equals_the_launch_pairs(N, E, auto_reset, max_steps, T):
    """Every array of two consecutive collect()s -- actions, recorded Q values, every observation slot, rewards, done, terminal
    captures, goal slots, the env's current-observation buffers, the live state, prev0 -- under policy_mode "episode" and "tick"."""
    one, name = _collect(N, E, auto_reset, max_steps, T, "episode")
    pairs, pname = _collect(N, E, auto_reset, max_steps, T, "tick")
    assert name.startswith("k_ck_policy_rollout_qmix<") and (",N=%d," % N) in name, name
    assert not pname.startswith("k_ck_policy_rollout"), pname
    _assert_equal(one, pairs)
    assert len(torch.unique(one[0]["actions"])) == 5 and float(one[0]["probs"].abs().max()) > 0
    if auto_reset:
        restarts = sum(s["done"].to(torch.int64).sum(0) for s in one)
        assert int(restarts.min()) >= 2, restarts          # every env restarted at least twice inside the launches


@pytest.mark.parametrize("eps", [0.0, 1.0, "device"])
def test_one_launch_rollout_equals_the_launch_pairs_at_other_epsilons(eps):
    """The two-agent restart case always greedy, always exploring, and with epsilon read from a one-element device tensor."""
    one, _ = _collect(2, 200, True, 9, 33, "episode", eps=eps)
    pairs, _ = _collect(2, 200, True, 9, 33, "tick", eps=eps)
    _assert_equal(one, pairs)
    restarts = sum(s["done"].to(torch.int64).sum(0) for s in one)
    assert int(restarts.min()) >= 2


# ---- 2. teacher-forced against the float64 restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2])
def test_one_launch_rollout_teacher_forced_against_float64(N):
    """At every tick the restatement is fed the rollout's OWN slot-t inputs: Q within 2e-5 (relative to max(1, max|Q|): the bound
    the stand-alone kernel is held to) on ALL rows; explored rows take rand5 of the recomputed action word; unexplored rows whose
    top two reference Q values are 1e-4 apart take the argmax; those clear rows are more than 0.9 of every tick's rows (the
    restatement alone keeps that on these weights: tests/test_qmix_checkers_rollout_abi.py)."""
    from cm3_amd.rollout import CheckersRollout
    from oracle import philox
    E, T, eps, seed, S = 128, 33, 0.3, 53, 12
    rows = E * N
    env = _env(E, N, seed=seed, max_steps=S, auto_reset=True)
    agent, w = _agent(N, seed=seed)
    ro = CheckersRollout(env, n_ticks=T, policy_mode="episode", record_probs=True)
    ro.collect(_goals(np.random.default_rng(2), E, N), policy=agent, epsilon=eps)
    torch.cuda.synchronize()
    done = ro.done.cpu().numpy().astype(np.int64)                                  # [T, E]
    # (episode, step) of every tick from the counters the launch left and the done flags: a restart adds one episode and zeroes the step
    later = np.cumsum(done[::-1], axis=0)[::-1]                                    # dones at ticks >= t
    episode = env._episode.cpu().numpy()[None, :] - later
    step = np.zeros((T + 1, E), np.int64)
    for t in range(T):
        step[t + 1] = np.where(done[t] != 0, 0, step[t] + 1)
    assert np.array_equal(step[T], env._steps.cpu().numpy()) and done.sum(0).min() >= 2
    worst, explored_rows = 0.0, 0
    for t in range(T):
        ref = QC.q_values(w, ro.actions_prev_at(t).cpu().numpy().reshape(rows),
                          ro.obs_self_t[t].cpu().numpy().astype(np.float64).reshape(rows, 5, 5, 3),
                          ro.obs_self_v[t].cpu().numpy().reshape(rows, 4), ro.obs_others[t].cpu().numpy().reshape(rows, -1),
                          ro.goals_at(t).cpu().numpy().reshape(rows, 2))
        q = ro.probs[t].cpu().numpy().astype(np.float64).reshape(rows, 5)
        rel = np.abs(q - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))
        print("N=%d tick %2d worst |Q - float64| / max(1, max|Q|) %.2e" % (N, t, rel.max()))
        worst = max(worst, float(rel.max()))
        assert rel.max() <= 2e-5, (t, float(rel.max()))
        we, wa = QR.explore_words(seed, np.arange(E), episode[t], step[t], N)
        explored = (philox.u01(we) < float(np.float32(eps))).reshape(rows)
        a = ro.actions[t].cpu().numpy().reshape(rows)
        assert np.array_equal(a[explored], philox.rand5(wa).reshape(rows)[explored]), t
        top2 = np.sort(ref, axis=1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > 1e-4
        assert clear.mean() > 0.9, (t, float(clear.mean()))
        sel = clear & ~explored
        assert np.array_equal(a[sel], np.argmax(ref, axis=1)[sel]), t
        explored_rows += int(explored.sum())
    assert abs(explored_rows / (T * rows) - eps) < 5 * np.sqrt(eps * (1 - eps) / (T * rows))
    print("N=%d worst over the rollout %.2e" % (N, worst))
    ro.close()


# ---- 3. which kernel ran ---------------------------------------------------------------------------------------------------------
def test_episode_mode_runs_the_one_launch_kernels():
    from cm3_amd import _lib
    from cm3_amd.actor import CheckersActor
    from cm3_amd.rollout import CheckersRollout
    from oracle import actor_checkers_oracle as AO
    E, N, seed, T = 96, 2, 12341, 6
    env = _env(E, N, seed=seed)
    agent, _ = _agent(N, seed=seed)
    ro = CheckersRollout(env, n_ticks=T, policy_mode="episode")
    calls = []
    agent.enqueue = lambda *a, **k: calls.append(1)
    ro.collect(np.eye(2), policy=agent, epsilon=0.1)
    v = _lib.last_kernel_variant()
    torch.cuda.synchronize()
    assert not calls
    assert v.startswith("k_ck_policy_rollout_qmix<") and ",N=2," in v, v
    assert ro._actor_graph.graph is None                                 # nothing was captured: one plain launch
    actor = CheckersActor(AO.init_weights(np.random.default_rng(0), N), N, device="cuda:0", seed=seed, precision="f16x3")
    ro.collect(np.eye(2), policy=actor, epsilon=0.1)
    v = _lib.last_kernel_variant()
    torch.cuda.synchronize()
    assert v.startswith("k_ck_policy_rollout<") and ",N=2," in v, v
    ro.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_episode_mode_refuses_what_the_kernel_does_not_cover():
    """Each one a Cm3Error out of collect() that names the condition, before the env is reset or anything is launched."""
    from cm3_amd import Cm3Error, _lib
    from cm3_amd.rollout import CheckersRollout
    E, seed = 64, 9
    cases = [(2, dict(precision="f32", seed=seed), "precision"), (3, dict(seed=seed), "agent count"),
             (2, dict(seed=seed + 1), "seed / env_id_base"), (2, dict(seed=seed, env_id_base=64), "seed / env_id_base")]
    for N, kw, needle in cases:
        env = _env(E, N, seed=seed)
        agent, _ = _agent(N, **kw)
        ro = CheckersRollout(env, n_ticks=4, policy_mode="episode")
        launched = []
        ro._enqueue_policy_rollout = lambda *a, **k: launched.append(1)
        env.reset = lambda *a, **k: launched.append(2)
        before = _lib.last_kernel_variant()
        with pytest.raises(Cm3Error, match=needle):
            ro.collect(np.eye(N, 2), policy=agent, epsilon=0.1)
        assert not launched and _lib.last_kernel_variant() == before
        ro.close()
    with pytest.raises(Cm3Error, match="policy_mode"):
        CheckersRollout(_env(E, 2, seed=seed), policy_mode="bogus")


def test_episode_mode_leaves_random_and_host_policies_alone():
    """policy=None and a host callable behave under "episode" as under "auto"."""
    from cm3_amd.rollout import CheckersRollout
    E, N, T = 64, 2, 5
    host = lambda prev, oo, ot, ov, g: torch.ones(E, N, dtype=torch.int32)  # noqa: E731
    out = {}
    for mode in ("episode", "auto"):
        env = _env(E, N, seed=3)
        ro = CheckersRollout(env, n_ticks=T, policy_mode=mode)
        ro.collect(np.eye(2))
        a = ro.actions.clone()
        ro.collect(np.eye(2), policy=host)
        out[mode] = (a, ro.actions.clone(), ro.grid.clone(), ro.reward.clone())
        ro.close()
    for x, y in zip(out["episode"], out["auto"]):
        assert torch.equal(x, y)
    assert bool((out["episode"][1] == 1).all())


# ---- 5. replay -------------------------------------------------------------------------------------------------------------------
def test_off_policy_batches_are_the_launch_pairs_batches():
    from cm3_amd.replay import DeviceReplayBuffer, off_policy_batches
    from cm3_amd.rollout import CheckersRollout
    E, N, T, chunks = 96, 2, 10, 3
    got = {}
    for mode in ("episode", "tick"):
        agent, _ = _agent(N, seed=4)
        env = _env(E, N, seed=4, auto_reset=True)
        ro = CheckersRollout(env, n_ticks=T, policy_mode=mode)
        buf = DeviceReplayBuffer(size=100000, device="cuda:0")
        g = torch.Generator(device="cuda:0").manual_seed(0)
        batches = [{k: v.clone() for k, v in b.items()}
                   for b in off_policy_batches(ro, buf, chunks, batch_size=128, generator=g, goals=np.eye(2), policy=agent, epsilon=0.1)]
        assert len(buf) == chunks * E * T
        got[mode] = (batches, {k: v[:len(buf)].clone() for k, v in buf.all().items()})
        ro.close()
    for a, b in zip(got["episode"][0], got["tick"][0]):
        assert set(a) == set(b) == set(CheckersRollout.ORDER)
        for name in a:
            assert torch.equal(a[name], b[name]), name
    for name, v in got["episode"][1].items():
        assert torch.equal(v, got["tick"][1][name]), name


# ---- 6. determinism --------------------------------------------------------------------------------------------------------------
def test_one_launch_rollout_is_deterministic():
    a, _ = _collect(2, 200, True, 9, 33, "episode", collects=3, seed=77)
    b, _ = _collect(2, 200, True, 9, 33, "episode", collects=3, seed=77)
    _assert_equal(a, b)
    assert not torch.equal(a[0]["actions"], a[1]["actions"])
