"""GPU: the particle QMIX agent's one-launch rollout (cm3_policy_rollout_qmix_f32; ParticleQmixAgent(..., episode_kernel=True) under
ParticleRollout) -- bit equality with the launch pairs, Q values and choices against the float64 restatement (tests/qmix_ref.py,
teacher-forced on the launch's own observations), routing, the consumers that go through collect(), determinism.

Shapes (N, E): (1, 70), (2, 37), (4, 37), (8, 19) -- more than one workgroup of 64 rows, a ragged last workgroup (E * N % 64 != 0), a
wave with only some of its rows, whole envs per 16-lane tile."""
import numpy as np
import pytest
import torch

from tests import qmix_ref as QR
from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu

SHAPES = [(1, 70), (2, 37), (4, 37), (8, 19)]
SEED = 11


def _cfg(N):
    return {1: "particle_stage1.json", 2: "particle_stage2_merge.json", 9: "particle_ring10.json",
            10: "particle_ring10.json"}.get(N, "particle_merge8.json")


def _env(E, N, dtype=torch.float32, max_steps=33, seed=SEED, **kw):
    from cm3_amd.particle import VecParticleEnv
    return VecParticleEnv(load_cfg(_cfg(N)), N, 0.2, max_steps, E, device="cuda:0", dtype=dtype, seed=seed, **kw)


def _weights(N):
    return QR.init_weights(np.random.default_rng(100 + N), N)


def _agent(N, seed=SEED, episode_kernel=True):
    from cm3_amd.qmix import ParticleQmixAgent
    return ParticleQmixAgent(_weights(N), N, device="cuda:0", seed=seed, episode_kernel=episode_kernel)


def _snapshot(ro, env):
    """Every array a collect() leaves behind, cloned."""
    out = dict(state=ro.state, obs_others=ro.obs_others, goals=ro.goals, actions=ro.actions, reward=ro.reward,
               reward_n=ro.reward_n, done=ro.done, collisions=ro.collisions, meta=env._meta, episode=env._episode,
               env_state=env._state[env._cur], env_obs=env._obs_others[env._cur], env_goals=env._goals)
    if ro.auto_reset:
        d = ro.done.bool()
        out["term_state"] = ro.term_state * d[:, None, :, None]            # (the capture is defined where an episode ended)
        out["term_obs_others"] = ro.term_obs_others * d[:, :, None, None]
    return {k: v.clone() for k, v in out.items() if v is not None}       # (goals: None for an episode-synchronous collector)


def _collect(N, E, mode, eps, auto_reset, max_steps, T, collects=1, env_id_base=0):
    from cm3_amd import _lib
    from cm3_amd.rollout import ParticleRollout
    env = _env(E, N, max_steps=max_steps, auto_reset=auto_reset, env_id_base=env_id_base)
    env.reset()
    agent = _agent(N)
    ro = ParticleRollout(env, n_ticks=T, policy_mode=mode)
    if isinstance(eps, torch.Tensor):
        eps = eps.clone()
    snaps, names = [], []
    for _ in range(collects):
        ro.collect(policy=agent, epsilon=eps, reset=False)
        names.append(_lib.last_kernel_variant())
        torch.cuda.synchronize()
        snaps.append(_snapshot(ro, env))
    ro.close()
    return snaps, names


def _assert_same(one, pairs):
    assert len(one) == len(pairs)
    for k, (a, b) in enumerate(zip(one, pairs)):
        assert a.keys() == b.keys()
        for name in a:
            assert torch.equal(a[name], b[name]), (k, name)


# ---- 1. equality with the launch pairs -------------------------------------------------------------------------------------------
CASES = {"a_resets": dict(auto_reset=True, max_steps=5, T=12, collects=1),
         "b_synchronous": dict(auto_reset=False, max_steps=33, T=10, collects=1),
         "c_two_collects": dict(auto_reset=True, max_steps=7, T=5, collects=2)}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("N,E", SHAPES)
def test_one_launch_equals_the_launch_pairs(N, E, case):
    """state, obs_others, goals, actions, reward, reward_n, done, per-tick collisions, the terminal captures, and the env's meta /
    episode / current buffers afterwards: bit for bit what the agent / step launch pairs write, at epsilon 0.3.  (a) several
    same-tick resets inside the launch; (b) episode-synchronous; (c) a second collect without a reset, so the launch starts from
    non-zero steps / episode."""
    kw = CASES[case]
    one, names = _collect(N, E, "episode", 0.3, **kw)
    pairs, pnames = _collect(N, E, "tick", 0.3, **kw)
    assert all(n.startswith("k_policy_rollout_qmix<f32,N=%d," % N) for n in names), names
    assert not any(n.startswith("k_policy_rollout") for n in pnames), pnames
    if kw["auto_reset"]:
        assert int(one[-1]["done"].sum()) > 0 and int(one[-1]["episode"].max()) >= 1        # resets fell inside the launch
    if kw["collects"] == 2:
        assert not torch.equal(one[0]["actions"], one[1]["actions"])
    _assert_same(one, pairs)


# ---- 2. epsilon -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", ["0.0", "1.0", "device"])
def test_one_launch_equals_the_launch_pairs_at_other_epsilons(eps):
    N, E = 4, 37
    value = torch.tensor(0.3, dtype=torch.float32, device="cuda:0") if eps == "device" else float(eps)
    kw = dict(auto_reset=True, max_steps=5, T=12)
    one, _ = _collect(N, E, "episode", value, **kw)
    pairs, _ = _collect(N, E, "tick", value, **kw)
    _assert_same(one, pairs)
    if eps == "device":                                       # a device epsilon is read, not ignored: the bits of epsilon = 0.3
        ref, _ = _collect(N, E, "episode", 0.3, **kw)
        _assert_same(one, ref)
        zero, _ = _collect(N, E, "episode", 0.0, **kw)
        assert not torch.equal(one[0]["actions"], zero[0]["actions"])


# ---- 3. against the float64 restatement, teacher-forced ------------------------------------------------------------------------
@pytest.mark.parametrize("N,E", SHAPES)
def test_q_values_and_choices_match_the_float64_restatement(N, E):
    """For every tick t the restatement's Q values on the float32-rounded slot-t observation match the launch's q_values[t] within
    2e-5 * max(1, |q|max) (the bound the launch-pair agent is held to, test_gpu_qmix_particle._check_q), and on clearly decided rows
    (top-two gap > 1e-4, more than 0.9 of every tick's rows) the action is the restatement's epsilon-greedy choice for the per-tick
    (episode, steps) counters rebuilt from `done`."""
    from cm3_amd import _lib
    from cm3_amd.rollout import ParticleRollout
    T, eps, base = 12, 0.3, 5
    env = _env(E, N, max_steps=5, auto_reset=True, env_id_base=base)
    env.reset()
    agent, w = _agent(N), _weights(N)
    ro = ParticleRollout(env, n_ticks=T)
    episode = env._episode.cpu().numpy().astype(np.int64)
    steps = env._meta[:, 0].cpu().numpy().astype(np.int64)
    q_dev = torch.full((T, E, N, 5), float("nan"), dtype=torch.float32, device="cuda:0")
    ro._load_slot0()
    env._desc.flags = _lib.FLAG_AUTO_RESET
    agent.enqueue_episode(env._desc, ro._traj(0), E, T, eps, q_values=q_dev, stream=env._stream())
    torch.cuda.synchronize()
    assert _lib.last_kernel_variant().startswith("k_policy_rollout_qmix<f32,N=%d," % N)
    f = lambda t: t.double().cpu().numpy()  # noqa: E731
    done = ro.done.cpu().numpy().astype(bool)
    actions = ro.actions.cpu().numpy()
    q_all = f(q_dev)
    assert np.isfinite(q_all).all()
    ids = base + np.arange(E)
    for t in range(T):
        oo = f(ro.obs_others[t]).reshape(E * N, env.L)
        vo = f(ro.state[t].permute(1, 0, 2)).reshape(E * N, 4)
        vg = f(ro._goals_buf[t].permute(1, 0, 2)).reshape(E * N, 2)
        ref = QR.q_values(w, oo, vo, vg)
        q = q_all[t].reshape(E * N, 5)
        bound = 2e-5 * np.maximum(1.0, np.abs(ref).max(axis=1))
        err = np.abs(q - ref).max(axis=1)
        assert (err <= bound).all(), (t, float((err / bound).max()))
        top2 = np.sort(ref, axis=1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0] > 1e-4).reshape(E, N)
        assert clear.mean() > 0.9, (t, float(clear.mean()))
        want = QR.epsilon_greedy(np.argmax(ref, axis=1).reshape(E, N), SEED, ids, episode, steps, eps)
        assert np.array_equal(actions[t][clear], want[clear]), t
        episode, steps = episode + done[t], np.where(done[t], 0, steps + 1)
    assert done.any()
    assert np.array_equal(env._episode.cpu().numpy(), episode) and np.array_equal(env._meta[:, 0].cpu().numpy(), steps)
    ro.close()


# ---- 4. routing -------------------------------------------------------------------------------------------------------------------
def _variant_of(env, agent, **kw):
    from cm3_amd import _lib
    from cm3_amd.rollout import ParticleRollout
    ro = ParticleRollout(env, n_ticks=3, **kw)
    try:
        ro.collect(policy=agent, epsilon=0.1)
        v = _lib.last_kernel_variant()
        torch.cuda.synchronize()
    finally:
        ro.close()
    return v


def test_routing_with_and_without_the_flag():
    from cm3_amd import Cm3Error
    N, E = 4, 37
    agent = _agent(N)
    for mode in ("episode", "auto"):
        v = _variant_of(_env(E, N), agent, policy_mode=mode)
        assert v.startswith("k_policy_rollout_qmix<f32,N=4,"), (mode, v)
    seen = []
    orig = agent.enqueue

    def spy(*a, **k):
        from cm3_amd import _lib
        orig(*a, **k)
        seen.append(_lib.last_kernel_variant())
    agent.enqueue = spy
    v = _variant_of(_env(E, N), agent, policy_mode="tick", use_graph=False)
    agent.enqueue = orig
    assert seen and all(s.startswith("k_qmix_particle<f32,N=4,") for s in seen), seen
    assert not v.startswith("k_policy_rollout"), v
    # not eligible: "episode" names the reason, "auto" runs the launch pairs
    refusals = [(_env(E, N, dtype=torch.float64), agent, "float32"),
                (_env(E, 3), _agent(3), "{1, 2, 4, 8}"),
                (_env(E, N, seed=SEED + 1), agent, "seed")]
    for env, ag, word in refusals:
        with pytest.raises(Cm3Error) as e:
            _variant_of(env, ag, policy_mode="episode")
        assert word in str(e.value), str(e.value)
        v = _variant_of(env, ag, policy_mode="auto")
        assert not v.startswith("k_policy_rollout"), v
    with pytest.raises(Cm3Error) as e:
        _variant_of(_env(E, 2), agent, policy_mode="episode")
    assert "agent count" in str(e.value)
    # the CM3 actor's fused kernels stay refused, flag or not; a default agent is refused under "episode" as before
    for kw in (dict(fused=True), dict(fused_policy_tick=True)):
        with pytest.raises(Cm3Error):
            _variant_of(_env(E, N), agent, **kw)
    plain = _agent(N, episode_kernel=False)
    with pytest.raises(Cm3Error):
        _variant_of(_env(E, N), plain, policy_mode="episode")
    v = _variant_of(_env(E, N), plain, policy_mode="auto")
    assert not v.startswith("k_policy_rollout"), v


# ---- 5. consumers -----------------------------------------------------------------------------------------------------------------
def test_replay_and_evaluation_give_the_tensors_of_the_launch_pairs():
    from cm3_amd.evaluate import test_particle as evaluate_particle
    from cm3_amd.replay import DeviceReplayBuffer, off_policy_batches
    from cm3_amd.rollout import ParticleRollout
    N, E, T = 4, 37, 6
    out = {}
    for mode in ("auto", "tick"):
        agent = _agent(N)
        env = _env(E, N, auto_reset=True, max_steps=5)
        env.reset()
        ro = ParticleRollout(env, n_ticks=T, policy_mode=mode)
        buf = DeviceReplayBuffer(4 * E * T, device="cuda:0")
        g = torch.Generator(device="cuda:0").manual_seed(0)
        batches = [{k: v.clone() for k, v in b.items()}
                   for b in off_policy_batches(ro, buf, 3, batch_size=64, generator=g, policy=agent, epsilon=0.1)]
        assert len(batches) == 3 and len(buf) == 3 * E * T
        ring = {k: v.clone() for k, v in buf.cols.items()}
        ro.close()
        ev = _env(E, N, max_steps=33)
        ro = ParticleRollout(ev, policy_mode=mode)
        r_local, r_global, n = evaluate_particle(ev, agent, n_rounds=1, rollout=ro)
        ro.close()
        out[mode] = (batches, ring, r_local, r_global, n)
    (b1, ring1, l1, g1, n1), (b2, ring2, l2, g2, n2) = out["auto"], out["tick"]
    for x, y in zip(b1, b2):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), k
    assert ring1.keys() == ring2.keys() and all(torch.equal(ring1[k], ring2[k]) for k in ring1)
    assert n1 == n2 == E and np.array_equal(l1, l2) and g1 == g2


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------------
def test_two_collects_from_the_same_state_are_identical():
    N, E = 8, 19
    kw = dict(auto_reset=True, max_steps=5, T=12)
    a, _ = _collect(N, E, "episode", 0.3, **kw)
    b, _ = _collect(N, E, "episode", 0.3, **kw)
    _assert_same(a, b)
