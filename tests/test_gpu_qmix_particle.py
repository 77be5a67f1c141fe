"""GPU: the on-device QMIX agent (cm3_qmix_particle_f32 / _f64, cm3_amd.qmix.ParticleQmixAgent) -- Q values against the float64
restatement (tests/qmix_ref.py) and the reference-recorded fixture, the epsilon-greedy law and its stream, the captured rollout
graph under annealing, rollout / evaluation / replay parity with a host loop of agent.act + env.step."""
import numpy as np
import pytest
import torch

from tests import qmix_ref as QR
from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu


def _cfg(N):
    return {1: "particle_stage1.json", 2: "particle_stage2_merge.json", 9: "particle_ring10.json",
            10: "particle_ring10.json"}.get(N, "particle_merge8.json")


def _env(E, N, dtype=torch.float32, max_steps=33, seed=11, **kw):
    from cm3_amd.particle import VecParticleEnv
    return VecParticleEnv(load_cfg(_cfg(N)), N, 0.2, max_steps, E, device="cuda:0", dtype=dtype, seed=seed, **kw)


def _agent(N, seed=11, wseed=None, scale=1.0):
    from cm3_amd.qmix import ParticleQmixAgent
    w = QR.init_weights(np.random.default_rng(100 + N if wseed is None else wseed), N, scale=scale)
    return ParticleQmixAgent(w, N, device="cuda:0", seed=seed), w


def _inputs(env):
    """float64 inputs [E*N, .] of the env's current observation, rounded to float32 first (what the agent stages)."""
    cur = env._cur
    f = lambda t: t.float().double().cpu().numpy()  # noqa: E731
    oo = f(env._obs_others[cur]).reshape(env.E * env.n, env.L)
    vo = f(env._state[cur].permute(1, 0, 2)).reshape(-1, 4)
    vg = f(env._goals.permute(1, 0, 2)).reshape(-1, 2)
    return oo, vo, vg


def _check_q(q_dev, a_dev, ref):
    q = q_dev.reshape(-1, 5).double().cpu().numpy()
    a = a_dev.reshape(-1).cpu().numpy()
    bound = 2e-5 * np.maximum(1.0, np.abs(ref).max(axis=1))
    assert (np.abs(q - ref).max(axis=1) <= bound).all(), float((np.abs(q - ref).max(axis=1) / bound).max())
    top2 = np.sort(ref, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-4
    assert clear.mean() > 0.9
    assert np.array_equal(a[clear], np.argmax(ref, axis=1)[clear])


# ---- 1. Q values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("N", list(range(1, 11)))
def test_q_values_match_the_float64_restatement(N, dtype):
    from cm3_amd import _lib
    E = 333                                                  # E * N rows: the last workgroup is ragged for every N
    assert (E * N) % 64 != 0
    env = _env(E, N, dtype=dtype, env_id_base=5)
    env.reset()
    for _ in range(3):
        env.step()
    agent, w = _agent(N)
    a, q = agent.act(env, 0.0, return_q=True)
    torch.cuda.synchronize()
    v = _lib.last_kernel_variant()
    assert v.startswith("k_qmix_particle<%s,N=%d," % ("f32" if dtype == torch.float32 else "f64", N)), v
    assert q.shape == (E, N, 5) and a.shape == (E, N) and a.dtype == torch.int32
    _check_q(q, a, QR.q_values(w, *_inputs(env)))


@pytest.mark.parametrize("N", [1, 4, 8, 10])
def test_q_values_on_the_reference_recorded_fixture(N, golden_dir):
    import os
    from cm3_amd.qmix import ParticleQmixAgent
    z = np.load(os.path.join(golden_dir, "qmix_particle.npz"))
    tag = "n%d" % N
    w = {str(k): z[tag + "/w/" + str(k)] for k in z[tag + "/names"]}
    oo, vo, vg = (z[tag + "/in/" + k] for k in ("obs_others", "v_obs", "v_goal"))
    rows = vo.shape[0]
    E = rows // N
    agent = ParticleQmixAgent(w, N, device="cuda:0")
    dev = lambda x: torch.as_tensor(x, device="cuda:0").contiguous()  # noqa: E731
    actions = torch.empty(E, N, dtype=torch.int32, device="cuda:0")
    q = torch.empty(E, N, 5, dtype=torch.float32, device="cuda:0")
    zeros = torch.zeros(E, 2, dtype=torch.int32, device="cuda:0")
    agent.enqueue(E, dev(oo.reshape(E, N, -1)), dev(vo.reshape(E, N, 4).transpose(1, 0, 2)), dev(vg.reshape(E, N, 2).transpose(1, 0, 2)),
                  zeros, zeros[:, 0].contiguous(), actions, 0.0, q)
    torch.cuda.synchronize()
    assert np.abs(q.reshape(-1, 5).cpu().numpy() - z[tag + "/q"]).max() < 2e-5 * max(1.0, float(np.abs(z[tag + "/q"]).max()))
    _check_q(q, actions, QR.q_values(w, oo, vo, vg))
    assert np.array_equal(actions.reshape(-1).cpu().numpy(), z[tag + "/argmax"])


# ---- 2. the epsilon-greedy law -------------------------------------------------------------------------------------------------
def _chi2_uniform(x):
    c = np.bincount(np.asarray(x).ravel(), minlength=5).astype(np.float64)
    e = c.sum() / 5
    return float(((c - e) ** 2 / e).sum())


def test_epsilon_greedy_law_and_stream():
    E, N, seed = 65536, 4, 11                                 # 2^18 rows
    env = _env(E, N, env_id_base=0, seed=seed)
    env.reset()
    for _ in range(2):
        env.step()
    agent, _ = _agent(N, seed=seed, scale=2.0)
    greedy = agent.act(env, 0.0).cpu().numpy()
    assert len(np.unique(greedy)) > 1
    ep, st = env._episode.cpu().numpy(), env._meta[:, 0].cpu().numpy()
    ids = np.arange(E)
    # epsilon = 1: uniform (chi^2, 4 degrees of freedom: 40 is p ~ 5e-8)
    a1 = agent.act(env, 1.0).cpu().numpy()
    assert _chi2_uniform(a1) < 40
    assert np.array_equal(a1, QR.epsilon_greedy(greedy, seed, ids, ep, st, 1.0))
    # epsilon = 0.3: a non-greedy fraction of 0.3 * 4/5, explored actions uniform
    a3 = agent.act(env, 0.3).cpu().numpy()
    p, n = 0.3 * 4 / 5, a3.size
    assert abs(np.mean(a3 != greedy) - p) < 5 * np.sqrt(p * (1 - p) / n)
    we, _ = QR.explore_words(seed, ids, ep, st, N)
    explored = (we.astype(np.float64) + 0.5) / 2.0 ** 32 < np.float32(0.3)
    assert abs(explored.mean() - 0.3) < 5 * np.sqrt(0.21 / n)
    assert _chi2_uniform(a3[explored]) < 40
    assert np.array_equal(a3, QR.epsilon_greedy(greedy, seed, ids, ep, st, 0.3))
    # the same launch twice: the same actions; another episode or step: other draws
    assert np.array_equal(agent.act(env, 0.3).cpu().numpy(), a3)
    saved_ep, saved_meta = env._episode.clone(), env._meta.clone()
    env._episode += 1
    a_ep = agent.act(env, 0.3).cpu().numpy()
    env._episode.copy_(saved_ep)
    env._meta[:, 0] += 1
    a_st = agent.act(env, 0.3).cpu().numpy()
    env._meta.copy_(saved_meta)
    for other in (a_ep, a_st):
        assert np.mean(other != a3) > 0.2
    # two shards with env_id_base reproduce the single-process actions
    cur, h = env._cur, E // 2
    parts = []
    for lo, hi in ((0, h), (h, E)):
        out = torch.empty(hi - lo, N, dtype=torch.int32, device="cuda:0")
        agent.enqueue(hi - lo, env._obs_others[cur][lo:hi].contiguous(), env._state[cur][:, lo:hi].contiguous(),
                      env._goals[:, lo:hi].contiguous(), env._meta[lo:hi].contiguous(), env._episode[lo:hi].contiguous(), out, 0.3,
                      env_id_base=lo)
        parts.append(out.cpu().numpy())
    assert np.array_equal(np.concatenate(parts), a3)
    # epsilon = 0: greedy throughout
    assert np.array_equal(agent.act(env, 0.0).cpu().numpy(), greedy)


# ---- 3. annealing inside the captured graph ------------------------------------------------------------------------------------
def test_agent_graph_follows_annealed_epsilon_without_recapture():
    from cm3_amd.rollout import ParticleRollout
    E, N, T = 200, 4, 12
    outs = []
    for graph in (True, False):
        env = _env(E, N, seed=12341, auto_reset=True, max_steps=7)
        env.reset()
        agent, _ = _agent(N, seed=12341)
        ro = ParticleRollout(env, n_ticks=T, use_graph=graph)
        handles, acts = [], []
        for eps in (0.5, 0.3, 0.05):
            ro.collect(policy=agent, epsilon=eps, reset=False)
            acts.append(ro.actions.clone())
            handles.append(ro._actor_graph.graph.value if graph else None)
        outs.append((acts, handles, ro))
    for a, b in zip(outs[0][0], outs[1][0]):
        assert torch.equal(a, b)
    assert len(set(outs[0][1])) == 1
    assert not torch.equal(outs[0][0][0], outs[0][0][2])
    for _, _, ro in outs:
        ro.close()


# ---- 4. rollout parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("N", [1, 3, 4, 8, 10])
def test_rollout_equals_host_loop(N, dtype, auto_reset, graph):
    from cm3_amd.rollout import ParticleRollout
    E, seed, eps, S = 300, 7, 0.2, 9
    T = 33 if not auto_reset else 20
    agent, _ = _agent(N, seed=seed)
    env_a = _env(E, N, dtype=dtype, seed=seed, auto_reset=auto_reset, max_steps=S if auto_reset else 33)
    env_b = _env(E, N, dtype=dtype, seed=seed, auto_reset=auto_reset, max_steps=S if auto_reset else 33)
    env_a.reset()
    env_b.reset()
    if auto_reset:
        env_b.enable_terminal_capture()
    ro = ParticleRollout(env_a, n_ticks=T, use_graph=graph, live_state=False)
    ro.collect(policy=agent, epsilon=eps, reset=False)
    torch.cuda.synchronize()
    assert torch.equal(ro.state[0], env_b._state[env_b._cur]) and torch.equal(ro.obs_others[0], env_b._obs_others[env_b._cur])
    for t in range(T):
        a = agent.act(env_b, eps)
        assert torch.equal(a, ro.actions[t]), t
        _, _, _, rew, rew_n, done = env_b.step(a)
        cur = env_b._cur
        assert torch.equal(ro.state[t + 1], env_b._state[cur]), t
        assert torch.equal(ro.obs_others[t + 1], env_b._obs_others[cur]), t
        assert torch.equal(rew, ro.reward[t]) and torch.equal(rew_n, ro.reward_n[t]), t
        assert torch.equal(done.to(torch.uint8), ro.done[t]), t
        if auto_reset:
            assert torch.equal(ro.goals[t + 1], env_b._goals), t
            assert torch.equal(ro.collisions[t], env_b.collisions_after_last_step), t
            d = done.bool()
            assert torch.equal(ro.term_state[t][:, d], env_b._term_state[:, d]), t
            assert torch.equal(ro.term_obs_others[t][d], env_b._term_obs_others[d]), t
        else:
            assert torch.equal(ro.collisions[t], env_b.collisions), t
    ro.close()


def test_rollout_names_the_qmix_kernel_and_refuses_the_fused_modes():
    from cm3_amd import Cm3Error, _lib
    from cm3_amd.rollout import ParticleRollout
    N, E = 4, 256
    agent, _ = _agent(N, seed=11)
    env = _env(E, N, seed=11)                                  # actor.seed == env.seed: "auto" would pick the one-launch episode
    ro = ParticleRollout(env, n_ticks=1, use_graph=False)
    agent_ran = []
    orig = agent.enqueue

    def spy(*a, **k):
        orig(*a, **k)
        torch.cuda.synchronize()
        agent_ran.append(_lib.last_kernel_variant())
    agent.enqueue = spy
    ro.collect(policy=agent, epsilon=0.1)
    assert agent_ran and agent_ran[0].startswith("k_qmix_particle<f32,N=4,"), agent_ran
    ro.close()
    for kw in (dict(policy_mode="episode"), dict(fused=True), dict(fused_policy_tick=True)):
        ro = ParticleRollout(_env(E, N, seed=11), **kw)
        with pytest.raises(Cm3Error):
            ro.collect(policy=agent, epsilon=0.1)
        ro.close()


# ---- 5. evaluation and replay ----------------------------------------------------------------------------------------------------
def test_evaluation_equals_host_loop_at_epsilon_zero():
    from cm3_amd.evaluate import test_particle
    N, E, seed = 4, 256, 9
    agent, _ = _agent(N, seed=seed)
    env = _env(E, N, dtype=torch.float64, seed=seed, max_steps=33)
    r_local, r_global, n = test_particle(env, agent, n_rounds=1)
    assert n == E and r_local.shape == (N,)
    ref = _env(E, N, dtype=torch.float64, seed=seed, max_steps=33)
    ref.reset()
    alive = torch.ones(E, dtype=torch.bool, device="cuda")
    acc_l = torch.zeros(E, N, dtype=torch.float64, device="cuda")
    acc_g = torch.zeros(E, dtype=torch.float64, device="cuda")
    for _ in range(33):
        a = agent.act(ref, 0.0)
        _, _, _, rew, rew_n, done = ref.step(a)
        acc_l += torch.where(alive.unsqueeze(1), rew_n.double(), torch.zeros_like(acc_l))
        acc_g += torch.where(alive, rew.double(), torch.zeros_like(acc_g))
        alive = alive & ~done.bool()
    assert np.allclose(r_local, acc_l.mean(0).cpu().numpy(), rtol=1e-9, atol=1e-9)
    assert abs(r_global - float(acc_g.mean())) < 1e-9


def test_off_policy_batches_fill_a_device_replay_buffer():
    from cm3_amd.replay import DeviceReplayBuffer, off_policy_batches
    from cm3_amd.rollout import ParticleRollout
    N, E, T = 4, 128, 10
    agent, _ = _agent(N, seed=3)
    env = _env(E, N, seed=3, auto_reset=True, max_steps=25)
    env.reset()
    ro = ParticleRollout(env, n_ticks=T)
    buf = DeviceReplayBuffer(4 * E * T, device="cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(0)
    batches = list(off_policy_batches(ro, buf, 3, batch_size=64, generator=g, policy=agent, epsilon=0.1))
    assert len(batches) == 3 and len(buf) == 3 * E * T
    acts = batches[-1]["actions"]
    assert acts.shape[0] == 64
    ro.close()
