"""GPU: policy-driven collection on float64 (reference-precision) particle envs.

The device actor reads a float64 env's buffers and rounds them to float32 as it stages its inputs (what the reference's tf.float32
placeholders do with its float64 observations); the physics of the one-launch episode (csrc/policy.hip, PolicyReal = double) runs
in float64 with the operation order of the f64 step kernel.  Checked here: the rounding (against the f32 entry on the cast
buffers), launch pairs against the host loop, the one-launch episode against launch pairs at every row-tile build, and the
free-running episode against the float64 env oracle chained with the actor oracle."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import actor_oracle as AO
from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu

CFG = {1: "particle_stage1.json", 2: "particle_stage2_merge.json", 4: "particle_stage2_cross.json", 5: "particle_ring10.json",
       8: "particle_merge8.json"}


def _env(E, N, cfg, max_steps=33, dtype=torch.float64, **kw):
    from cm3_amd.particle import VecParticleEnv
    return VecParticleEnv(load_cfg(cfg), N, 0.2, max_steps, E, device="cuda:0", dtype=dtype, **kw)


def _actor(N, stage, precision, seed, wseed=None):
    from cm3_amd.actor import ParticleActor
    w = AO.init_weights(np.random.default_rng(N + 7 if wseed is None else wseed), N, stage=stage)
    return ParticleActor(w, N, stage=stage, device="cuda:0", seed=seed, precision=precision), w


@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16"])
@pytest.mark.parametrize("N,stage", [(1, 1), (2, 2), (4, 1), (4, 2), (5, 2), (8, 2)])
def test_actor_on_f64_env_equals_f32_entry_on_the_rounded_buffers(N, stage, precision):
    """cm3_actor_particle_f64 == cm3_actor_particle_f32 on float32 copies of the same buffers, bit for bit (ragged E)."""
    from cm3_amd import _lib
    E, seed = 333, 31
    env = _env(E, N, CFG[N], seed=seed, env_id_base=77)
    env.reset()
    for _ in range(3):
        env.step()
    actor, _ = _actor(N, stage, precision, seed)
    a64, p64 = actor.act(env, 0.2, return_probs=True)
    torch.cuda.synchronize()
    variant = _lib.last_kernel_variant()
    assert variant.startswith("k_actor_particle<f64,N=%d," % N), variant
    cur = env._cur
    a32 = torch.empty_like(a64)
    p32 = torch.empty_like(p64)
    actor.enqueue(E, env._obs_others[cur].float().contiguous(), env._state[cur].float().contiguous(), env._goals.float().contiguous(),
                  env._meta, env._episode, a32, 0.2, p32, env_id_base=env.env_id_base, dtype=torch.float32)
    torch.cuda.synchronize()
    assert _lib.last_kernel_variant().startswith("k_actor_particle<f32,N=%d," % N)
    assert torch.equal(p64, p32)
    assert torch.equal(a64, a32)


@pytest.mark.parametrize("graph", [True, False])
def test_launch_pairs_on_f64_env_equal_host_driven_policy(graph):
    """ParticleRollout(env_f64, policy_mode="tick").collect(policy=actor) == actor.act + env.step from the host, bit for bit."""
    from cm3_amd.rollout import ParticleRollout
    N, E, seed = 4, 512, 5
    actor, _ = _actor(N, 2, "f32", seed, wseed=3)
    env_a = _env(E, N, "particle_stage2_cross.json", seed=seed)
    ro = ParticleRollout(env_a, use_graph=graph, policy_mode="tick").collect(policy=actor, epsilon=0.2)
    ro.collect(policy=actor, epsilon=0.2)                       # second collection = a fresh episode (graph replay)
    env_b = _env(E, N, "particle_stage2_cross.json", seed=seed)
    env_b.reset()
    env_b.reset()
    assert torch.equal(env_b.global_state, ro.state[0].permute(1, 0, 2))
    for t in range(33):
        a = actor.act(env_b, 0.2)
        assert torch.equal(a, ro.actions[t]), t
        gs, oo, _, rew, rew_n, done = env_b.step(a)
        assert torch.equal(gs, ro.state[t + 1].permute(1, 0, 2))
        assert torch.equal(oo, ro.obs_others[t + 1])
        assert torch.equal(rew, ro.reward[t]) and torch.equal(rew_n, ro.reward_n[t])
        assert torch.equal(done.to(torch.uint8), ro.done[t])
    ro.close()


@pytest.mark.parametrize("N", [4, 2, 8, 1])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("precision", ["f32", "bf16", "f16x3"])
def test_f64_one_launch_episode_equals_launch_pairs(N, auto_reset, precision):
    """The f64 one-launch episode, and ONE fused launch per tick (eager and captured), == alternating f64 actor / step launches."""
    from cm3_amd import _lib
    from cm3_amd.rollout import ParticleRollout
    E, T, seed = 333, 40, 13
    stage = 1 if N == 1 else 2
    outs = []
    for fused, ftick, graph in ((False, False, False), (True, False, False), (False, True, False), (False, True, True)):
        env = _env(E, N, CFG[N], seed=seed, auto_reset=auto_reset, max_steps=9)
        env.reset()
        actor, _ = _actor(N, stage, precision, seed, wseed=N)
        ro = ParticleRollout(env, n_ticks=T, use_graph=graph, fused=fused, fused_policy_tick=ftick, policy_mode="tick")
        ro.collect(policy=actor, epsilon=0.15, reset=False)
        torch.cuda.synchronize()
        if fused:
            v = _lib.last_kernel_variant()
            assert v.startswith("k_policy_rollout<f64,N=%d," % N) and "fused=1" in v, v
        outs.append((ro, env))
    a, ea = outs[0]
    for b, eb in outs[1:]:
        for name in ("actions", "state", "obs_others", "reward", "reward_n", "done", "collisions"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        if auto_reset:
            assert torch.equal(a.goals, b.goals)
            d = a.done.bool()
            assert int(d.sum()) > 0
            assert torch.equal(a.term_state.permute(0, 2, 1, 3)[d], b.term_state.permute(0, 2, 1, 3)[d])
            assert torch.equal(a.term_obs_others[d], b.term_obs_others[d])
        assert torch.equal(ea.steps, eb.steps) and torch.equal(ea.collisions, eb.collisions)
        assert torch.equal(ea.episode, eb.episode) and torch.equal(ea.global_state, eb.global_state)
        assert torch.equal(ea.get_obs()[1], eb.get_obs()[1])
    for ro, _ in outs:
        ro.close()


def _policy_run(E, N, precision, T, mode, seed=21, **kw):
    from cm3_amd import _lib
    from cm3_amd.rollout import ParticleRollout
    stage = 1 if N == 1 else 2
    env = _env(E, N, CFG[N], seed=seed, auto_reset=True, max_steps=7)
    env.reset()
    actor, _ = _actor(N, stage, precision, seed, wseed=N + 100)
    ro = ParticleRollout(env, n_ticks=T, use_graph=False, policy_mode=mode, **kw)
    ro.collect(policy=actor, epsilon=0.15, reset=False)
    torch.cuda.synchronize()
    return ro, env, _lib.last_kernel_variant()


def _same_rollout(a, ea, b, eb):
    for name in ("actions", "state", "obs_others", "reward", "reward_n", "done", "collisions", "goals"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    d = a.done.bool()
    assert int(d.sum()) > 0
    assert torch.equal(a.term_state.permute(0, 2, 1, 3)[d], b.term_state.permute(0, 2, 1, 3)[d])
    assert torch.equal(a.term_obs_others[d], b.term_obs_others[d])
    assert torch.equal(ea.steps, eb.steps) and torch.equal(ea.collisions, eb.collisions)
    assert torch.equal(ea.episode, eb.episode) and torch.equal(ea.global_state, eb.global_state)


@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16"])
@pytest.mark.parametrize("N", [4, 8, 2, 1])
def test_every_row_tile_build_of_the_f64_policy_rollout_is_the_same_rollout(N, precision):
    """k_policy_rollout<N, prec, RT, double> at RT = 1, 2, 4 (forced) == the f64 launch pairs, and the variant names the build."""
    from cm3_amd import _lib
    E, T = 600, 16
    _lib.check(_lib.lib().cm3_policy_force_row_tiles(0))
    ref, eref, _ = _policy_run(E, N, precision, T, "tick")
    try:
        for rt in (1, 2, 4):
            _lib.check(_lib.lib().cm3_policy_force_row_tiles(rt))
            ro, env, variant = _policy_run(E, N, precision, T, "episode")
            assert variant.startswith("k_policy_rollout<f64,N=%d," % N) and ("g=%d," % rt) in variant, variant
            _same_rollout(ref, eref, ro, env)
            ro.close()
    finally:
        _lib.check(_lib.lib().cm3_policy_force_row_tiles(0))
    ref.close()


def _one_launch_with_probs(env, actor, T, epsilon):
    """cm3_policy_rollout_f64 over T ticks from the env's current state, as ParticleRollout's "episode" mode launches it, with the
    per-tick probabilities -> (rollout, probs [T, E, N, 5])."""
    from cm3_amd import _lib
    from cm3_amd.rollout import ParticleRollout
    ro = ParticleRollout(env, n_ticks=T, use_graph=False, policy_mode="episode")
    ro._load_slot0()
    probs = torch.zeros(T, env.E, env.n, 5, dtype=torch.float32, device=env.device)
    env._desc.flags = 0
    traj = ro._traj(0)
    ad = actor._desc(env.E, epsilon, env.env_id_base)
    _lib.check(_lib.lib().cm3_policy_rollout_f64(ctypes.byref(env._desc), ctypes.byref(traj), ctypes.byref(ad), ctypes.byref(actor._wt),
                                                 probs.data_ptr(), probs[0].numel() * 4, T, env._stream()))
    torch.cuda.synchronize()
    return ro, probs


def test_f64_one_launch_probs_equal_host_driven_actor():
    """The probabilities the one-launch episode writes == actor.act(return_probs=True) of a host loop over the same f64 env."""
    N, E, T, seed = 4, 300, 33, 9
    actor, _ = _actor(N, 2, "f16x3", seed)
    env_a = _env(E, N, "particle_stage2_antipodal.json", seed=seed)
    env_a.reset()
    ro, probs = _one_launch_with_probs(env_a, actor, T, 0.1)
    env_b = _env(E, N, "particle_stage2_antipodal.json", seed=seed)
    env_b.reset()
    for t in range(T):
        a, p = actor.act(env_b, 0.1, return_probs=True)
        assert torch.equal(p, probs[t]), t
        assert torch.equal(a, ro.actions[t]), t
        gs, _, _, rew, _, _ = env_b.step(a)
        assert torch.equal(gs, ro.state[t + 1].permute(1, 0, 2)), t
        assert torch.equal(rew, ro.reward[t]), t


@pytest.mark.parametrize("N,cfg,stage,E", [(4, "particle_stage2_antipodal.json", 2, 256), (1, "particle_stage1.json", 1, 256)])
def test_f64_one_launch_episode_follows_both_oracles_free_running(N, cfg, stage, E):
    """The f64 one-launch episode against the float64 env oracle chained with the actor oracle (inputs rounded to float32, the
    build's Philox uniforms), each running on its own actions: probabilities within 2e-5 at every tick; for every env whose
    uniforms stay 1e-4 clear of a CDF boundary over all 33 ticks, the same actions and state / observation / rewards within 1e-9.
    (The margin is the 2e-5 bound summed over four CDF terms.  Four boundaries of 2e-4 each over 4 x 33 agent-ticks leave
    (1 - 8e-4)^132 = 90 % of the N = 4 envs in that set on average, 1.9 % standard deviation at E = 256: the floor is 85 %.)"""
    from oracle.particle_oracle import VecParticleOracle
    T, seed, eps = 33, 41, 0.1
    actor, w = _actor(N, stage, "f32", seed, wseed=N + 50)
    env = _env(E, N, cfg, seed=seed)
    env.reset()
    st = env.get_state()
    episode = env.episode.cpu().numpy()
    orc = VecParticleOracle(N, load_cfg(cfg), 0.2, 33, E)
    orc.set_state(st["pos"].cpu().numpy(), st["vel"].cpu().numpy(), st["landmarks"].cpu().numpy())
    goals = st["landmarks"].cpu().numpy().reshape(E * N, 2)
    ro, probs = _one_launch_with_probs(env, actor, T, eps)
    gs, oo = orc.observe()
    safe = np.ones(E, bool)
    got_actions = ro.actions.cpu().numpy()
    got_probs = probs.cpu().numpy()
    oracle_actions, traj = [], []
    for t in range(T):
        f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731  (the tf.float32 feed of a float64 observation)
        want = AO.mixed_probs(AO.actor_probs(w, f32(oo.reshape(E * N, -1)), f32(gs.reshape(E * N, 4)), f32(goals),
                                             dtype=np.float64), eps)
        assert np.abs(got_probs[t].reshape(E * N, 5) - want).max() < 2e-5, t
        u = AO.policy_uniforms(seed, np.arange(E), episode, np.full(E, t), N).reshape(E * N)
        cdf = np.cumsum(want, axis=1)
        safe &= (np.abs(cdf - u[:, None].astype(np.float64)).min(axis=1) > 1e-4).reshape(E, N).all(axis=1)
        acts = AO.sample_actions(want.astype(np.float32), u).reshape(E, N)
        oracle_actions.append(acts)
        gs, oo, _, rew, rew_n, _ = orc.step(acts)
        traj.append((gs, oo, rew, rew_n))
    assert safe.mean() >= 0.85, safe.mean()
    for t in range(T):
        assert np.array_equal(got_actions[t][safe], oracle_actions[t][safe]), t
        gs, oo, rew, rew_n = traj[t]
        assert np.abs(ro.state[t + 1].permute(1, 0, 2).cpu().numpy()[safe] - gs[safe]).max() < 1e-9, t
        assert np.abs(ro.obs_others[t + 1].cpu().numpy()[safe] - oo[safe]).max() < 1e-9, t
        assert np.abs(ro.reward[t].cpu().numpy()[safe] - rew[safe]).max() < 1e-9, t
        assert np.abs(ro.reward_n[t].cpu().numpy()[safe] - rew_n[safe]).max() < 1e-9, t
    ro.close()


def test_batched_evaluation_on_f64_env_matches_host_driven_episodes():
    """cm3_amd.evaluate.test_particle on a float64 env == host loop of actor.act + env.step summed to each env's first done."""
    from cm3_amd.evaluate import test_particle
    N, E, seed = 4, 256, 9
    actor, _ = _actor(N, 2, "f32", seed, wseed=1)
    env = _env(E, N, "particle_stage2_antipodal.json", seed=seed)
    r_local, r_global, n = test_particle(env, actor, n_rounds=1)
    assert n == E and r_local.shape == (N,)
    ref = _env(E, N, "particle_stage2_antipodal.json", seed=seed)
    ref.reset()
    alive = torch.ones(E, dtype=torch.bool, device="cuda")
    acc_l = torch.zeros(E, N, dtype=torch.float64, device="cuda")
    acc_g = torch.zeros(E, dtype=torch.float64, device="cuda")
    for t in range(33):
        a = actor.act(ref, 0.0)
        _, _, _, rew, rew_n, done = ref.step(a)
        acc_l += torch.where(alive.unsqueeze(1), rew_n, torch.zeros_like(acc_l))
        acc_g += torch.where(alive, rew, torch.zeros_like(acc_g))
        alive = alive & ~done
    assert np.allclose(r_local, acc_l.mean(0).cpu().numpy(), rtol=1e-9, atol=1e-9)
    assert abs(r_global - float(acc_g.mean())) < 1e-9


def test_auto_mode_runs_the_f64_one_launch_kernel_and_episode_mode_refuses_n3_alike():
    from cm3_amd import Cm3Error, _lib
    from cm3_amd.rollout import ParticleRollout
    seed = 3
    actor, _ = _actor(4, 2, "f16x3", seed)
    env = _env(256, 4, "particle_stage2_antipodal.json", seed=seed)
    ro = ParticleRollout(env, policy_mode="auto").collect(policy=actor, epsilon=0.1)
    torch.cuda.synchronize()
    v = _lib.last_kernel_variant()
    assert v.startswith("k_policy_rollout<f64,N=4,") and "fused=1" in v, v
    ro.close()
    a8, _ = _actor(8, 2, "f16x3", seed)                 # eight agents: "auto" keeps the f64 launch pairs (slower one-launch build)
    ro = ParticleRollout(_env(256, 8, "particle_merge8.json", seed=seed), policy_mode="auto").collect(policy=a8, epsilon=0.1)
    torch.cuda.synchronize()
    v = _lib.last_kernel_variant()
    assert v.startswith("k_particle_step") and "<f64,N=8," in v, v
    ro.close()
    msgs = []
    for dt in (torch.float32, torch.float64):
        a3, _ = _actor(3, 2, "f32", seed)
        env3 = _env(64, 3, "particle_ring10.json", seed=seed, dtype=dt)
        with pytest.raises(Cm3Error) as ei:
            ParticleRollout(env3, policy_mode="episode").collect(policy=a3)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1]
