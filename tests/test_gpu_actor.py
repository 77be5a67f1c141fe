"""GPU: the device actor (cm3_amd/csrc/actor.hip) against the NumPy restatement of networks.actor_particle +
the epsilon-mixed sampling of alg_credit.py:119-120 (oracle/actor_oracle.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import actor_oracle as AO
from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu


def _env(E, N, cfg, max_steps=33, **kw):
    from cm3_amd.particle import VecParticleEnv
    return VecParticleEnv(load_cfg(cfg), N, 0.2, max_steps, E, device="cuda:0", dtype=torch.float32, **kw)


@pytest.mark.parametrize("N,cfg,stage", [(4, "particle_stage2_antipodal.json", 2), (2, "particle_stage2_merge.json", 2),
                                         (1, "particle_stage1.json", 1), (8, "particle_merge8.json", 2),
                                         (10, "particle_ring10.json", 2), (9, "particle_ring10.json", 2)])
@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_actor_probs_and_samples_match_oracle(N, cfg, stage, eps, precision):
    """precision "f16x3" (split float16: hi hi + hi lo + lo hi on the f16 matrix cores) is held to the SAME bound as the
    exact float32 path: 2e-5 on every probability, identical actions off CDF boundaries."""
    from cm3_amd.actor import ParticleActor
    E, seed = 1000, 77
    rng = np.random.default_rng(N * 10 + stage)
    w = AO.init_weights(rng, N, stage=stage)
    env = _env(E, N, cfg, seed=seed)
    env.reset()
    for _ in range(3):
        env.step()
    actor = ParticleActor(w, N, stage=stage, device="cuda:0", seed=seed, precision=precision)
    actions, probs = actor.act(env, eps, return_probs=True)
    gs, oo = env.get_obs()
    rows = E * N
    want = AO.mixed_probs(AO.actor_probs(w, oo.reshape(rows, -1).cpu().numpy(), gs.reshape(rows, 4).cpu().numpy(),
                                         env.goals.reshape(rows, 2).cpu().numpy()), eps)
    got = probs.reshape(rows, 5).cpu().numpy()
    assert np.abs(got - want).max() < 2e-5
    assert np.abs(got.sum(1) - 1).max() < 1e-5
    u = AO.policy_uniforms(seed, np.arange(E), env.episode.cpu().numpy(), env.steps.cpu().numpy(), N).reshape(rows)
    want_a = AO.sample_actions(want, u)
    cdf = np.cumsum(want, axis=1)
    safe = np.abs(cdf - u[:, None]).min(axis=1) > 1e-4         # u not on a CDF boundary
    assert safe.mean() > 0.99
    assert np.array_equal(actions.reshape(rows).cpu().numpy()[safe], want_a[safe])
    # empirical action frequencies follow the probabilities
    freq = np.bincount(actions.reshape(rows).cpu().numpy(), minlength=5) / rows
    assert np.abs(freq - want.mean(0)).max() < 0.05


@pytest.mark.parametrize("policy_mode", ["auto", "tick"])
def test_policy_rollout_on_device_equals_host_driven_policy(policy_mode):
    """ParticleRollout.collect(policy=actor) -- "auto": the whole episode in one launch (the default since round 3); "tick":
    alternate actor / step launches in one hipGraph -- == calling the actor and the env from the host tick by tick."""
    from cm3_amd.actor import ParticleActor
    from cm3_amd.rollout import ParticleRollout
    N, E, seed = 4, 512, 5
    w = AO.init_weights(np.random.default_rng(3), N)
    actor = ParticleActor(w, N, device="cuda:0", seed=seed)
    env_a = _env(E, N, "particle_stage2_cross.json", seed=seed)
    ro = ParticleRollout(env_a, use_graph=True, policy_mode=policy_mode).collect(policy=actor, epsilon=0.2)
    ro.collect(policy=actor, epsilon=0.2)                       # second replay = a fresh episode
    env_b = _env(E, N, "particle_stage2_cross.json", seed=seed)
    env_b.reset()
    env_b.reset()                                               # same episode index as the second collect()
    assert torch.equal(env_b.global_state, ro.state[0].permute(1, 0, 2))
    for t in range(33):
        a = actor.act(env_b, 0.2)
        assert torch.equal(a, ro.actions[t]), t
        gs, oo, _, rew, rew_n, done = env_b.step(a)
        assert torch.equal(gs, ro.state[t + 1].permute(1, 0, 2))
        assert torch.equal(rew, ro.reward[t])
    ro.close()


def test_actor_rejects_bad_weights():
    from cm3_amd import Cm3Error
    from cm3_amd.actor import ParticleActor
    w = AO.init_weights(np.random.default_rng(0), 4)
    del w["actor_out/bias"]
    with pytest.raises(Cm3Error):
        ParticleActor(w, 4, device="cuda:0")
    w = AO.init_weights(np.random.default_rng(0), 4)
    w["W_branch_self_h2"] = w["W_branch_self_h2"][:, :32]
    with pytest.raises(Cm3Error):
        ParticleActor(w, 4, device="cuda:0")


def test_batched_evaluation_matches_host_driven_episodes():
    """cm3_amd.evaluate.test_particle (evaluate.py:87-123 for E episodes at once) == stepping the env with the actor
    from the host and accumulating rewards until each env's first `done`."""
    from cm3_amd.actor import ParticleActor
    from cm3_amd.evaluate import test_particle
    N, E, seed = 4, 256, 9
    w = AO.init_weights(np.random.default_rng(1), N)
    actor = ParticleActor(w, N, device="cuda:0", seed=seed)
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
        acc_l += torch.where(alive.unsqueeze(1), rew_n.double(), torch.zeros_like(acc_l))
        acc_g += torch.where(alive, rew.double(), torch.zeros_like(acc_g))
        alive = alive & ~done
    assert np.allclose(r_local, acc_l.mean(0).cpu().numpy(), rtol=1e-6, atol=1e-6)
    assert abs(r_global - float(acc_g.mean())) < 1e-5


def test_replay_buffers_take_device_rollouts():
    from cm3_amd.replay import DeviceDualReplayBuffer, DeviceReplayBuffer
    from cm3_amd.rollout import ParticleRollout
    env = _env(64, 4, "particle_stage2_cross.json", seed=2)
    ro = ParticleRollout(env, use_graph=False).collect()
    cols = ro.as_reference_batch(numpy=False)
    buf = DeviceReplayBuffer(size=1000, device="cuda:0")
    buf.add(cols)
    assert len(buf) == 1000                                           # 64 x 33 = 2112 > capacity: newest 1000 kept
    b = buf.sample_batch(128, generator=torch.Generator(device="cuda").manual_seed(0))
    assert b["obs_others"].shape == (128, 4, 12) and b["reward"].shape == (128,)
    dual = DeviceDualReplayBuffer(size=5000, device="cuda:0")
    tt, ee = ro.valid_indices()
    dual.add(cols, (env.collisions != 0)[ee])                          # train_onpolicy.py:356
    assert len(dual.mem1) + len(dual.mem2) == tt.numel()
    ro.close()


@pytest.mark.parametrize("N,cfg", [(4, "particle_stage2_antipodal.json"), (8, "particle_merge8.json")])
def test_bf16_second_layer_is_close_to_float32(N, cfg):
    """Opt-in precision="bf16": same actor with the 192->64 layer on the bf16 matrix cores.  Not the parity path --
    probabilities must stay close to the float32 oracle (max 0.1, mean 5e-3 with deliberately large test weights) and the sampled actions agree except near CDF edges."""
    from cm3_amd.actor import ParticleActor
    E, seed = 2000, 11
    w = AO.init_weights(np.random.default_rng(5), N)
    env = _env(E, N, cfg, seed=seed)
    env.reset()
    env.step()
    a32, p32 = ParticleActor(w, N, device="cuda:0", seed=seed).act(env, 0.1, return_probs=True)
    a16, p16 = ParticleActor(w, N, device="cuda:0", seed=seed, precision="bf16").act(env, 0.1, return_probs=True)
    gs, oo = env.get_obs()
    rows = E * N
    want = AO.mixed_probs(AO.actor_probs(w, oo.reshape(rows, -1).cpu().numpy(), gs.reshape(rows, 4).cpu().numpy(),
                                         env.goals.reshape(rows, 2).cpu().numpy()), 0.1)
    diff = np.abs(p16.reshape(rows, 5).cpu().numpy() - want)
    # really different arithmetic (test weights are 50x the reference's initial scale, so logits are large), but close
    assert 1e-6 < diff.max() < 0.1 and diff.mean() < 5e-3, (diff.max(), diff.mean())
    assert np.abs(p16.sum(-1).cpu().numpy() - 1).max() < 1e-5
    assert float((a32 == a16).float().mean()) > 0.97


@pytest.mark.parametrize("N,cfg", [(4, "particle_stage2_cross.json"), (2, "particle_stage2_merge.json"),
                                    (8, "particle_merge8.json"), (1, "particle_stage1.json")])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("precision", ["f32", "bf16", "f16x3"])
def test_fused_policy_rollout_equals_launch_per_tick(N, cfg, auto_reset, precision):
    """csrc/policy.hip -- a whole policy-driven episode in one launch, or ONE fused launch per tick (eager and as a
    captured graph) -- is bit-identical to alternating actor / step launches: trajectories, sampled actions, terminal
    captures, per-tick collision counts, live counters."""
    from cm3_amd.actor import ParticleActor
    from cm3_amd.rollout import ParticleRollout
    E, T, seed = 333, 40, 13
    stage = 1 if N == 1 else 2
    w = AO.init_weights(np.random.default_rng(N), N, stage=stage)
    outs = []
    # (fused episode, fused per tick, graph): alternating launches first -- the reference for the other three
    for fused, ftick, graph in ((False, False, False), (True, False, False), (False, True, False), (False, True, True)):
        env = _env(E, N, cfg, seed=seed, auto_reset=auto_reset, max_steps=9)
        env.reset()
        actor = ParticleActor(w, N, stage=stage, device="cuda:0", seed=seed, precision=precision)
        ro = ParticleRollout(env, n_ticks=T, use_graph=graph, fused=fused, fused_policy_tick=ftick, policy_mode="tick")
        ro.collect(policy=actor, epsilon=0.15, reset=False)
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
    for ro, _ in outs:
        ro.close()


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("E,N,cfg", [(16384, 4, "particle_stage2_antipodal.json"), (8192, 8, "particle_merge8.json"),
                                     (32768, 2, "particle_stage2_merge.json")])
def test_actor_on_a_large_batch_equals_the_same_rows_in_small_batches(E, N, cfg, precision):
    """65 536 agent rows = 1024 workgroups, several per CU at once (the oracle tests above run 1-32 workgroups, alone on their
    CUs): every row's probabilities and action must be the bits the same row gets when its env shard is evaluated on its own
    (env_id_base: a shard of a batch is that part of the batch, tests/test_gpu_multirank.py), and a second launch must repeat the
    first -- rows are independent, so any difference is a fault of the launch, not of the arithmetic."""
    from cm3_amd.actor import ParticleActor
    seed, eps, Es = 17, 0.1, 512
    w = AO.init_weights(np.random.default_rng(N), N)

    def run(n, base):
        env = _env(n, N, cfg, seed=seed, env_id_base=base)
        env.reset()
        for _ in range(3):
            env.step()
        actor = ParticleActor(w, N, device="cuda:0", seed=seed, precision=precision)
        a, p = actor.act(env, eps, return_probs=True)
        a2, p2 = actor.act(env, eps, return_probs=True)
        assert torch.equal(a, a2) and torch.equal(p, p2)
        return a, p

    a_big, p_big = run(E, 0)
    assert np.abs(p_big.sum(-1).cpu().numpy() - 1).max() < 1e-5
    for base in (0, E // 2 - Es, E - Es):
        a, p = run(Es, base)
        assert torch.equal(p, p_big[base:base + Es]), base
        assert torch.equal(a, a_big[base:base + Es]), base


def _policy_run(E, N, cfg, precision, T, mode, seed=21, **kw):
    from cm3_amd import _lib
    from cm3_amd.actor import ParticleActor
    from cm3_amd.rollout import ParticleRollout
    stage = 1 if N == 1 else 2
    w = AO.init_weights(np.random.default_rng(N + 100), N, stage=stage)
    env = _env(E, N, cfg, seed=seed, auto_reset=True, max_steps=7)
    env.reset()
    actor = ParticleActor(w, N, stage=stage, device="cuda:0", seed=seed, precision=precision)
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
    assert torch.equal(ea.steps, eb.steps) and torch.equal(ea.collisions, eb.collisions)
    assert torch.equal(ea.episode, eb.episode) and torch.equal(ea.global_state, eb.global_state)


@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16"])
@pytest.mark.parametrize("N,cfg", [(4, "particle_stage2_cross.json"), (8, "particle_merge8.json"), (2, "particle_stage2_merge.json"),
                                   (1, "particle_stage1.json")])
def test_every_row_tile_build_of_the_policy_rollout_is_the_same_rollout(N, cfg, precision, monkeypatch):
    """k_policy_rollout<N, prec, RT>: 16 / 32 / 64 agent rows per workgroup are three builds of the kernel (policy.hip picks one by
    batch size; the small test batches elsewhere only ever reach RT = 1).  cm3_policy_force_row_tiles forces each in turn on ONE
    batch: all three must reproduce the alternating actor / step launches bit for bit, and cm3_last_kernel_variant() must name the
    build that ran.  With N in {1, 2, 4, 8} and the three precisions these are all 36 builds; the actor launches they are compared
    with are held to the float64 oracle at the same N and precision in tests/test_gpu_actor_f64.py."""
    from cm3_amd import _lib
    E, T = 600, 16            # ragged: 600 x N rows is no multiple of 64
    _lib.check(_lib.lib().cm3_policy_force_row_tiles(0))
    ref, eref, _ = _policy_run(E, N, cfg, precision, T, "tick")
    try:
        for rt in (1, 2, 4):
            _lib.check(_lib.lib().cm3_policy_force_row_tiles(rt))
            ro, env, variant = _policy_run(E, N, cfg, precision, T, "episode")
            assert variant.startswith("k_policy_rollout<") and ("g=%d," % rt) in variant, variant
            _same_rollout(ref, eref, ro, env)
            ro.close()
        assert _lib.lib().cm3_policy_force_row_tiles(3) != 0           # only 0, 1, 2, 4
    finally:
        _lib.check(_lib.lib().cm3_policy_force_row_tiles(0))
    ref.close()


@pytest.mark.parametrize("E,N,cfg,rt,rt_tick", [(4096, 4, "particle_stage2_antipodal.json", 2, 4),     # C2: two 32-row workgroups per CU
                                                (8192, 4, "particle_stage2_antipodal.json", 4, 4),
                                                (2048, 4, "particle_stage2_antipodal.json", 1, 2),
                                                (8192, 8, "particle_merge8.json", 4, 4),              # C5
                                                (2048, 8, "particle_merge8.json", 2, 4),
                                                (16384, 2, "particle_stage2_merge.json", 4, 4),       # two 64-row workgroups per CU, N = 2 ...
                                                (32768, 1, "particle_stage1.json", 4, 4)])            # ... and N = 1
def test_policy_rollout_row_tile_rule_at_the_baseline_sizes(E, N, cfg, rt, rt_tick, monkeypatch):
    """The rule itself (policy_launch): which build a whole-episode launch and a one-tick launch take at the BASELINE batch sizes,
    and that those launches equal the alternating actor / step launches there too."""
    from cm3_amd import _lib
    _lib.check(_lib.lib().cm3_policy_force_row_tiles(0))
    T = 9
    ref, eref, _ = _policy_run(E, N, cfg, "f16x3", T, "tick")
    ro, env, variant = _policy_run(E, N, cfg, "f16x3", T, "episode")
    assert ("g=%d," % rt) in variant and "fused=1" in variant, variant
    _same_rollout(ref, eref, ro, env)
    ro.close()
    ro, env, variant = _policy_run(E, N, cfg, "f16x3", T, "tick", fused_policy_tick=True)
    assert ("g=%d," % rt_tick) in variant and "fused=0" in variant, variant
    _same_rollout(ref, eref, ro, env)
    ro.close()
    ref.close()


def test_policy_rollout_soak_with_two_workgroups_per_cu():
    """The short soak (tools/probes/policy_soak.py is the long one): whole-episode launches against alternating actor / step
    launches on the batches that put two N = 8 workgroups on every CU -- the occupancy at which round 4's withdrawn layer returned
    wrong rows (root cause found in round 5: a packed float32 multiply with a cross-half select, profiles/r05_policy_fault.txt;
    the build no longer contains that instruction form, tests/test_abi.py) -- fresh seeds, both precisions, full 33-tick episodes
    with terminal capture.  About 15 s."""
    n = 0
    for seed in range(500, 503):
        for E, N, cfg in ((8192, 8, "particle_merge8.json"), (4096, 8, "particle_merge8.json"), (4096, 4, "particle_stage2_antipodal.json")):
            for prec in ("f16x3", "f32"):
                ref, eref, _ = _policy_run(E, N, cfg, prec, 33, "tick", seed=seed)
                ro, env, v = _policy_run(E, N, cfg, prec, 33, "episode", seed=seed)
                for name in ("actions", "state", "obs_others", "reward", "reward_n", "done", "collisions"):
                    assert torch.equal(getattr(ref, name), getattr(ro, name)), (E, N, prec, seed, name, v)
                ro.close()
                ref.close()
                n += 1
    assert n == 18


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("tag,N,stage", [("n4_stage2", 4, 2), ("n1_stage1", 1, 1), ("n8_stage2", 8, 2)])
def test_device_actor_matches_vectors_from_the_reference_function_body(tag, N, stage, precision):
    """tests/golden/actor_particle.npz: probabilities obtained by executing the reference's networks.actor_particle under
    the NumPy TF stand-in (oracle/gen_golden_actor.py).  The rows are laid out as E = rows / N envs for the kernel."""
    from cm3_amd.actor import ParticleActor
    from tests.test_oracle_actor_golden import load_cases
    w, inp, want = load_cases("actor_particle")[tag]
    rows = want.shape[0]
    E = rows // N
    dev = "cuda:0"
    obs = torch.as_tensor(inp["obs_others"]).reshape(E, N, -1).contiguous().to(dev)
    state = torch.as_tensor(inp["v_obs"]).reshape(E, N, 4).permute(1, 0, 2).contiguous().to(dev)       # [N][E][4]
    goals = torch.as_tensor(inp["v_goal"]).reshape(E, N, 2).permute(1, 0, 2).contiguous().to(dev)      # [N][E][2]
    meta = torch.zeros(E, 2, dtype=torch.int32, device=dev)
    episode = torch.zeros(E, dtype=torch.int32, device=dev)
    actions = torch.empty(E, N, dtype=torch.int32, device=dev)
    probs = torch.empty(E, N, 5, dtype=torch.float32, device=dev)
    ParticleActor(w, N, stage=stage, device=dev, precision=precision).enqueue(E, obs, state, goals, meta, episode, actions,
                                                                             0.0, probs)
    assert np.abs(probs.reshape(rows, 5).cpu().numpy() - want).max() < 2e-5


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("w2_scale,w1_scale", [(1e-3, 60.0), (3e-5, 300.0), (0.05, 1.0)])
@pytest.mark.parametrize("N,cfg", [(4, "particle_stage2_antipodal.json"), (8, "particle_merge8.json"),   # (N = 5..9: actor_others in split
                                   (5, "particle_merge8.json"), (6, "particle_merge8.json"),             #  float16 too, L = 16 .. 32 inputs)
                                   (7, "particle_merge8.json"), (9, "particle_ring10.json")])
def test_actor_split_precision_with_small_weights_and_large_activations(precision, w2_scale, w1_scale, N, cfg):
    """the float16 split x = hi + lo loses its residual to float16's subnormals once |x| < 0.125 unless the residual
    is kept scaled (csrc/actor.hip kLoScale).  Second-layer weights of 1e-3 / 3e-5 against first-layer activations of 1e2 / 1e3
    (logits still O(1)), and the reference's own scale: every probability within 2e-5 of a FLOAT64 evaluation of the network."""
    from cm3_amd.actor import ParticleActor
    E, seed = 512, 5
    rng = np.random.default_rng(17)
    w = AO.init_weights(rng, N, stage=2, scale=1.0)
    for k in ("actor_branch_self/kernel", "actor_branch_self/bias", "stage-2/actor_others/kernel", "stage-2/actor_others/bias"):
        w[k] = (w[k] * w1_scale).astype(np.float32)
    for k in ("W_branch_self_h2", "stage-2/W_others_h2"):
        w[k] = (w[k] * w2_scale / (w1_scale * 4.0)).astype(np.float32) if w2_scale >= 0.05 else (w[k] * w2_scale).astype(np.float32)
    w["b"] = (w["b"] * 0.1).astype(np.float32)
    env = _env(E, N, cfg, seed=seed)
    env.reset()
    for _ in range(3):
        env.step()
    actor = ParticleActor(w, N, stage=2, device="cuda:0", seed=seed, precision=precision)
    _, probs = actor.act(env, 0.0, return_probs=True)
    gs, oo = env.get_obs()
    rows = E * N
    f64 = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
    x = np.concatenate([f64(gs.reshape(rows, 4).cpu().numpy()), f64(env.goals.reshape(rows, 2).cpu().numpy())], axis=1)
    h_self = np.maximum(x @ f64(w["actor_branch_self/kernel"]) + f64(w["actor_branch_self/bias"]), 0)
    h_oth = np.maximum(f64(oo.reshape(rows, -1).cpu().numpy()) @ f64(w["stage-2/actor_others/kernel"]) + f64(w["stage-2/actor_others/bias"]), 0)
    h2 = np.maximum(h_self @ f64(w["W_branch_self_h2"]) + h_oth @ f64(w["stage-2/W_others_h2"]) + f64(w["b"]), 0)
    out = h2 @ f64(w["actor_out/kernel"]) + f64(w["actor_out/bias"])
    out = out - out.max(axis=1, keepdims=True)
    want = np.exp(out) / np.exp(out).sum(axis=1, keepdims=True)
    assert float(h_self.max()) > 20 * w1_scale / 60.0                 # the activations really are large
    assert 0.02 < float(want.max(axis=1).mean()) < 0.999               # ... and the policy neither uniform nor saturated everywhere
    assert np.abs(probs.reshape(rows, 5).cpu().numpy().astype(np.float64) - want).max() < 2e-5


@pytest.mark.parametrize("N,cfg", [(4, "particle_stage2_cross.json"), (8, "particle_merge8.json"), (3, "particle_merge8.json")])
@pytest.mark.parametrize("graph", [True, False])
def test_policy_launch_per_tick_on_the_live_state_rollout(N, cfg, graph):
    """Policy-driven collection, an actor launch and a step launch per tick, with the LIVE-state rollout forced (the env's state and
    goals step in place, the slots get copies; since ABI 5 a goals slot is written only where an env restarts, and the actor reads the
    live goals array): same trajectories -- goals completed on access -- as the slot-chained rollout, and, for N in {4, 8}, as the
    whole episode in one launch."""
    from cm3_amd.actor import ParticleActor
    from cm3_amd.rollout import ParticleRollout
    E, T, seed = 500, 30, 29
    w = AO.init_weights(np.random.default_rng(N), N, stage=2)
    outs = []
    modes = [dict(policy_mode="tick", live_state=True), dict(policy_mode="tick", live_state=False)]
    if N in (4, 8):
        modes.append(dict(policy_mode="episode"))
    for kw in modes:
        env = _env(E, N, cfg, seed=seed, auto_reset=True, max_steps=7)
        env.reset()
        actor = ParticleActor(w, N, stage=2, device="cuda:0", seed=seed, precision="f32")
        ro = ParticleRollout(env, n_ticks=T, use_graph=graph, **kw)
        for _ in range(2):
            ro.collect(policy=actor, epsilon=0.2, reset=False)
        outs.append((ro, env))
    a, ea = outs[0]
    assert a._live and not outs[1][0]._live
    for b, eb in outs[1:]:
        for name in ("actions", "state", "obs_others", "reward", "reward_n", "done", "collisions", "goals"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert torch.equal(ea.global_state, eb.global_state) and torch.equal(ea.goals, eb.goals) and torch.equal(ea.episode, eb.episode)
    assert int(a.done.sum()) >= 3 * E
    for ro, _ in outs:
        ro.close()


def test_packed_multiply_reproducer_controls_are_clean(tmp_path):
    """The standalone reproducer of round 5's hardware finding (tools/probes/pk_opsel_mfma_repro.hip): its CONTROL configurations --
    no aggressor wave, and the packed multiply WITHOUT a cross-half select under the worst aggressor -- must give zero wrong
    results on this box (if they did not, every comparison in this suite would be suspect).  The faulty form itself is run and
    its count printed, not asserted: a fixed chip or firmware must not fail the suite."""
    import subprocess
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "repro"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-o", str(exe),
                           os.path.join(root, "tools", "probes", "pk_opsel_mfma_repro.hip")])

    def run(victim, aggressor):
        out = subprocess.run([str(exe), str(victim), str(aggressor), "4000"], capture_output=True, text=True, timeout=120).stdout
        nums = out.split("lanes 0-15 / 16-31 / 32-47 / 48-63:")[1].split("(")[0].split()
        hi = out.split("wrong HIGH:")[1].split()
        return [int(x) for x in nums], [int(x) for x in hi], out
    lo, hi, _ = run(0, 0)
    assert lo == [0, 0, 0, 0] and hi == [0, 0, 0, 0]
    lo, hi, _ = run(2, 9)
    assert lo == [0, 0, 0, 0] and hi == [0, 0, 0, 0]
    lo, hi, text = run(0, 9)
    print("v_pk_mul_f32 op_sel:[0,1] against one 32x32x16_f16 per ~64 cycles:", text.strip())
    assert lo[:3] == [0, 0, 0]               # (only ever the last 16 lanes)
