"""GPU: the one-launch policy rollout at the agent counts whose 16-row wave tiles are padded -- N in {3, 5, 6, 7, 9, 10}, 16 // N whole
envs per tile (csrc/policy_tiles.h; k_policy_rollout in csrc/policy.hip) -- behind ParticleRollout(..., partial_tiles=True).

What is asserted is bit equality with the launch pairs (policy_mode="tick": an actor launch and a step launch per tick), for every
new agent count, every precision of the actor and every row-tile build, plus the routing and the consumers.  The launch pairs this is
compared with are themselves held to the float64 oracles at these agent counts by the existing actor and env tests
(tests/test_gpu_actor_f64.py: the actor at every N the ABI accepts and every precision; tests/test_gpu_particle*.py: the step
kernels at 1..10 agents), so equality with them is equality with a checked path.

All of it runs on particle_ring10.json, the shipped ten-agent config (fewer agents use its first N positions)."""
import numpy as np
import pytest
import torch

from oracle import actor_oracle as AO
from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu

CFG = "particle_ring10.json"
NEW_N = [3, 5, 6, 7, 9, 10]
SEED = 21
TODAY = "policy_mode='episode' needs n_agents in {1, 2, 4, 8} and actor.seed == env.seed"     # the refusal without the keyword
ARRAYS = ("actions", "state", "obs_others", "reward", "reward_n", "done", "collisions", "goals")


def _env(E, N, dtype=torch.float32, max_steps=7, seed=SEED, auto_reset=True):
    from cm3_amd.particle import VecParticleEnv
    return VecParticleEnv(load_cfg(CFG), N, 0.2, max_steps, E, device="cuda:0", dtype=dtype, seed=seed, auto_reset=auto_reset)


def _actor(N, precision="f32", seed=SEED):
    from cm3_amd.actor import ParticleActor
    w = AO.init_weights(np.random.default_rng(N + 100), N, stage=2)
    return ParticleActor(w, N, stage=2, device="cuda:0", seed=seed, precision=precision)


def _run(E, N, precision, T, mode, auto_reset=True, **kw):
    """One collect on a freshly reset env.  auto_reset: continue from the reset env (reset=False); else episode-synchronous, the
    collector resets at collect."""
    from cm3_amd import _lib
    from cm3_amd.rollout import ParticleRollout
    env = _env(E, N, auto_reset=auto_reset)
    env.reset()
    ro = ParticleRollout(env, n_ticks=T, use_graph=False, policy_mode=mode, **kw)
    ro.collect(policy=_actor(N, precision), epsilon=0.15, reset=None if not auto_reset else False)
    torch.cuda.synchronize()
    return ro, env, _lib.last_kernel_variant()


def _same_rollout(a, ea, b, eb):
    for name in ARRAYS:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or torch.equal(x, y), name          # (goals: None for an episode-synchronous collector)
    d = a.done.bool()
    assert int(d.sum()) > 0                                                  # at least one episode ended
    if a.auto_reset:
        assert torch.equal(a.term_state.permute(0, 2, 1, 3)[d], b.term_state.permute(0, 2, 1, 3)[d])
        assert torch.equal(a.term_obs_others[d], b.term_obs_others[d])
    else:
        assert torch.equal(a.valid, b.valid)
    assert torch.equal(ea.steps, eb.steps) and torch.equal(ea.collisions, eb.collisions)
    assert torch.equal(ea.episode, eb.episode) and torch.equal(ea.global_state, eb.global_state)


def _forced(rt):
    from cm3_amd import _lib
    _lib.check(_lib.lib().cm3_policy_force_row_tiles(rt))


@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16"])
@pytest.mark.parametrize("N", NEW_N)
def test_every_padded_tile_build_is_the_launch_pairs_bit_for_bit(N, precision):
    """All 54 new builds, k_policy_rollout<N, prec, RT>: 37 envs, 16 ticks, max_steps 7 with same-launch resets, continuing from a
    reset env.  37 envs leave the last tile partly filled at every N (37 mod 5, 3, 2, 2 != 0; one env per tile at N = 9, 10), RT = 4
    gives at least two workgroups with an incomplete last one, and pad lanes sit beside owned ones in every wave.  Every trajectory
    array, the terminal captures where an episode ended and the env's counters equal those of the launch pairs, which the existing
    actor and env tests hold to the float64 oracles at these N (see the head of this file)."""
    E, T = 37, 16
    _forced(0)
    ref, eref, v = _run(E, N, precision, T, "tick")
    assert not v.startswith("k_policy_rollout"), v
    try:
        for rt in (1, 2, 4):
            _forced(rt)
            ro, env, variant = _run(E, N, precision, T, "episode", partial_tiles=True)
            assert variant.startswith("k_policy_rollout<") and ("N=%d" % N) in variant and ("g=%d," % rt) in variant, variant
            _same_rollout(ref, eref, ro, env)
            ro.close()
    finally:
        _forced(0)
    ref.close()


@pytest.mark.parametrize("N,E,auto_reset", [(3, 37, False), (10, 37, False),      # episode-synchronous: reset at collect, no same-launch resets
                                            (10, 1, True),                          # a single tile, pad lanes only beside it
                                            (3, 5, True)])                          # exactly one full tile, nothing partial
def test_further_shapes_equal_the_launch_pairs(N, E, auto_reset):
    T = 7 if not auto_reset else 16
    _forced(0)
    ref, eref, _ = _run(E, N, "f16x3", T, "tick", auto_reset=auto_reset)
    ro, env, variant = _run(E, N, "f16x3", T, "episode", auto_reset=auto_reset, partial_tiles=True)
    assert variant.startswith("k_policy_rollout<f32,N=%d" % N), variant
    _same_rollout(ref, eref, ro, env)
    ro.close()
    ref.close()


def _variant_of(env, policy, **kw):
    from cm3_amd import _lib
    from cm3_amd.rollout import ParticleRollout
    env.reset()
    ro = ParticleRollout(env, n_ticks=3, use_graph=False, **kw)
    try:
        ro.collect(policy=policy, epsilon=0.1, reset=False)
        torch.cuda.synchronize()
        return _lib.last_kernel_variant()
    finally:
        ro.close()


def test_routing_with_and_without_the_keyword():
    from cm3_amd._lib import Cm3Error
    from cm3_amd.qmix import ParticleQmixAgent
    from tests import qmix_ref as QR
    E = 37
    _forced(0)
    # without the keyword nothing changes: "episode" refuses three agents with today's words, "auto" runs the launch pairs
    with pytest.raises(Cm3Error) as e:
        _variant_of(_env(E, 3), _actor(3), policy_mode="episode")
    assert str(e.value) == TODAY
    assert _variant_of(_env(E, 3), _actor(3), policy_mode="auto").startswith("k_particle_step")
    # with it, "episode" runs the one-launch kernel
    assert _variant_of(_env(E, 3), _actor(3), policy_mode="episode", partial_tiles=True).startswith("k_policy_rollout<f32,N=3")
    # a float64 env or the QMIX agent at such a count: as today -- "episode" raises and names the condition, "auto" runs pairs
    qmix = ParticleQmixAgent(QR.init_weights(np.random.default_rng(103), 3), 3, device="cuda:0", seed=SEED, episode_kernel=True)
    for env_of, policy, word in ((lambda: _env(E, 3, dtype=torch.float64), _actor(3), "float32"),
                                 (lambda: _env(E, 3), qmix, "{1, 2, 4, 8}")):
        with pytest.raises(Cm3Error) as e:
            _variant_of(env_of(), policy, policy_mode="episode", partial_tiles=True)
        assert word in str(e.value), str(e.value)
        v = _variant_of(env_of(), policy, policy_mode="auto", partial_tiles=True)
        assert v.startswith("k_particle_step"), v
    # fused=True reaches the same entry and needs no keyword
    assert _variant_of(_env(E, 3), _actor(3), fused=True).startswith("k_policy_rollout<f32,N=3")


@pytest.mark.parametrize("N", NEW_N)
def test_auto_follows_the_committed_table(N):
    """policy_mode="auto" with the keyword: the one launch up to rollout.PARTIAL_TILES_AUTO[N] envs (measured faster there,
    profiles/r21_policy_partial_tiles.txt), the launch pairs beyond.  The table is read from the module; both sides of the bound
    are run (three ticks each)."""
    from cm3_amd.rollout import PARTIAL_TILES_AUTO
    _forced(0)
    bound = PARTIAL_TILES_AUTO[N]
    for E in (37, bound, bound + 1):
        if E < 1:
            continue
        v = _variant_of(_env(E, N), _actor(N, "f16x3"), policy_mode="auto", partial_tiles=True)
        want = "k_policy_rollout<f32,N=%d" % N if E <= bound else "k_particle_step"
        assert v.startswith(want), (E, v, want)


def test_evaluation_and_transition_export_on_a_partial_tiles_rollout():
    """evaluate.test_particle and as_reference_batch need no change: ten agents, 37 envs, one round, against the launch pairs."""
    from cm3_amd import _lib
    from cm3_amd.evaluate import test_particle as evaluate_particle
    from cm3_amd.rollout import ParticleRollout
    N, E = 10, 37
    _forced(0)
    got = []
    for kw in (dict(policy_mode="tick"), dict(policy_mode="episode", partial_tiles=True)):
        env = _env(E, N, auto_reset=False)
        ro = ParticleRollout(env, use_graph=False, **kw)
        local, glob, n = evaluate_particle(env, _actor(N, "f16x3"), n_rounds=1, epsilon=0.05, rollout=ro)
        variant = _lib.last_kernel_variant()
        cols = ro.as_reference_batch(numpy=False)
        got.append((local, glob, n, {k: v.clone() for k, v in cols.items()}, variant))
        ro.close()
    (l0, g0, n0, c0, v0), (l1, g1, n1, c1, v1) = got
    assert v0.startswith("k_particle_step") and v1.startswith("k_policy_rollout<f32,N=10"), (v0, v1)
    assert n0 == n1 == E and g0 == g1 and np.array_equal(l0, l1)
    assert c0.keys() == c1.keys()
    for name in c0:
        assert torch.equal(c0[name], c1[name]), name


def test_row_tile_rule_at_nine_and_ten_agents():
    """policy_launch: the row-tile thresholds are those of the dense agent counts, counted in tiles -- 1040 envs of ten agents are
    1040 tiles = 260 64-row workgroups, more than one per CU: RT = 4 -- except that nine and ten agents at f16x3 stay at two tiles
    (their 64-row build holds one workgroup per CU; profiles/r21_policy_partial_tiles.txt).  float32 keeps the inherited choice."""
    _forced(0)
    for N, precision, rt in ((10, "f16x3", 2), (9, "f16x3", 2), (10, "f32", 4), (7, "f16x3", 4)):
        E = 1040 if N >= 9 else 2080                      # (seven agents: two envs per tile)
        v = _variant_of(_env(E, N), _actor(N, precision), policy_mode="episode", partial_tiles=True)
        assert v.startswith("k_policy_rollout<f32,N=%d" % N) and ("g=%d," % rt) in v, (N, precision, v)
