"""GPU: every build of the particle actor (csrc/actor.hip k_actor_particle<N, precision>, N = 1..10) against the FLOAT64 oracle
(oracle/actor_oracle.py actor_probs(..., dtype=np.float64)).  The float32 oracle spends up to ~40 % of the 2e-5 parity budget on its
own rounding (tests/test_oracle_actor_f64.py); against float64 the whole budget is the kernel's.

Each case runs the three precision builds on the same rows -- env-driven (random-config envs from crowded set_state states, stepped
a few ticks) or synthetic (large-magnitude obs_others / state / goals through ParticleActor.enqueue) -- at batch sizes whose last
64-row workgroup holds the fewest and the most rows it can (E N mod 64 = 1 and 63 for odd N), at E = 1, and with env_id_base != 0,
for epsilon 0 and 0.3.  "f32" and "f16x3" are held to the parity bound; "bf16" to the bounds of
test_bf16_second_layer_is_close_to_float32."""
import numpy as np
import pytest
import torch

from oracle import actor_oracle as AO
from tests.test_gpu_particle import _random_states

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "f16x3", "bf16")
# (N, stage): stage 2 from two agents on, stage 1 at N = 1 and once more at N = 5 (others branch off while L = 16)
CASES = [(1, 1)] + [(n, 2) for n in range(2, 11)] + [(5, 1)]
BASE = 1000003


def _sizes(N):
    """(E, env_id_base): one env; the last workgroup holding the fewest rows E N mod 64 can be, then the most (1 and 63 for odd N;
    gcd(N, 64) and 64 - gcd(N, 64) otherwise), each over several workgroups; the second of those once more at env_id_base != 0."""
    g = int(np.gcd(N, 64))
    lo = next(e for e in range(200 // N, 10000) if (e * N) % 64 == g)
    hi = next(e for e in range(200 // N, 10000) if (e * N) % 64 == 64 - g)
    return [(1, 0), (lo, 0), (hi, 0), (hi, BASE)]


def _env_rows(N, stage, E, base, seed, rng):
    """Random-config env (as test_f64_free_running_random_configs_all_agent_counts builds it), crowded set_state state, three
    ticks of random actions: -> (inputs [E, N, ...] on the device, episode, steps)."""
    from cm3_amd.particle import VecParticleEnv
    cfg = dict(n_agents=N, agents_x=rng.uniform(-1, 1, N).tolist(), agents_y=rng.uniform(-1, 1, N).tolist(),
               landmarks_x=rng.uniform(-1, 1, N).tolist(), landmarks_y=rng.uniform(-1, 1, N).tolist(), initial_std=0.1)
    env = VecParticleEnv(cfg, N, 0.2, 20, E, device="cuda:0", dtype=torch.float32, seed=seed, env_id_base=base)
    pos, vel, lm = _random_states(rng, E, N, crowd=0.7)
    env.set_state(pos, vel, lm, steps=rng.integers(0, 15, E), episode=rng.integers(0, 1000, E))
    for _ in range(3):
        env.step(torch.as_tensor(rng.integers(0, 5, (E, N))))
    cur = env._cur
    return dict(obs_others=env._obs_others[cur], state=env._state[cur], goals=env._goals, meta=env._meta, episode=env._episode)


def _synthetic_rows(N, E, rng):
    """Large-magnitude inputs straight into the launch: obs_others / state / goals uniform in +-30 (velocities, positions and
    relative positions of a scattered world), random step counters and episodes."""
    L = 4 * max(N - 1, 1)
    dev = "cuda:0"
    f = lambda *shape: torch.as_tensor(rng.uniform(-30, 30, shape), dtype=torch.float32, device=dev)  # noqa: E731
    meta = torch.as_tensor(np.stack([rng.integers(0, 33, E), rng.integers(0, 50, E)], 1), dtype=torch.int32, device=dev)
    return dict(obs_others=f(E, N, L), state=f(N, E, 4), goals=f(N, E, 2), meta=meta.contiguous(),
                episode=torch.as_tensor(rng.integers(0, 1 << 20, E), dtype=torch.int32, device=dev))


def _weights(N, stage, kind, rng):
    w = AO.init_weights(rng, N, stage=stage)
    if kind == "synthetic":          # first layers 20x smaller against the 30x larger inputs: the policy stays informative
        for k in ("actor_branch_self/kernel", "stage-2/actor_others/kernel"):
            if k in w:
                w[k] = (w[k] / 20).astype(np.float32)
    return w


def _oracle64(w, inp, E, N):
    """float64 probabilities [E N, 5] of the rows the launch read (inputs fetched back as the float32 the kernel saw)."""
    rows = E * N
    oo = inp["obs_others"].reshape(rows, -1).cpu().numpy()
    st = inp["state"].permute(1, 0, 2).reshape(rows, 4).cpu().numpy()          # [N][E][4] -> rows e * N + i
    gl = inp["goals"].permute(1, 0, 2).reshape(rows, 2).cpu().numpy()
    return AO.actor_probs(w, oo, st, gl, dtype=np.float64)


def _run(actor, inp, E, eps, base):
    from cm3_amd import _lib
    actions = torch.empty(E, actor.n, dtype=torch.int32, device="cuda:0")
    probs = torch.empty(E, actor.n, 5, dtype=torch.float32, device="cuda:0")
    actor.enqueue(E, inp["obs_others"], inp["state"], inp["goals"], inp["meta"], inp["episode"], actions, eps, probs,
                  env_id_base=base)
    v = _lib.last_kernel_variant()
    torch.cuda.synchronize()
    return actions.reshape(-1).cpu().numpy(), probs.reshape(-1, 5).cpu().numpy().astype(np.float64), v


@pytest.mark.parametrize("kind", ["env", "synthetic"])
@pytest.mark.parametrize("N,stage", CASES)
def test_every_particle_actor_build_against_float64(N, stage, kind):
    from cm3_amd.actor import ParticleActor
    seed = 4242 + N
    rng = np.random.default_rng(100 * N + 10 * stage + (kind == "env"))
    w = _weights(N, stage, kind, rng)
    actors = {p: ParticleActor(w, N, stage=stage, device="cuda:0", seed=seed, precision=p) for p in PRECISIONS}
    err = {p: [] for p in PRECISIONS}
    safe_all, agree_bf16, ptp = [], [], []
    for E, base in _sizes(N):
        inp = _env_rows(N, stage, E, base, seed, rng) if kind == "env" else _synthetic_rows(N, E, rng)
        p64 = _oracle64(w, inp, E, N)
        ptp.append(np.ptp(p64, axis=1))
        u = AO.policy_uniforms(seed, base + np.arange(E), inp["episode"].cpu().numpy(), inp["meta"][:, 0].cpu().numpy(),
                               N).reshape(-1)
        for eps in (0.0, 0.3):
            want = AO.mixed_probs(p64, eps)
            want_a = AO.sample_actions(want, u)
            safe = np.abs(np.cumsum(want, axis=1) - u[:, None]).min(axis=1) > 1e-4       # u not on a CDF boundary
            safe_all.append(safe)
            acts = {}
            for prec, actor in actors.items():
                a, p, v = _run(actor, inp, E, eps, base)
                assert v.startswith("k_actor_particle<") and (",N=%d," % N) in v and v.endswith(",prec=%s>" % prec), v
                acts[prec] = a
                d = np.abs(p - want)
                err[prec].append(d)
                assert np.abs(p.sum(1) - 1).max() < 1e-5, (prec, E)
                if prec != "bf16":
                    assert d.max() < 2e-5, (prec, E, base, eps, d.max())
                    assert np.array_equal(a[safe], want_a[safe]), (prec, E, base, eps)
            agree_bf16.append(acts["bf16"] == acts["f32"])
    worst = {p: float(np.concatenate(e).max()) for p, e in err.items()}
    print("particle actor N=%d stage=%d %-9s worst |p - float64|: f32 %.2e  f16x3 %.2e  bf16 %.2e"
          % (N, stage, kind, worst["f32"], worst["f16x3"], worst["bf16"]))
    assert np.concatenate(ptp).mean() > 0.05                          # the policy is not uniform
    assert np.concatenate(safe_all).mean() > 0.99
    # split float16 is in the float32 error class (measured on MI355X: worst f16x3 error 0.5 .. 1.8 x the f32 build's over the 22
    # cases, largest 8.3e-6 at N = 6 against f32's 4.7e-6; f32 itself 0.8e-6 .. 7.0e-6)
    assert worst["f16x3"] <= 4 * worst["f32"] + 1e-6, worst
    # bf16 second layer: really different arithmetic, but close -- the bounds of test_bf16_second_layer_is_close_to_float32 (max 0.1,
    # mean 5e-3), except the max at ten agents: measured on MI355X 0.012 (N = 1) growing to 0.075 (N = 7, 8) and 0.117 (N = 10, env
    # rows; means <= 7e-4).  That is the arithmetic, not a fault: rounding both operands of the second layer to bf16 (nearest even) in
    # an otherwise float64 evaluation of the same construction gives worst errors of 0.043 / 0.083 / 0.100 / 0.141 at N = 4 / 8 / 9 / 10.
    bf = np.concatenate(err["bf16"])
    assert 1e-6 < bf.max() < (0.15 if N == 10 else 0.1) and bf.mean() < 5e-3, (bf.max(), bf.mean())
    assert np.concatenate(agree_bf16).mean() > 0.97


def test_particle_actor_abi_rejects_agent_counts_outside_1_to_10():
    """The launch and the pack entry point refuse N = 0 and N = 11 before touching a buffer; N = 4 on the same actor still runs."""
    from cm3_amd import Cm3Error
    from cm3_amd.actor import ParticleActor
    w = AO.init_weights(np.random.default_rng(0), 4)
    actor = ParticleActor(w, 4, device="cuda:0")
    inp = _synthetic_rows(4, 8, np.random.default_rng(1))
    actions = torch.zeros(8, 4, dtype=torch.int32, device="cuda:0")
    for n in (0, 11):
        actor.n = n
        with pytest.raises(Cm3Error, match="n_agents"):
            actor.enqueue(8, inp["obs_others"], inp["state"], inp["goals"], inp["meta"], inp["episode"], actions, 0.0)
        with pytest.raises(Cm3Error, match="n_agents"):
            actor.repack()
    actor.n = 4
    actor.enqueue(8, inp["obs_others"], inp["state"], inp["goals"], inp["meta"], inp["episode"], actions, 0.0)
    torch.cuda.synchronize()
