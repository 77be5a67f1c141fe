"""GPU: every build of the Checkers actor (csrc/actor_checkers.hip: k_ck_actor<false> "f32", k_ck_actor_x3 "f16x3", k_ck_actor<true>
"bf16") at every agent count it accepts, N = 1..8, against the FLOAT64 oracle (oracle/actor_checkers_oracle.py
actor_probs(..., dtype=np.float64)).  The reference configurations stop at N = 2; from N = 3 on the others branch has Lo = 2 (N - 1)
= 4..14 inputs (k_ck_actor: ceil(Lo / 4) matrix k-steps; k_ck_actor_x3: more than two staged values per row), env records straddle
a 64-row workgroup whenever N does not divide 64, and the dword window path runs 16 or 32 lanes per env (N = 4, 8).

Each case runs the three builds on the same rows -- env-driven (a generic n_obs = 2 geometry: a 7 x 8 band for N <= 7, 9 x 6 for
N = 8, stepped a few ticks) or synthetic (int8 windows in {-1, 0, 1}, random obs_self_v / obs_others / actions_prev / prev_done
through CheckersActor.enqueue, at record strides 75 N and 75 N + 1) -- at E = 1, at the fewest and the most rows a last workgroup
can hold, and with env_id_base != 0, for epsilon 0 and 0.3.  Same checks as tests/test_gpu_actor_f64.py."""
import numpy as np
import pytest
import torch

from oracle import actor_checkers_oracle as AO
from tests.test_gpu_actor_f64 import BASE, PRECISIONS, _sizes

pytestmark = pytest.mark.gpu

KERNEL = {"f32": "k_ck_actor<", "bf16": "k_ck_actor<", "f16x3": "k_ck_actor_x3<"}


def _env_rows(N, E, base, seed, rng):
    """Generic geometry with n_obs = 2, agents on distinct rows of the start column; three ticks of random actions.  (Records of
    75 N bytes: the env pads records only for the reference's 3 x 8 band; the dword window path is the synthetic cases' stride 75 N
    at N = 4 and 8.)"""
    from cm3_amd.checkers import VecCheckersEnv
    R, C = (7, 8) if N <= 7 else (9, 6)
    rows = rng.permutation(R)[:N]
    init = dict(n_rows=R, n_columns=C, n_obs=2, agents_r=[int(r) for r in rows], agents_c=[C] * N)
    env = VecCheckersEnv(init, N, 30, E, device="cuda:0", seed=seed, env_id_base=base)
    env.reset(goal_index=torch.as_tensor(rng.integers(0, 2, (E, N))))
    for _ in range(3):
        env.step(torch.as_tensor(rng.integers(0, 5, (E, N))))
    s = env._slots[env._cur]
    dev = "cuda:0"
    return dict(raw=s["obs_self_t_raw"], stride=env.obst_stride, obs_self_v=s["obs_self_v"], obs_others=s["obs_others"],
                goals=env._goals, steps=env._steps, episode=env._episode,
                actions_prev=torch.as_tensor(rng.integers(0, 5, (E, N)), dtype=torch.int32, device=dev), prev_done=None)


def _synthetic_rows(N, E, stride, rng):
    """int8 windows in {-1, 0, 1} at `stride` bytes per env (the bytes past 75 N hold 5, a value no window has), random obs_self_v
    and float64 obs_others, actions_prev, prev_done, goals, step counters and episodes."""
    dev = "cuda:0"
    Lo = 2 * max(N - 1, 1)
    raw = np.full((E, stride), 5, np.int8)
    raw[:, :75 * N] = rng.integers(-1, 2, (E, 75 * N))
    i32 = lambda a: torch.as_tensor(a, dtype=torch.int32, device=dev)  # noqa: E731
    f64 = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    return dict(raw=torch.as_tensor(raw, device=dev), stride=stride, obs_self_v=f64(rng.uniform(-0.5, 1.0, (E, N, 4))),
                obs_others=f64(rng.uniform(-1, 1, (E, N, Lo))),
                goals=torch.as_tensor(rng.integers(0, 2, (E, N)), dtype=torch.uint8, device=dev),
                steps=i32(rng.integers(0, 33, E)), episode=i32(rng.integers(0, 1 << 20, E)),
                actions_prev=i32(rng.integers(0, 5, (E, N))),
                prev_done=torch.as_tensor(rng.random(E) < 0.3, dtype=torch.uint8, device=dev))


def _oracle64(w, inp, E, N):
    rows = E * N
    ot = inp["raw"][:, :75 * N].cpu().numpy().astype(np.float64).reshape(rows, 5, 5, 3)
    prev = inp["actions_prev"].cpu().numpy()
    if inp["prev_done"] is not None:                       # a fresh episode starts from actions_prev = zeros
        prev = np.where(inp["prev_done"].cpu().numpy().astype(bool)[:, None], 0, prev)
    goals = np.eye(2)[inp["goals"].cpu().numpy().reshape(rows).astype(np.int64)]
    return AO.actor_probs(w, prev.reshape(rows), ot, inp["obs_self_v"].reshape(rows, 4).cpu().numpy(),
                          inp["obs_others"].reshape(rows, -1).cpu().numpy(), goals, dtype=np.float64)


def _run(actor, inp, E, eps, base):
    from cm3_amd import _lib
    actions = torch.empty(E, actor.n, dtype=torch.int32, device="cuda:0")
    probs = torch.empty(E, actor.n, 5, dtype=torch.float32, device="cuda:0")
    actor.enqueue(E, inp["raw"], inp["stride"], inp["obs_self_v"], inp["obs_others"], inp["goals"], inp["actions_prev"], inp["steps"],
                  inp["episode"], actions, eps, probs, env_id_base=base, prev_done=inp["prev_done"])
    v = _lib.last_kernel_variant()
    torch.cuda.synchronize()
    return actions.reshape(-1).cpu().numpy(), probs.reshape(-1, 5).cpu().numpy().astype(np.float64), v


@pytest.mark.parametrize("kind", ["env", "stride75N", "stride75N+1"])
@pytest.mark.parametrize("N", range(1, 9))
def test_every_checkers_actor_build_against_float64(N, kind):
    from cm3_amd.actor import CheckersActor
    stage = 1 if N == 1 else 2
    seed = 5150 + N
    rng = np.random.default_rng(1000 + 10 * N + len(kind))
    w = AO.init_weights(rng, N, stage=stage)
    actors = {p: CheckersActor(w, N, stage=stage, device="cuda:0", seed=seed, precision=p) for p in PRECISIONS}
    err = {p: [] for p in PRECISIONS}
    safe_all, agree_bf16, ptp = [], [], []
    for E, base in _sizes(N):
        if kind == "env":
            inp = _env_rows(N, E, base, seed, rng)
        else:
            inp = _synthetic_rows(N, E, 75 * N + (kind == "stride75N+1"), rng)
        p64 = _oracle64(w, inp, E, N)
        ptp.append(np.ptp(p64, axis=1))
        u = AO.policy_uniforms(seed, base + np.arange(E), inp["episode"].cpu().numpy(), inp["steps"].cpu().numpy(), N).reshape(-1)
        for eps in (0.0, 0.3):
            want = AO.mixed_probs(p64, eps)
            want_a = AO.sample_actions(want, u)
            safe = np.abs(np.cumsum(want, axis=1) - u[:, None]).min(axis=1) > 1e-4       # u not on a CDF boundary
            safe_all.append(safe)
            acts = {}
            for prec, actor in actors.items():
                a, p, v = _run(actor, inp, E, eps, base)
                assert v.startswith(KERNEL[prec]) and (",N=%d," % N) in v and v.endswith(",prec=%s>" % prec), v
                acts[prec] = a
                d = np.abs(p - want)
                err[prec].append(d)
                assert np.abs(p.sum(1) - 1).max() < 1e-5, (prec, E)
                if prec != "bf16":
                    assert d.max() < 2e-5, (prec, E, base, eps, d.max())
                    assert np.array_equal(a[safe], want_a[safe]), (prec, E, base, eps)
            agree_bf16.append(acts["bf16"] == acts["f32"])
    worst = {p: float(np.concatenate(e).max()) for p, e in err.items()}
    print("checkers actor N=%d %-11s worst |p - float64|: f32 %.2e  f16x3 %.2e  bf16 %.2e"
          % (N, kind, worst["f32"], worst["f16x3"], worst["bf16"]))
    assert np.concatenate(ptp).mean() > 0.05                          # the policy is not uniform
    assert np.concatenate(safe_all).mean() > 0.99
    # split float16 is in the float32 error class (measured on MI355X: worst f16x3 error 0.8 .. 2.0 x the f32 build's, all cases
    # within 1.3e-6 of float64 -- the Checkers actor's weights are fan-in scaled, its logits O(1))
    assert worst["f16x3"] <= 4 * worst["f32"] + 1e-6, worst
    # bf16 256 x 256 layers: really different arithmetic, but close (the bounds of test_bf16_layers_are_close_to_float32)
    bf = np.concatenate(err["bf16"])
    assert 1e-6 < bf.max() < 0.1 and bf.mean() < 5e-3, (bf.max(), bf.mean())
    assert np.concatenate(agree_bf16).mean() > 0.97


def test_checkers_actor_abi_rejects_agent_counts_outside_1_to_8():
    """The launch and the pack entry point refuse N = 0 and N = 9 before touching a buffer; N = 2 on the same actor still runs."""
    from cm3_amd import Cm3Error
    from cm3_amd.actor import CheckersActor
    actor = CheckersActor(AO.init_weights(np.random.default_rng(0), 2), 2, device="cuda:0")
    inp = _synthetic_rows(2, 8, 152, np.random.default_rng(1))
    actions = torch.zeros(8, 2, dtype=torch.int32, device="cuda:0")
    args = (8, inp["raw"], inp["stride"], inp["obs_self_v"], inp["obs_others"], inp["goals"], inp["actions_prev"], inp["steps"],
            inp["episode"], actions, 0.0)
    for n in (0, 9):
        actor.n = n
        with pytest.raises(Cm3Error, match="n_agents"):
            actor.enqueue(*args)
        with pytest.raises(Cm3Error, match="n_agents"):
            actor.repack()
    actor.n = 2
    actor.enqueue(*args)
    torch.cuda.synchronize()
