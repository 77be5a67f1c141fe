#!/usr/bin/env python
"""Timing of the CM3 actor over transition rows (profiles/r19_actor_rows.txt), one JSON line per mode.

  rows    the rows kernel against the kernel it shares its forward pass with: 16 384 rows at N = 4 (4096 envs x 4 agents), for each
          precision ParticleActor.enqueue_rows with only `probs` requested (the probs fetch), with only `actions` (the draw), and
          actor.act's launch (actions only) on the same observation, each inside a captured graph of 200 launches (the same launch
          gap for all), alternating in one process; us per launch, event timing.
  batch   one training batch, 128 transitions x N = 4 (512 rows, launch-bound): train_step_feeds with target_actor and actor end to
          end (`run` = preallocated answers for the critics) against the same call without them, where `run` plays the two actor
          ops with a torch network (five matmuls, softmax, mixing, torch.multinomial); host wall time per call, synchronised.

    python tools/actor_rows_timing.py [rows] [batch] [--out FILE]     (default: both modes, FILE = profiles/r19_actor_rows.txt)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, LAUNCHES, INNER = 7, 200, 10


def _weights(N, rng):
    import numpy as np
    L = 4 * max(N - 1, 1)
    f = lambda *s: (rng.standard_normal(s) * 0.1).astype(np.float32)  # noqa: E731
    return {"actor_branch_self/kernel": f(6, 64), "actor_branch_self/bias": f(64), "W_branch_self_h2": f(64, 64), "b": f(64),
            "actor_out/kernel": f(64, 5), "actor_out/bias": f(5), "stage-2/actor_others/kernel": f(L, 128),
            "stage-2/actor_others/bias": f(128), "stage-2/W_others_h2": f(128, 64)}


def _stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def _time_graph(graph, dev):
    """us per launch over INNER replays of a graph of LAUNCHES launches"""
    import torch
    from cm3_amd import _lib
    s = torch.cuda.current_stream(dev).cuda_stream
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        _lib.check(_lib.lib().cm3_graph_launch(graph, s))
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / (INNER * LAUNCHES)


def mode_rows(dev):
    import numpy as np
    import torch
    import cm3_amd
    from cm3_amd import _lib
    from cm3_amd.actor import ParticleActor
    from cm3_amd.particle import VecParticleEnv
    N, E = 4, 4096
    env = VecParticleEnv(cm3_amd.load_config("particle_stage2_antipodal"), N, 0.2, 33, E, device=dev)
    env.reset()
    for _ in range(3):
        env.step()
    cur = env._cur
    gs, oo = env.get_obs()
    oo, vo, vg = (oo.reshape(E * N, -1).contiguous(), gs.reshape(E * N, 4).contiguous(), env.goals.reshape(E * N, 2).contiguous())
    probs = torch.empty(E * N, 5, dtype=torch.float32, device=dev)
    actions = torch.empty(E * N, dtype=torch.int32, device=dev)
    act_out = torch.empty(E, N, dtype=torch.int32, device=dev)
    w = _weights(N, np.random.default_rng(0))
    graphs = {}
    for precision in ("f32", "f16x3", "bf16"):
        actor = ParticleActor(w, N, stage=2, device=dev, precision=precision)

        def rows_probs(stream, actor=actor):
            for _ in range(LAUNCHES):
                actor.enqueue_rows(E * N, oo, vo, vg, 0.3, probs=probs, stream=stream)

        def rows_actions(stream, actor=actor):
            for _ in range(LAUNCHES):
                actor.enqueue_rows(E * N, oo, vo, vg, 0.3, actions=actions, stream=stream)

        def act(stream, actor=actor):
            for _ in range(LAUNCHES):
                actor.enqueue(E, env._obs_others[cur], env._state[cur], env._goals, env._meta, env._episode, act_out, 0.3,
                              stream=stream, env_id_base=env.env_id_base, dtype=env.dtype)
        for name, fn in (("rows_probs", rows_probs), ("rows_actions", rows_actions), ("act", act)):
            graphs[name + "_" + precision] = _lib.capture_graph(dev, fn)
    for g in graphs.values():
        _time_graph(g, dev)
    times = {k: [] for k in graphs}
    for _ in range(REPS):
        for k, g in graphs.items():
            times[k].append(_time_graph(g, dev))
    torch.cuda.synchronize()
    for g in graphs.values():
        _lib.lib().cm3_graph_destroy(g)
    return {"mode": "rows", "rows": E * N, "agents": N, "launches_per_graph": LAUNCHES, "replays": INNER, "repeats": REPS,
            **{k + "_us": _stats(v) for k, v in times.items()}, **{k + "_us_all": [round(x, 3) for x in v] for k, v in times.items()}}


def mode_batch(dev):
    import numpy as np
    import torch
    from cm3_amd.actor import ParticleActor
    from cm3_amd.batch import train_step_feeds
    N, B, gamma, eps, calls = 4, 128, 0.99, 0.3, 50
    L = 4 * (N - 1)
    rng = np.random.default_rng(0)
    f = lambda *s: torch.as_tensor(rng.standard_normal(s).astype(np.float32), device=dev)          # noqa: E731
    cols = {"v_global": f(B, N, 4), "obs_others": f(B, N, L), "v_local": f(B, N, 4),
            "actions": torch.as_tensor(rng.integers(0, 5, (B, N)), device=dev), "reward": f(B), "reward_local": f(B, N),
            "v_global_next": f(B, N, 4), "obs_others_next": f(B, N, L), "v_local_next": f(B, N, 4),
            "done": torch.as_tensor(rng.random(B) < 0.1, device=dev), "goals": f(B, N, 2)}
    main = ParticleActor(_weights(N, rng), N, stage=2, device=dev)
    target = ParticleActor(_weights(N, rng), N, stage=2, device=dev)
    z = lambda n: torch.zeros(n, 1, dtype=torch.float64, device=dev)                                # noqa: E731
    answers = {"Q_global_target": z(B * N), "Q_global": z(B * N), "Q_credit_target": z(B * N * N), "V_target": z(B * N), "V": z(B * N),
               "Q_credit": z(B * N * N * 5)}

    def run_device(ops, feed):
        return [answers.get(op) for op in ops]

    def torch_probs(w, feed):
        hs = torch.relu(torch.cat([feed["v_obs"], feed["v_goal"]], dim=1) @ w["w_self"] + w["b_self"])
        ho = torch.relu(feed["obs_others"] @ w["w_others"] + w["b_others"])
        h2 = torch.relu(hs @ w["w_self_h2"] + ho @ w["w_others_h2"] + w["b_h2"])
        return (1.0 - eps) * torch.softmax(h2 @ w["w_out"] + w["b_out"], dim=1) + eps / 5.0

    def run_torch(ops, feed):
        if ops == ["action_samples_target"]:
            return [torch.multinomial(torch_probs(target.w, feed), 1).reshape(-1)]
        if ops == ["probs"]:
            return [torch_probs(main.w, feed)]
        return run_device(ops, feed)

    paths = {"device_actors": lambda: train_step_feeds(cols, run_device, gamma, eps, target_actor=target, actor=main),
             "torch_actors_in_run": lambda: train_step_feeds(cols, run_torch, gamma, eps)}
    for fn in paths.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(REPS):
        for k, fn in paths.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e6 / calls)
    return {"mode": "batch", "transitions": B, "agents": N, "calls_per_repeat": calls, "repeats": REPS,
            **{k + "_us": _stats(v) for k, v in times.items()}, **{k + "_us_all": [round(x, 1) for x in v] for k, v in times.items()}}


def main():
    import torch
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "r19_actor_rows.txt")
    if "--out" in args:
        k = args.index("--out")
        out = args[k + 1]
        del args[k:k + 2]
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    modes = {"rows": mode_rows, "batch": mode_batch}
    lines = []
    for m in args or ["rows", "batch"]:
        lines.append(json.dumps(modes[m](dev)))
        print(lines[-1], flush=True)
    with open(out, "w") as fh:
        fh.write("# tools/actor_rows_timing.py on %s; us, min / median / max over %d repeats\n" % (torch.cuda.get_device_name(dev), REPS))
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
