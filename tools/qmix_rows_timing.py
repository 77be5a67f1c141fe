#!/usr/bin/env python
"""Timing of the QMIX train-step data side (profiles/r16_qmix_train_feeds.txt), one JSON line per mode.

  rows    the rows kernel against the kernel it was cut from: 16 384 rows at N = 4 (4096 envs x 4 agents, the C2 row count),
          ParticleQmixAgent.greedy_rows' launch with only `argmax` requested and agent.act's launch at epsilon 0, each inside a
          captured graph of 200 launches (the same launch gap for both), alternating in one process; us per launch.
  batch   one training batch, 128 transitions x N = 4 (512 rows, launch-bound): qmix_train_step_feeds with target_agent end to
          end (`run` = a no-op returning a preallocated mixer_target) against the torch composition on the same device columns
          with the argmax answered by a three-matmul torch network; host wall time per call, synchronised.
  act     agent.act's launch alone at 4096 envs, (N, dtype) = (4, f32), (1, f64), (2, f64), graphs of 200 launches.  It uses
          nothing newer than ParticleQmixAgent.enqueue: copied into tools/ of a checkout of an earlier commit it times that
          build, so two builds can be compared by alternating the two processes.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS, LAUNCHES, INNER = 7, 200, 10


def _weights(N, rng):
    import numpy as np
    L = 4 * max(N - 1, 1)
    f = lambda *s: (rng.standard_normal(s) * 0.1).astype(np.float32)  # noqa: E731
    return {"Agent_target/h/kernel": f(L + 6, 64), "Agent_target/h/bias": f(64), "Agent_target/h2/kernel": f(64, 64),
            "Agent_target/h2/bias": f(64), "Agent_target/out/kernel": f(64, 5), "Agent_target/out/bias": f(5)}


def _stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def _env(N, E, dev, dtype=None, **kw):
    import torch
    import cm3_amd
    from cm3_amd.particle import VecParticleEnv
    cfg = {1: "particle_stage1", 2: "particle_stage2_merge", 4: "particle_stage2_antipodal"}[N]
    env = VecParticleEnv(cm3_amd.load_config(cfg), N, 0.2, 33, E, device=dev, dtype=dtype or torch.float32, **kw)
    env.reset()
    for _ in range(3):
        env.step()
    return env


def _act_graph(agent, env, dev):
    import torch
    from cm3_amd import _lib
    cur = env._cur
    actions = torch.empty(env.E, env.n, dtype=torch.int32, device=dev)

    def enqueue(stream):
        for _ in range(LAUNCHES):
            agent.enqueue(env.E, env._obs_others[cur], env._state[cur], env._goals, env._meta, env._episode, actions, 0.0,
                          stream=stream, env_id_base=env.env_id_base, dtype=env.dtype)
    return _lib.capture_graph(dev, enqueue), actions


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
    from cm3_amd import _lib
    from cm3_amd.qmix import ParticleQmixAgent
    N, E = 4, 4096
    env = _env(N, E, dev)
    agent = ParticleQmixAgent(_weights(N, np.random.default_rng(0)), N, device=dev)
    cur = env._cur
    oo = env._obs_others[cur].reshape(E * N, -1).contiguous()
    vo = env._state[cur].permute(1, 0, 2).reshape(E * N, 4).contiguous()
    vg = env._goals.permute(1, 0, 2).reshape(E * N, 2).contiguous()
    argmax = torch.empty(E * N, dtype=torch.int32, device=dev)

    def enqueue(stream):
        for _ in range(LAUNCHES):
            agent.enqueue_rows(E * N, oo, vo, vg, argmax=argmax, stream=stream)
    graphs = {"rows_argmax": _lib.capture_graph(dev, enqueue), "act_eps0": _act_graph(agent, env, dev)[0]}
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


def mode_act(dev):
    import numpy as np
    import torch
    from cm3_amd import _lib
    from cm3_amd.qmix import ParticleQmixAgent
    out = {"mode": "act", "envs": 4096}
    for N, dtype, tag in ((4, torch.float32, "n4_f32"), (1, torch.float64, "n1_f64"), (2, torch.float64, "n2_f64")):
        env = _env(N, 4096, dev, dtype=dtype)
        agent = ParticleQmixAgent(_weights(N, np.random.default_rng(0)), N, device=dev)
        g, _ = _act_graph(agent, env, dev)
        _time_graph(g, dev)
        t = [_time_graph(g, dev) for _ in range(REPS)]
        torch.cuda.synchronize()
        _lib.lib().cm3_graph_destroy(g)
        out[tag + "_us"] = _stats(t)
        out[tag + "_us_all"] = [round(x, 3) for x in t]
    return out


def mode_batch(dev):
    import numpy as np
    import torch
    from cm3_amd.batch import qmix_train_step_feeds
    from cm3_amd.qmix import NAMES, ParticleQmixAgent
    from cm3_amd.replay import DeviceReplayBuffer
    from cm3_amd.rollout import ParticleRollout
    N, E, T, B, gamma, calls = 4, 64, 8, 128, 0.99, 50
    rng = np.random.default_rng(0)
    target = ParticleQmixAgent(_weights(N, rng), N, device=dev)
    env = _env(N, E, dev, auto_reset=True)
    ro = ParticleRollout(env, n_ticks=T)
    ro.collect(policy=target, epsilon=0.3, reset=False)
    buf = DeviceReplayBuffer(E * T, device=dev)
    buf.add_rollout(ro)
    cols = buf.sample_batch(B, generator=torch.Generator(device=dev).manual_seed(0))
    q_tot = torch.zeros(B, 1, dtype=torch.float32, device=dev)
    w = [target.w[k] for k in NAMES]

    def run_device(ops, feed):
        return [q_tot] if ops == ["mixer_target"] else [None]

    def run_torch(ops, feed):
        if ops == ["argmax_Q_target"]:
            x = torch.cat([feed["obs_others"], feed["v_obs"], feed["v_goal"]], dim=1)
            h = torch.relu(x @ w[0] + w[1])
            h = torch.relu(h @ w[2] + w[3])
            return [torch.argmax(h @ w[4] + w[5], dim=1)]
        return run_device(ops, feed)

    paths = {"device_feeds": lambda: qmix_train_step_feeds(cols, run_device, gamma, target_agent=target),
             "torch_composition": lambda: qmix_train_step_feeds(cols, run_torch, gamma)}
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
    ro.close()
    return {"mode": "batch", "transitions": B, "agents": N, "calls_per_repeat": calls, "repeats": REPS,
            **{k + "_us": _stats(v) for k, v in times.items()}, **{k + "_us_all": [round(x, 1) for x in v] for k, v in times.items()}}


def main():
    import torch
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    modes = {"rows": mode_rows, "batch": mode_batch, "act": mode_act}
    for m in sys.argv[1:] or ["rows", "batch"]:
        print(json.dumps(modes[m](dev)), flush=True)


if __name__ == "__main__":
    main()
