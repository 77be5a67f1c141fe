#!/usr/bin/env python
"""Timing of the Checkers QMIX train-step data side (profiles/r17_qmix_checkers_train_feeds.txt), one JSON line per mode.

  rows    the rows kernels against the kernels they were cut from: 16 384 rows at N = 2 (8192 envs x 2 agents, the C3 row count).
          Per precision ("f32", "f16x3"): CheckersQmixAgent.enqueue_rows with only `argmax` requested, on narrow inputs (int8
          windows, uint8 goal index) and on wide inputs (float64 windows, int64 one-hot goals: 600 B per row more), against
          agent.enqueue at epsilon 0 on the same rows handed over as the env does -- records of 152 bytes (padded: the dword
          staging path) and of 150 bytes (the byte path).  Each inside a captured graph of 200 launches (the same launch gap for
          all), all alternating in one process; us per launch.
  batch   one training batch, 128 transitions x N = 2 (256 rows, launch-bound): qmix_train_step_feeds(env="checkers") with
          target_agent end to end (`run` = a no-op returning a preallocated mixer_target) against the torch composition on the same
          device columns with the argmax answered by a torch restatement of the network; host wall time per call, synchronised.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS, LAUNCHES, INNER = 7, 200, 10


def _weights(N, rng):
    import numpy as np
    Lo = 2 * max(N - 1, 1)
    shapes = {"conv/Conv/weights": (3, 3, 3, 6), "conv/Conv/biases": (6,), "conv_linear/kernel": (150, 32), "conv_linear/bias": (32,),
              "branch_self/kernel": (43, 256), "branch_self/bias": (256,), "W_self_h2": (256, 256),
              "branch_others/kernel": (Lo, 256), "branch_others/bias": (256,), "W_others_h2": (256, 256), "b": (256,),
              "Qmix_single_out/kernel": (256, 5), "Qmix_single_out/bias": (5,)}
    return {"Agent_target/" + k: (rng.standard_normal(s) / np.sqrt(max(s[0], 4))).astype(np.float32) for k, s in shapes.items()}


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
    from cm3_amd import _lib
    from cm3_amd.qmix import CheckersQmixAgent
    N, E = 2, 8192
    R, Lo = E * N, 2
    rng = np.random.default_rng(0)
    t = lambda a, dt: torch.as_tensor(a, dtype=dt, device=dev)  # noqa: E731
    win = rng.integers(-1, 2, (E, 75 * N))
    raw150 = t(win, torch.int8)
    raw152 = torch.zeros(E, 152, dtype=torch.int8, device=dev)
    raw152[:, :150] = raw150
    v = t(rng.uniform(-0.5, 1.0, (E, N, 4)), torch.float64)
    oo = t(rng.uniform(-1, 1, (E, N, Lo)), torch.float64)
    goals = t(rng.integers(0, 2, (E, N)), torch.uint8)
    prev = t(rng.integers(0, 5, (E, N)), torch.int32)
    steps, episode = t(rng.integers(0, 33, E), torch.int32), t(rng.integers(0, 1 << 20, E), torch.int32)
    narrow_t, wide_t = raw150.view(R, 75), raw150.view(R, 75).double()
    wide_g = torch.nn.functional.one_hot(goals.view(R).long(), 2).contiguous()
    actions = torch.empty(E, N, dtype=torch.int32, device=dev)
    argmax = torch.empty(R, dtype=torch.int32, device=dev)
    out = {"mode": "rows", "rows": R, "agents": N, "launches_per_graph": LAUNCHES, "replays": INNER, "repeats": REPS}
    graphs = {}
    agents = []
    for precision in ("f32", "f16x3"):
        agent = CheckersQmixAgent(_weights(N, np.random.default_rng(1)), N, device=dev, precision=precision)
        agents.append(agent)

        def rows_graph(ot, vg, agent=agent):
            def enqueue(stream):
                for _ in range(LAUNCHES):
                    agent.enqueue_rows(R, ot, v.view(R, 4), oo.view(R, Lo), prev.view(R), vg, argmax=argmax, stream=stream)
            return _lib.capture_graph(dev, enqueue)

        def act_graph(raw, stride, agent=agent):
            def enqueue(stream):
                for _ in range(LAUNCHES):
                    agent.enqueue(E, raw, stride, v, oo, goals, prev, steps, episode, actions, 0.0, stream=stream)
            return _lib.capture_graph(dev, enqueue)
        graphs[precision + "_rows_narrow"] = rows_graph(narrow_t, goals.view(R))
        graphs[precision + "_rows_wide"] = rows_graph(wide_t, wide_g)
        graphs[precision + "_enqueue_stride152"] = act_graph(raw152, 152)
        graphs[precision + "_enqueue_stride150"] = act_graph(raw150, 150)
    for g in graphs.values():
        _time_graph(g, dev)
    times = {k: [] for k in graphs}
    for _ in range(REPS):
        for k, g in graphs.items():
            times[k].append(_time_graph(g, dev))
    torch.cuda.synchronize()
    for g in graphs.values():
        _lib.lib().cm3_graph_destroy(g)
    out.update({k + "_us": _stats(x) for k, x in times.items()})
    out.update({k + "_us_all": [round(y, 3) for y in x] for k, x in times.items()})
    return out


def mode_batch(dev):
    import numpy as np
    import torch
    import cm3_amd
    from cm3_amd.batch import qmix_train_step_feeds
    from cm3_amd.checkers import VecCheckersEnv
    from cm3_amd.qmix import CheckersQmixAgent
    from cm3_amd.replay import DeviceReplayBuffer
    from cm3_amd.rollout import CheckersRollout
    N, E, T, B, gamma, calls = 2, 64, 8, 128, 0.99, 50
    out = {"mode": "batch", "transitions": B, "agents": N, "calls_per_repeat": calls, "repeats": REPS}
    cfg = cm3_amd.load_config("checkers_stage2")
    for precision in ("f32", "f16x3"):
        target = CheckersQmixAgent(_weights(N, np.random.default_rng(0)), N, device=dev, precision=precision)
        env = VecCheckersEnv(cfg["init"], N, 33, E, device=dev, seed=12341, auto_reset=True)
        ro = CheckersRollout(env, n_ticks=T)
        ro.collect(np.eye(2), policy=target, epsilon=0.3)
        buf = DeviceReplayBuffer(size=E * T, device=dev)
        buf.add_rollout(ro)
        cols = buf.sample_batch(B, generator=torch.Generator(device=dev).manual_seed(0))
        q_tot = torch.zeros(B, 1, dtype=torch.float32, device=dev)
        w = target.w
        conv_w = w["conv_w"].permute(3, 2, 0, 1).contiguous()                # HWIO -> OIHW

        def run_device(ops, feed):
            return [q_tot] if ops == ["mixer_target"] else [None]

        def run_torch(ops, feed):
            if ops == ["argmax_Q_target"]:
                f32 = torch.float32
                x = feed["obs_self_t"].to(f32).permute(0, 3, 1, 2)
                c = torch.relu(torch.nn.functional.conv2d(x, conv_w, w["conv_b"], padding=1)).permute(0, 2, 3, 1).reshape(x.shape[0], -1)
                lin = torch.relu(c @ w["lin_w"] + w["lin_b"])
                cat = torch.cat([lin, feed["obs_self_v"].to(f32), feed["actions_prev"].to(f32), feed["v_goal"].to(f32)], dim=1)
                hs = torch.relu(cat @ w["self_w"] + w["self_b"])
                ho = torch.relu(feed["obs_others"].to(f32) @ w["others_w"] + w["others_b"])
                h2 = torch.relu(hs @ w["w_self_h2"] + ho @ w["w_others_h2"] + w["b_h2"])
                return [torch.argmax(h2 @ w["out_w"] + w["out_b"], dim=1)]
            return run_device(ops, feed)

        paths = {"device_feeds": lambda: qmix_train_step_feeds(cols, run_device, gamma, target_agent=target, env="checkers"),
                 "torch_composition": lambda: qmix_train_step_feeds(cols, run_torch, gamma, env="checkers")}
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
        out.update({precision + "_" + k + "_us": _stats(x) for k, x in times.items()})
        out.update({precision + "_" + k + "_us_all": [round(y, 1) for y in x] for k, x in times.items()})
    return out


def main():
    import torch
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    modes = {"rows": mode_rows, "batch": mode_batch}
    for m in sys.argv[1:] or ["rows", "batch"]:
        print(json.dumps(modes[m](dev)), flush=True)


if __name__ == "__main__":
    main()
