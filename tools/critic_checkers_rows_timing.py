#!/usr/bin/env python
"""Timing of the CM3 Checkers critics over transition rows (profiles/r25_critic_checkers_rows.txt), one JSON line per mode.

  rows    the three launches of a train step -- q_rows (Q_global_target + TD target), q_pairs (Q_credit_target + TD target) and
          q_counterfactual (Q_credit over every action) -- at 128 time steps x 2 agents (256 / 512 / 2560 rows) and at
          16 384 x 2 (32 768 / 65 536 / 327 680 rows), on float64 columns (what sample_batch returns), each inside a captured graph
          of 200 launches (50 at 16 384), alternating in one process; us per launch, event timing.
  batch   one training batch, 128 transitions x N = 2: train_step_feeds(env="checkers") with the three critics end to end (`run` =
          preallocated answers for everything else) against the same call without them, where `run` plays the three ops with a torch
          network (conv2d and matmuls on the tiled feeds it is handed, cast to float32 as a tf.float32 placeholder would); host wall
          time per call, synchronised.  No time is a pass criterion.

    python tools/critic_checkers_rows_timing.py [rows] [batch] [--out FILE]   (default: both modes, FILE = profiles/r25_critic_checkers_rows.txt)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, INNER = 7, 10
LAUNCHES = {128: 200, 16384: 50}


def _weights(N, kind, rng):
    import numpy as np
    f = lambda *s: (rng.standard_normal(s) * 0.05).astype(np.float32)  # noqa: E731
    k2 = 9 * (N - 1) if kind == "global" else 4 * N
    return {"conv/Conv/weights": f(3, 5, 2, 4), "conv/Conv/biases": f(4), "conv_o/Conv/weights": f(3, 3, 3, 6), "conv_o/Conv/biases": f(6),
            "Q_branch1/kernel": f(273, 256), "Q_branch1/bias": f(256), "W_branch1_h2": f(256, 256), "stage-2/Q_branch2/kernel": f(k2, 32),
            "stage-2/Q_branch2/bias": f(32), "stage-2/W_branch2_h2": f(32, 256), "Q_out/kernel": f(256, 1), "Q_out/bias": f(1)}


def _stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def _time_graph(graph, dev, launches):
    """us per launch over INNER replays of a graph of `launches` launches"""
    import torch
    from cm3_amd import _lib
    s = torch.cuda.current_stream(dev).cuda_stream
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        _lib.check(_lib.lib().cm3_graph_launch(graph, s))
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / (INNER * launches)


def _cols(B, N, rng, dev):
    import numpy as np
    import torch
    Lo = 2 * (N - 1)
    f = lambda *s: torch.as_tensor(rng.uniform(-1, 1, s), device=dev)          # noqa: E731
    grid = lambda: torch.as_tensor(rng.integers(0, 2, (B, 3, 9, 2)).astype(np.float64), device=dev)          # noqa: E731
    win = lambda: torch.as_tensor(rng.integers(-1, 2, (B, N, 5, 5, 3)).astype(np.float64), device=dev)          # noqa: E731
    i32 = lambda: torch.as_tensor(rng.integers(0, 5, (B, N)).astype(np.int32), device=dev)          # noqa: E731
    return {"grid": grid(), "vec": f(B, N, 4), "obs_others": f(B, N, Lo), "obs_self_t": win(), "obs_self_v": f(B, N, 4),
            "actions_prev": i32(), "actions": i32(), "reward": f(B), "local_rewards": f(B, N), "next_grid": grid(), "next_vec": f(B, N, 4),
            "next_obs_others": f(B, N, Lo), "next_obs_self_t": win(), "next_obs_self_v": f(B, N, 4),
            "done": torch.as_tensor(rng.random(B) < 0.1, device=dev),
            "goals": torch.as_tensor(np.eye(2, dtype=np.int64)[rng.integers(0, 2, (B, N))], device=dev)}


def mode_rows(dev):
    import numpy as np
    import torch
    from cm3_amd import _lib
    from cm3_amd.critic import CheckersCritic
    N = 2
    rng = np.random.default_rng(0)
    q_g = CheckersCritic(_weights(N, "global", rng), N, kind="global", device=dev)
    q_c = CheckersCritic(_weights(N, "credit", rng), N, kind="credit", device=dev)
    graphs, hold = {}, []
    for B in (128, 16384):
        c = _cols(B, N, rng, dev)
        base = (c["next_grid"], c["next_vec"], c["goals"], c["next_obs_self_t"], c["next_obs_self_v"])
        ac, rw, dn = c["actions"], c["local_rewards"], c["done"].view(torch.uint8)
        out = {k: torch.empty(B * N * N * 5, dtype=torch.float32 if k == "q" else torch.float64, device=dev) for k in ("q", "q64", "td")}
        hold.append((c, dn, out))
        launches = LAUNCHES[B]

        def rows(stream, n=launches, a=base + (ac, rw, dn), o=out, B=B):
            for _ in range(n):
                q_g.enqueue(_lib.CRITIC_ROWS, B, *a, 0.99, stream=stream, **o)

        def pairs(stream, n=launches, a=base + (ac, rw, dn), o=out, B=B):
            for _ in range(n):
                q_c.enqueue(_lib.CRITIC_PAIRS, B, *a, 0.99, stream=stream, **o)

        def cf(stream, n=launches, a=base, o=out, B=B):
            for _ in range(n):
                q_c.enqueue(_lib.CRITIC_CF, B, *a, q=o["q"], stream=stream)
        for name, fn in (("q_rows", rows), ("q_pairs", pairs), ("q_counterfactual", cf)):
            graphs["%s_%d" % (name, B)] = (_lib.capture_graph(dev, fn), launches)
    for g, n in graphs.values():
        _time_graph(g, dev, n)
    times = {k: [] for k in graphs}
    for _ in range(REPS):
        for k, (g, n) in graphs.items():
            times[k].append(_time_graph(g, dev, n))
    torch.cuda.synchronize()
    for g, _ in graphs.values():
        _lib.lib().cm3_graph_destroy(g)
    return {"mode": "rows", "agents": N, "launches_per_graph": {k: n for k, (_, n) in graphs.items()}, "replays": INNER, "repeats": REPS,
            **{k + "_us": _stats(v) for k, v in times.items()}, **{k + "_us_all": [round(x, 3) for x in v] for k, v in times.items()}}


def mode_batch(dev):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from cm3_amd.batch import train_step_feeds
    from cm3_amd.critic import CheckersCritic
    N, B, gamma, eps, calls = 2, 128, 0.99, 0.3, 50
    rng = np.random.default_rng(0)
    cols = _cols(B, N, rng, dev)
    q_gt = CheckersCritic(_weights(N, "global", rng), N, kind="global", device=dev)
    q_ct = CheckersCritic(_weights(N, "credit", rng), N, kind="credit", device=dev)
    q_c = CheckersCritic(_weights(N, "credit", rng), N, kind="credit", device=dev)
    z = lambda n, w=1: torch.zeros(n, w, dtype=torch.float64, device=dev)                           # noqa: E731
    answers = {"action_samples_target": torch.as_tensor(rng.integers(0, 5, B * N), device=dev), "probs": z(B * N, 5) + 0.2,
               "Q_global": z(B * N), "Q_global_target": z(B * N), "Q_credit_target": z(B * N * N), "Q_credit": z(B * N * N * 5)}

    def run_device(ops, feed):
        return [answers.get(op) for op in ops]

    f32 = lambda t: t.to(torch.float32)                                                             # noqa: E731

    def conv(x, shape, kernel, bias):
        """relu(conv2d SAME) of NHWC rows with a [kh][kw][in][out] kernel, flattened NHWC"""
        x = f32(x).reshape(-1, *shape).permute(0, 3, 1, 2)
        y = F.conv2d(x, kernel.permute(3, 2, 0, 1), bias, padding=(kernel.shape[0] // 2, kernel.shape[1] // 2))
        return torch.relu(y).permute(0, 2, 3, 1).reshape(x.shape[0], -1)

    def torch_net(w, feed, x2):
        x1 = torch.cat([conv(feed["state_env"], (3, 9, 2), w["conv_w"], w["conv_b"]), f32(feed["v_state_one_agent"]), f32(feed["v_goal"]),
                        f32(feed["action_one"]), conv(feed["obs_self_t"], (5, 5, 3), w["conv_o_w"], w["conv_o_b"]),
                        f32(feed["obs_self_v"])], dim=1)
        b1 = torch.relu(x1 @ w["w_b1"] + w["b_b1"])
        b2 = torch.relu(torch.cat([f32(t).reshape(t.shape[0], -1) for t in x2], dim=1) @ w["w_b2"] + w["b_b2"])
        return torch.relu(b1 @ w["w_b1_h2"] + b2 @ w["w_b2_h2"]) @ w["w_out"] + w["b_out"]

    def run_torch(ops, feed):
        if ops == ["Q_global_target"]:
            return [torch_net(q_gt.w, feed, (feed["v_state_other_agents"], feed["action_others"]))]
        if ops in (["Q_credit_target"], ["Q_credit"]):
            w = q_ct.w if ops == ["Q_credit_target"] else q_c.w
            return [torch_net(w, feed, (feed["v_state_m"], feed["v_state_other_agents"]))]
        return run_device(ops, feed)

    kw = dict(env="checkers", use_V=False)
    paths = {"device_critics": lambda: train_step_feeds(cols, run_device, gamma, eps, q_global_target=q_gt, q_credit_target=q_ct,
                                                        q_credit=q_c, **kw),
             "torch_critics_in_run": lambda: train_step_feeds(cols, run_torch, gamma, eps, **kw)}
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
    out = os.path.join(ROOT, "profiles", "r25_critic_checkers_rows.txt")
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
        fh.write("# tools/critic_checkers_rows_timing.py on %s; us, min / median / max over %d repeats\n"
                 % (torch.cuda.get_device_name(dev), REPS))
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
