#!/usr/bin/env python
"""Timing of the Checkers IAC / COMA baseline critics over transition rows (profiles/r30_baseline_checkers_rows.txt), one JSON line
per mode.

  rows    the three rows launches -- v_rows of a local and of a global value network (V + TD target) and q_rows of the COMA critic
          (Q, the own action's value, TD target) -- at 128 time steps x 2 agents (256 rows) and at 16 384 x 2 (32 768 rows), on the
          float64 / int64 one-hot columns a sampled batch holds, each inside a captured graph of 200 launches, alternating in one
          process; us per launch, event timing.
  batch   one training batch, 128 transitions x N = 2, both critics on (use_Q = 1, use_V = 1):
          baseline_train_step_feeds(env="checkers") with all six device networks end to end (`run` = preallocated answers for the
          optimiser ops) against the same call without the four value networks, where `run` plays V_target / V, Q_target and Q with
          a torch network (convolutions and matmuls on the tiled feeds it is handed, cast to float32 as a tf.float32 placeholder
          would) and answers the two actor ops from the same device actors; host wall time per call, synchronised.
  No time is a pass criterion.

    python tools/baseline_checkers_rows_timing.py [rows] [batch] [--out FILE]     (default: both modes, FILE as above)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, LAUNCHES, INNER = 7, 200, 10
N_AGENTS = 2


def _value_weights(N, kind, rng):
    import numpy as np
    from cm3_amd.baseline import CK_VALUE_NAMES, checkers_value_weight_shapes
    return {CK_VALUE_NAMES[kind][s]: (rng.standard_normal(shape) * 0.1).astype(np.float32)
            for s, shape in checkers_value_weight_shapes(N, kind, 2).items()}


def _coma_weights(N, rng):
    import numpy as np
    from cm3_amd.baseline import CK_COMA_NAMES, checkers_coma_weight_shapes
    return {CK_COMA_NAMES[s]: (rng.standard_normal(shape) * 0.1).astype(np.float32) for s, shape in checkers_coma_weight_shapes(N).items()}


def _actor(N, rng, dev):
    from cm3_amd.actor import CheckersActor
    from oracle import actor_checkers_oracle as CO
    return CheckersActor(CO.init_weights(rng, N, stage=2), N, stage=2, device=dev)


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
    """the 16 columns of a sampled Checkers batch: wide columns float64, goals int64 one-hot"""
    import numpy as np
    import torch
    Lo = 2 * (N - 1)
    u = lambda *s: torch.as_tensor(rng.uniform(-1, 1, s), device=dev)          # noqa: E731
    grid = lambda: torch.as_tensor(rng.integers(0, 2, (B, 3, 9, 2)).astype(np.float64), device=dev)          # noqa: E731
    win = lambda: torch.as_tensor(rng.integers(-1, 2, (B, N, 5, 5, 3)).astype(np.float64), device=dev)          # noqa: E731
    acts = lambda: torch.as_tensor(rng.integers(0, 5, (B, N)).astype(np.int32), device=dev)          # noqa: E731
    return {"grid": grid(), "vec": u(B, N, 4), "obs_others": u(B, N, Lo), "obs_self_t": win(), "obs_self_v": u(B, N, 4),
            "actions_prev": acts(), "actions": acts(), "reward": u(B), "local_rewards": u(B, N), "next_grid": grid(),
            "next_vec": u(B, N, 4), "next_obs_others": u(B, N, Lo), "next_obs_self_t": win(), "next_obs_self_v": u(B, N, 4),
            "done": torch.as_tensor(rng.random(B) < 0.1, device=dev),
            "goals": torch.as_tensor(np.eye(2, dtype=np.int64)[rng.integers(0, 2, (B, N))], device=dev)}


def mode_rows(dev):
    import numpy as np
    import torch
    from cm3_amd import _lib
    from cm3_amd.baseline import CheckersComaCritic, CheckersValue
    N = N_AGENTS
    rng = np.random.default_rng(0)
    v_l = CheckersValue(_value_weights(N, "local", rng), N, kind="local", device=dev)
    v_g = CheckersValue(_value_weights(N, "global", rng), N, kind="global", device=dev)
    q = CheckersComaCritic(_coma_weights(N, rng), N, device=dev)
    graphs, hold = {}, []
    for B in (128, 16384):
        c = _cols(B, N, rng, dev)
        go, ac, dn = c["goals"], c["actions"], c["done"].view(torch.uint8)
        R = B * N
        ov = {"v": torch.empty(R, dtype=torch.float32, device=dev), "v64": torch.empty(R, dtype=torch.float64, device=dev),
              "td": torch.empty(R, dtype=torch.float64, device=dev)}
        oq = {"q": torch.empty(R, 5, dtype=torch.float32, device=dev), "q_taken": torch.empty(R, dtype=torch.float32, device=dev),
              "q_taken64": torch.empty(R, dtype=torch.float64, device=dev), "td": torch.empty(R, dtype=torch.float64, device=dev)}
        hold.append((c, dn, ov, oq))

        def local(stream, c=c, go=go, dn=dn, o=ov, B=B):
            for _ in range(LAUNCHES):
                v_l.enqueue(B, go, windows=c["next_obs_self_t"], obs_self_v=c["next_obs_self_v"], obs_others=c["next_obs_others"],
                            reward=c["local_rewards"], done=dn, gamma=0.99, stream=stream, **o)

        def glob(stream, c=c, go=go, dn=dn, o=ov, B=B):
            for _ in range(LAUNCHES):
                v_g.enqueue(B, go, grid=c["next_grid"], vec=c["next_vec"], reward=c["local_rewards"], done=dn, gamma=0.99, stream=stream, **o)

        def coma(stream, c=c, go=go, ac=ac, dn=dn, o=oq, B=B):
            for _ in range(LAUNCHES):
                q.enqueue(B, c["next_grid"], c["next_vec"], go, c["next_obs_self_t"], c["next_obs_self_v"], ac, ac, c["reward"], dn, 0.99,
                          stream=stream, **o)
        for name, fn in (("v_rows_local", local), ("v_rows_global", glob), ("q_rows_coma", coma)):
            graphs["%s_%d" % (name, B)] = (_lib.capture_graph(dev, fn), LAUNCHES)
    for g, n in graphs.values():
        _time_graph(g, dev, n)
    times = {k: [] for k in graphs}
    for _ in range(REPS):
        for k, (g, n) in graphs.items():
            times[k].append(_time_graph(g, dev, n))
    torch.cuda.synchronize()
    for g, _ in graphs.values():
        _lib.lib().cm3_graph_destroy(g)
    return {"mode": "rows", "agents": N, "launches_per_graph": LAUNCHES, "replays": INNER, "repeats": REPS,
            **{k + "_us": _stats(v) for k, v in times.items()}, **{k + "_us_all": [round(x, 3) for x in v] for k, v in times.items()}}


def mode_batch(dev):
    import numpy as np
    import torch
    from cm3_amd.baseline import CheckersComaCritic, CheckersValue
    from cm3_amd.batch import baseline_train_step_feeds
    N, B, gamma, eps, calls = N_AGENTS, 128, 0.99, 0.3, 50
    rng = np.random.default_rng(0)
    cols = _cols(B, N, rng, dev)
    v_t, v_m = (CheckersValue(_value_weights(N, "global", rng), N, kind="global", device=dev) for _ in range(2))
    q_t, q_m = (CheckersComaCritic(_coma_weights(N, rng), N, device=dev) for _ in range(2))
    target_actor, actor = _actor(N, rng, dev), _actor(N, rng, dev)
    v_res = torch.zeros(B * N, 1, dtype=torch.float32, device=dev)
    f32 = lambda t: t.to(torch.float32).reshape(t.shape[0], -1)                                     # noqa: E731

    def run_device(ops, feed):
        return [v_res if op == "V" else None for op in ops]

    def conv(x, kernel, bias):          # relu(conv2d SAME) of NHWC x with a TF kernel [kh, kw, C, F], flattened NHWC
        y = torch.nn.functional.conv2d(x.to(torch.float32).permute(0, 3, 1, 2), kernel.permute(3, 2, 0, 1), bias,
                                       padding=(kernel.shape[0] // 2, kernel.shape[1] // 2))
        return torch.relu(y).permute(0, 2, 3, 1).reshape(x.shape[0], -1)

    def torch_value(w, feed):
        x1 = torch.cat([conv(feed["state_env"], w["conv_w"], w["conv_b"]), f32(feed["v_state_one_agent"]), f32(feed["v_goal"])], dim=1)
        b1 = torch.relu(x1 @ w["w_b1"] + w["b_b1"])
        b2 = torch.relu(f32(feed["v_state_other_agents"]) @ w["w_b2"] + w["b_b2"])
        return torch.relu(b1 @ w["w_b1_h2"] + b2 @ w["w_b2_h2"]) @ w["w_out"] + w["b_out"]

    def torch_coma(w, feed):
        x = torch.cat([conv(feed["state_env"], w["conv_s_w"], w["conv_s_b"])]
                      + [f32(feed[k]) for k in ("v_state", "action_others", "v_goal", "v_goal_others", "v_labels")]
                      + [conv(feed["obs_self_t"], w["conv_o_w"], w["conv_o_b"]), f32(feed["obs_self_v"])], dim=1)
        h = torch.relu(torch.relu(x @ w["w_h1"] + w["b_h1"]) @ w["w_h2"] + w["b_h2"])
        return h @ w["w_out"] + w["b_out"]

    def actor_args(feed):
        return (feed["obs_self_t"], feed["obs_self_v"], feed["obs_others"], feed["actions_prev"].argmax(dim=1), feed["v_goal"], feed["epsilon"])

    def run_torch(ops, feed):
        if ops == ["V_target", "V"]:
            return [torch_value(v_t.w, feed), torch_value(v_m.w, feed)]
        if ops == ["action_samples_target"]:
            return [target_actor.sample_rows(*actor_args(feed))["actions"]]
        if ops == ["Q_target"]:
            return [torch_coma(q_t.w, feed)]
        if ops == ["Q", "probs"]:
            return [torch_coma(q_m.w, feed), actor.probs_rows(*actor_args(feed))]
        return run_device(ops, feed)

    paths = {"device_networks": lambda: baseline_train_step_feeds(cols, run_device, gamma, eps, target_actor=target_actor, actor=actor,
                                                                  v_target=v_t, v_main=v_m, q_target=q_t, q_main=q_m, env="checkers"),
             "torch_networks_in_run": lambda: baseline_train_step_feeds(cols, run_torch, gamma, eps, env="checkers")}
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
    return {"mode": "batch", "transitions": B, "agents": N, "use_Q": 1, "use_V": 1, "calls_per_repeat": calls, "repeats": REPS,
            **{k + "_us": _stats(v) for k, v in times.items()}, **{k + "_us_all": [round(x, 1) for x in v] for k, v in times.items()}}


def main():
    import torch
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "r30_baseline_checkers_rows.txt")
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
        fh.write("# tools/baseline_checkers_rows_timing.py on %s; us, min / median / max over %d repeats\n" % (torch.cuda.get_device_name(dev), REPS))
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
