#!/usr/bin/env python
"""Timing of the IAC / COMA baseline critics over transition rows (profiles/r29_baseline_rows.txt), one JSON line per mode.

  rows    the three rows launches -- v_rows of a local and of a global value network (V + TD target) and q_rows of the COMA critic
          (Q, the own action's value, TD target) -- at 128 time steps x 4 agents (512 rows) and at 16 384 x 4 (65 536 rows), each
          inside a captured graph of 200 launches, alternating in one process; us per launch, event timing.
  batch   one training batch, 128 transitions x N = 4, both critics on (use_Q = 1, use_V = 1): baseline_train_step_feeds with all
          six device networks end to end (`run` = preallocated answers for the optimiser ops) against the same call without the four
          value networks, where `run` plays V_target / V, Q_target and Q with a torch network (matmuls on the tiled feeds it is handed,
          cast to float32 as a tf.float32 placeholder would) and answers the two actor ops from the same device actors; host wall
          time per call, synchronised.  No time is a pass criterion.

    python tools/baseline_rows_timing.py [rows] [batch] [--out FILE]     (default: both modes, FILE = profiles/r29_baseline_rows.txt)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, LAUNCHES, INNER = 7, 200, 10


def _value_weights(N, kind, rng):
    import numpy as np
    from cm3_amd.baseline import VALUE_NAMES, value_weight_shapes
    return {VALUE_NAMES[kind][s]: (rng.standard_normal(shape) * 0.1).astype(np.float32) for s, shape in value_weight_shapes(N, kind, 2).items()}


def _coma_weights(N, rng):
    import numpy as np
    from cm3_amd.baseline import COMA_NAMES, coma_weight_shapes
    return {COMA_NAMES[s]: (rng.standard_normal(shape) * 0.1).astype(np.float32) for s, shape in coma_weight_shapes(N).items()}


def _actor(N, rng, dev):
    import numpy as np
    from cm3_amd.actor import ParticleActor
    f = lambda *s: (rng.standard_normal(s) * 0.1).astype(np.float32)  # noqa: E731
    w = {"actor_branch_self/kernel": f(6, 64), "actor_branch_self/bias": f(64), "W_branch_self_h2": f(64, 64), "b": f(64),
         "actor_out/kernel": f(64, 5), "actor_out/bias": f(5), "stage-2/actor_others/kernel": f(4 * (N - 1), 128),
         "stage-2/actor_others/bias": f(128), "stage-2/W_others_h2": f(128, 64)}
    return ParticleActor(w, N, stage=2, device=dev)


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
    L = 4 * (N - 1)
    f = lambda *s: torch.as_tensor(rng.standard_normal(s).astype(np.float32), device=dev)          # noqa: E731
    return {"v_global": f(B, N, 4), "obs_others": f(B, N, L), "v_local": f(B, N, 4),
            "actions": torch.as_tensor(rng.integers(0, 5, (B, N)), device=dev), "reward": f(B), "reward_local": f(B, N),
            "v_global_next": f(B, N, 4), "obs_others_next": f(B, N, L), "v_local_next": f(B, N, 4),
            "done": torch.as_tensor(rng.random(B) < 0.1, device=dev), "goals": f(B, N, 2)}


def mode_rows(dev):
    import numpy as np
    import torch
    from cm3_amd import _lib
    from cm3_amd.baseline import ParticleComaCritic, ParticleValue
    N = 4
    rng = np.random.default_rng(0)
    v_l = ParticleValue(_value_weights(N, "local", rng), N, kind="local", device=dev)
    v_g = ParticleValue(_value_weights(N, "global", rng), N, kind="global", device=dev)
    q = ParticleComaCritic(_coma_weights(N, rng), N, device=dev)
    graphs, hold = {}, []
    for B in (128, 16384):
        c = _cols(B, N, rng, dev)
        go, ac, dn = c["goals"], c["actions"].to(torch.int32), c["done"].view(torch.uint8)
        R = B * N
        ov = {"v": torch.empty(R, dtype=torch.float32, device=dev), "v64": torch.empty(R, dtype=torch.float64, device=dev),
              "td": torch.empty(R, dtype=torch.float64, device=dev)}
        oq = {"q": torch.empty(R, 5, dtype=torch.float32, device=dev), "q_taken": torch.empty(R, dtype=torch.float32, device=dev),
              "q_taken64": torch.empty(R, dtype=torch.float64, device=dev), "td": torch.empty(R, dtype=torch.float64, device=dev)}
        hold.append((c, ac, dn, ov, oq))

        def local(stream, c=c, go=go, dn=dn, o=ov, B=B):
            for _ in range(LAUNCHES):
                v_l.enqueue(B, c["v_local_next"], go, c["obs_others_next"], c["reward_local"], dn, 0.99, stream=stream, **o)

        def glob(stream, c=c, go=go, dn=dn, o=ov, B=B):
            for _ in range(LAUNCHES):
                v_g.enqueue(B, c["v_global_next"], go, None, c["reward_local"], dn, 0.99, stream=stream, **o)

        def coma(stream, c=c, go=go, ac=ac, dn=dn, o=oq, B=B):
            for _ in range(LAUNCHES):
                q.enqueue(B, c["v_global_next"], go, c["v_local_next"], ac, ac, c["reward"], dn, 0.99, stream=stream, **o)
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
    from cm3_amd.baseline import ParticleComaCritic, ParticleValue
    from cm3_amd.batch import baseline_train_step_feeds
    N, B, gamma, eps, calls = 4, 128, 0.99, 0.3, 50
    rng = np.random.default_rng(0)
    cols = _cols(B, N, rng, dev)
    v_t, v_m = (ParticleValue(_value_weights(N, "global", rng), N, kind="global", device=dev) for _ in range(2))
    q_t, q_m = (ParticleComaCritic(_coma_weights(N, rng), N, device=dev) for _ in range(2))
    target_actor, actor = _actor(N, rng, dev), _actor(N, rng, dev)
    v_res = torch.zeros(B * N, 1, dtype=torch.float32, device=dev)
    f32 = lambda t: t.to(torch.float32).reshape(t.shape[0], -1)                                     # noqa: E731

    def run_device(ops, feed):
        return [v_res if op == "V" else None for op in ops]

    def torch_value(w, feed):
        b1 = torch.relu(torch.cat([f32(feed["v_state_one_agent"]), f32(feed["v_goal"])], dim=1) @ w["w_b1"] + w["b_b1"])
        b2 = torch.relu(torch.cat([f32(feed["v_state_other_agents"]), f32(feed["v_goal_others"])], dim=1) @ w["w_b2"] + w["b_b2"])
        return torch.relu(b1 @ w["w_b1_h2"] + b2 @ w["w_b2_h2"]) @ w["w_out"]

    def torch_coma(w, feed):
        x = torch.cat([f32(feed[k]) for k in ("v_state", "action_others", "v_goal", "v_goal_others", "v_labels", "v_obs")], dim=1)
        h = torch.relu(torch.relu(x @ w["w_h1"] + w["b_h1"]) @ w["w_h2"] + w["b_h2"])
        return h @ w["w_out"] + w["b_out"]

    def run_torch(ops, feed):
        if ops == ["V_target", "V"]:
            return [torch_value(v_t.w, feed), torch_value(v_m.w, feed)]
        if ops == ["action_samples_target"]:
            return [target_actor.sample_rows(feed["obs_others"], feed["v_obs"], feed["v_goal"], feed["epsilon"])["actions"]]
        if ops == ["Q_target"]:
            return [torch_coma(q_t.w, feed)]
        if ops == ["Q", "probs"]:
            return [torch_coma(q_m.w, feed), actor.probs_rows(feed["obs_others"], feed["v_obs"], feed["v_goal"], feed["epsilon"])]
        return run_device(ops, feed)

    paths = {"device_networks": lambda: baseline_train_step_feeds(cols, run_device, gamma, eps, target_actor=target_actor, actor=actor,
                                                                  v_target=v_t, v_main=v_m, q_target=q_t, q_main=q_m),
             "torch_networks_in_run": lambda: baseline_train_step_feeds(cols, run_torch, gamma, eps)}
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
    out = os.path.join(ROOT, "profiles", "r29_baseline_rows.txt")
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
        fh.write("# tools/baseline_rows_timing.py on %s; us, min / median / max over %d repeats\n" % (torch.cuda.get_device_name(dev), REPS))
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
