#!/usr/bin/env python
"""Timing of the Checkers QMIX target mixer over transition rows (profiles/r28_qmix_mixer_checkers_rows.txt), one JSON line per mode.

  rows    the launch of a train step -- CheckersQmixMixer.q_tot's cm3_qmix_mixer_checkers_rows_f32 with all three outputs (q_tot,
          q_tot64, td) on float64 grids and one-hot goals (what sample_batch returns) -- at 128 and at 16 384 transitions with N = 2 and
          N = 8, each inside a captured graph of 200 launches, alternating in one process; us per launch, event timing.
  batch   one training batch, 128 transitions x N = 2: qmix_train_step_feeds(env="checkers") with target_agent and target_mixer end to
          end against the same call on the path without target_mixer, where `run` answers mixer_target with a torch mixer of the same
          weights (a convolution and matmuls on the arrays it is fed, agent_qs from the target agent's Q values times the fed one-hot
          actions); host wall time per call, synchronised, both in the same process.  No time is a pass criterion.

    python tools/qmix_mixer_checkers_timing.py [rows] [batch] [--out FILE]
                                                         (default: both modes, FILE = profiles/r28_qmix_mixer_checkers_rows.txt)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, LAUNCHES, INNER = 7, 200, 10
EMBED = 128


def _mixer_weights(N, rng):
    import numpy as np
    K = 108 + 6 * N
    f = lambda *s: (rng.standard_normal(s) * 0.5 / np.sqrt(np.prod(s[:-1]) if len(s) > 1 else 4)).astype(np.float32)  # noqa: E731
    return {"conv/Conv/weights": f(3, 5, 2, 4), "conv/Conv/biases": f(4), "hyper_w_1": f(K, EMBED * N), "hyper_w_final": f(K, EMBED),
            "hyper_b_1": f(K, EMBED), "hyper_b_final_l1/kernel": f(K, EMBED), "hyper_b_final/kernel": f(EMBED, 1)}


def _agent_weights(N, rng):
    import numpy as np
    from cm3_amd.actor import checkers_policy_shapes
    from cm3_amd.qmix import CK_NAMES
    f = lambda s: (rng.standard_normal(s) / np.sqrt(np.prod(s[:-1]) if len(s) > 1 else 4)).astype(np.float32)  # noqa: E731
    return {CK_NAMES[short]: f(shape) for short, shape in checkers_policy_shapes(2 * max(N - 1, 1)).items()}


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
    """the 16 columns of a sampled Checkers batch in the forms sample_batch returns"""
    import numpy as np
    import torch
    Lo = 2 * max(N - 1, 1)
    u = lambda lo, *s: torch.as_tensor(rng.uniform(-lo, lo, s), device=dev)                                  # noqa: E731
    grid = lambda: torch.as_tensor(rng.integers(0, 2, (B, 3, 9, 2)).astype(np.float64), device=dev)          # noqa: E731
    win = lambda: torch.as_tensor(rng.integers(-1, 2, (B, N, 5, 5, 3)).astype(np.float64), device=dev)       # noqa: E731
    act = lambda: torch.as_tensor(rng.integers(0, 5, (B, N)).astype(np.int32), device=dev)                   # noqa: E731
    return {"grid": grid(), "vec": u(2, B, N, 4), "obs_others": u(1, B, N, Lo), "obs_self_t": win(), "obs_self_v": u(1, B, N, 4),
            "actions_prev": act(), "actions": act(), "reward": u(1, B), "local_rewards": u(1, B, N), "next_grid": grid(),
            "next_vec": u(2, B, N, 4), "next_obs_others": u(1, B, N, Lo), "next_obs_self_t": win(), "next_obs_self_v": u(1, B, N, 4),
            "done": torch.as_tensor(rng.random(B) < 0.1, device=dev),
            "goals": torch.as_tensor(np.eye(2, dtype=np.int64)[rng.integers(0, 2, (B, N))], device=dev)}


def mode_rows(dev):
    import numpy as np
    import torch
    from cm3_amd import _lib
    from cm3_amd.qmix import CheckersQmixMixer
    rng = np.random.default_rng(0)
    graphs, hold = {}, []
    for N in (2, 8):
        mixer = CheckersQmixMixer(_mixer_weights(N, rng), N, device=dev)
        for B in (128, 16384):
            c = _cols(B, N, rng, dev)
            agent_qs = torch.as_tensor(rng.uniform(-5, 5, (B, N)).astype(np.float32), device=dev)
            args = (c["next_grid"].reshape(B, 54), c["next_vec"], c["goals"], agent_qs, c["local_rewards"], c["done"].view(torch.uint8))
            out = {"q_tot": torch.empty(B, dtype=torch.float32, device=dev), "q_tot64": torch.empty(B, dtype=torch.float64, device=dev),
                   "td": torch.empty(B, dtype=torch.float64, device=dev)}
            hold.append((mixer, c, args, out))

            def rows(stream, m=mixer, a=args, o=out, b=B, n=LAUNCHES):
                for _ in range(n):
                    m.enqueue(b, *a, 0.99, stream=stream, **o)
            graphs["q_tot_n%d_%d" % (N, B)] = (_lib.capture_graph(dev, rows), LAUNCHES)
    for g, n in graphs.values():
        _time_graph(g, dev, n)
    times = {k: [] for k in graphs}
    for _ in range(REPS):
        for k, (g, n) in graphs.items():
            times[k].append(_time_graph(g, dev, n))
    torch.cuda.synchronize()
    for g, _ in graphs.values():
        _lib.lib().cm3_graph_destroy(g)
    return {"mode": "rows", "launches_per_graph": LAUNCHES, "replays": INNER, "repeats": REPS,
            **{k + "_us": _stats(v) for k, v in times.items()}, **{k + "_us_all": [round(x, 3) for x in v] for k, v in times.items()}}


def mode_batch(dev):
    import numpy as np
    import torch
    from cm3_amd.batch import qmix_train_step_feeds
    from cm3_amd.qmix import CheckersQmixAgent, CheckersQmixMixer
    N, B, gamma, calls = 2, 128, 0.99, 50
    rng = np.random.default_rng(0)
    cols = _cols(B, N, rng, dev)
    agent = CheckersQmixAgent(_agent_weights(N, rng), N, device=dev)
    mixer = CheckersQmixMixer(_mixer_weights(N, rng), N, device=dev)
    w = mixer.w
    kernel = w["conv_w"].permute(3, 2, 0, 1).contiguous()                                               # [kh][kw][C][F] -> [F][C][kh][kw]

    def run_device(ops, feed):
        return [None]

    def run_torch(ops, feed):
        if ops != ["mixer_target"]:
            return [None]
        f32 = lambda t: t.to(torch.float32)                                                         # noqa: E731
        q = agent.greedy_rows(feed["obs_self_t"], feed["obs_self_v"], feed["obs_others"], feed["actions_prev"].argmax(1), feed["v_goal"],
                              q=True, onehot=False)["q"]
        agent_qs = (q * f32(feed["actions_1hot"])).sum(dim=1).reshape(B, 1, N)
        conv = torch.relu(torch.nn.functional.conv2d(f32(feed["state_env"]).permute(0, 3, 1, 2), kernel, w["conv_b"], padding=(1, 2)))
        x = torch.cat([conv.permute(0, 2, 3, 1).reshape(B, 108), f32(feed["v_state"]), f32(feed["v_goal_all"])], dim=1)
        b_final = torch.relu(x @ w["hyper_b_final_l1"]) @ w["hyper_b_final"]
        hidden = torch.nn.functional.elu(agent_qs @ torch.abs(x @ w["hyper_w_1"]).reshape(B, N, EMBED) + (x @ w["hyper_b_1"]).reshape(B, 1, EMBED))
        return [(hidden @ torch.abs(x @ w["hyper_w_final"]).reshape(B, EMBED, 1) + b_final.reshape(B, 1, 1)).reshape(B, 1)]

    paths = {"device_target_mixer": lambda: qmix_train_step_feeds(cols, run_device, gamma, target_agent=agent, target_mixer=mixer, env="checkers"),
             "torch_mixer_in_run": lambda: qmix_train_step_feeds(cols, run_torch, gamma, target_agent=agent, env="checkers")}
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
    out = os.path.join(ROOT, "profiles", "r28_qmix_mixer_checkers_rows.txt")
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
        fh.write("# tools/qmix_mixer_checkers_timing.py on %s; us, min / median / max over %d repeats\n" % (torch.cuda.get_device_name(dev), REPS))
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
