#!/usr/bin/env python
"""Timing of the particle QMIX target mixer over transition rows (profiles/r26_qmix_mixer_rows.txt), one JSON line per mode.

  rows    the launch of a train step -- ParticleQmixMixer.q_tot's cm3_qmix_mixer_particle_rows_f32 with all three outputs (q_tot,
          q_tot64, td) -- at 128 and at 16 384 transitions with N = 4 and N = 8, each inside a captured graph of 200 launches,
          alternating in one process; us per launch, event timing.
  batch   one training batch, 128 transitions x N = 4: qmix_train_step_feeds with target_agent and target_mixer end to end against
          the same call on the path without target_mixer, where `run` answers mixer_target with a torch mixer of the same weights
          (matmuls on the arrays it is fed, agent_qs from the target agent's Q values times the fed one-hot actions); host wall
          time per call, synchronised, both in the same process.  No time is a pass criterion.

    python tools/qmix_mixer_timing.py [rows] [batch] [--out FILE]     (default: both modes, FILE = profiles/r26_qmix_mixer_rows.txt)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, LAUNCHES, INNER = 7, 200, 10


def _mixer_weights(N, rng):
    import numpy as np
    K = 6 * N
    f = lambda *s: (rng.standard_normal(s) * 0.5 / np.sqrt(s[0])).astype(np.float32)  # noqa: E731
    return {"hyper_w_1": f(K, 64 * N), "hyper_w_final": f(K, 64), "hyper_b_1": f(K, 64), "hyper_b_final_l1/kernel": f(K, 64),
            "hyper_b_final/kernel": f(64, 1)}


def _agent_weights(N, rng):
    import numpy as np
    k = 4 * max(N - 1, 1) + 6
    f = lambda *s: (rng.standard_normal(s) / np.sqrt(s[0] if len(s) > 1 else 4)).astype(np.float32)  # noqa: E731
    return {"h/kernel": f(k, 64), "h/bias": f(64), "h2/kernel": f(64, 64), "h2/bias": f(64), "out/kernel": f(64, 5), "out/bias": f(5)}


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
    L = 4 * max(N - 1, 1)
    f = lambda *s: torch.as_tensor(rng.standard_normal(s).astype(np.float32), device=dev)          # noqa: E731
    return {"v_global": f(B, N, 4), "obs_others": f(B, N, L), "v_local": f(B, N, 4),
            "actions": torch.as_tensor(rng.integers(0, 5, (B, N)), device=dev), "reward": f(B), "reward_local": f(B, N),
            "v_global_next": f(B, N, 4), "obs_others_next": f(B, N, L), "v_local_next": f(B, N, 4),
            "done": torch.as_tensor(rng.random(B) < 0.1, device=dev), "goals": f(B, N, 2)}


def mode_rows(dev):
    import numpy as np
    import torch
    from cm3_amd import _lib
    from cm3_amd.qmix import ParticleQmixMixer
    rng = np.random.default_rng(0)
    graphs, hold = {}, []
    for N in (4, 8):
        mixer = ParticleQmixMixer(_mixer_weights(N, rng), N, device=dev)
        for B in (128, 16384):
            c = _cols(B, N, rng, dev)
            args = (c["v_global_next"], c["goals"], c["reward_local"].clone(), c["reward_local"], c["done"].view(torch.uint8))
            out = {"q_tot": torch.empty(B, dtype=torch.float32, device=dev), "q_tot64": torch.empty(B, dtype=torch.float64, device=dev),
                   "td": torch.empty(B, dtype=torch.float64, device=dev)}
            hold.append((mixer, c, args, out))

            def rows(stream, m=mixer, a=args, o=out, n=LAUNCHES):
                for _ in range(n):
                    m.enqueue(a[0].shape[0], *a, 0.99, stream=stream, **o)
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
    from cm3_amd.qmix import ParticleQmixAgent, ParticleQmixMixer
    N, B, gamma, calls = 4, 128, 0.99, 50
    rng = np.random.default_rng(0)
    cols = _cols(B, N, rng, dev)
    agent = ParticleQmixAgent(_agent_weights(N, rng), N, device=dev)
    mixer = ParticleQmixMixer(_mixer_weights(N, rng), N, device=dev)
    w = mixer.w

    def run_device(ops, feed):
        return [None]

    def run_torch(ops, feed):
        if ops != ["mixer_target"]:
            return [None]
        f32 = lambda t: t.to(torch.float32)                                                         # noqa: E731
        q = agent.greedy_rows(feed["obs_others"], feed["v_obs"], feed["v_goal"], q=True, onehot=False)["q"]
        agent_qs = (q * f32(feed["actions_1hot"])).sum(dim=1).reshape(B, 1, N)
        x = torch.cat([f32(feed["v_state"]), f32(feed["v_goal_all"])], dim=1)
        b_final = torch.relu(x @ w["b_final_l1"]) @ w["b_final"]
        hidden = torch.nn.functional.elu(agent_qs @ torch.abs(x @ w["w1"]).reshape(B, N, 64) + (x @ w["b1"]).reshape(B, 1, 64))
        return [(hidden @ torch.abs(x @ w["w_final"]).reshape(B, 64, 1) + b_final.reshape(B, 1, 1)).reshape(B, 1)]

    paths = {"device_target_mixer": lambda: qmix_train_step_feeds(cols, run_device, gamma, target_agent=agent, target_mixer=mixer),
             "torch_mixer_in_run": lambda: qmix_train_step_feeds(cols, run_torch, gamma, target_agent=agent)}
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
    out = os.path.join(ROOT, "profiles", "r26_qmix_mixer_rows.txt")
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
        fh.write("# tools/qmix_mixer_timing.py on %s; us, min / median / max over %d repeats\n" % (torch.cuda.get_device_name(dev), REPS))
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
