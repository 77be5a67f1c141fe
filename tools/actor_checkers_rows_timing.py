#!/usr/bin/env python
"""Timing of the CM3 Checkers actor over transition rows (profiles/r20_actor_checkers_rows.txt), one JSON line per mode.

  rows    the rows kernels against the kernels they share their layers with: 16 384 rows at N = 2 (8192 envs x 2 agents, stage 2).
          Per precision ("f32", "f16x3", "bf16"): CheckersActor.enqueue_rows with only `probs` requested (the probs fetch) on int8
          windows / uint8 goal index and on float64 windows / int64 one-hot goals (600 B per row more), with only `actions` (the
          draw, int8 windows), and actor.enqueue's launch (actions only) on the same rows handed over as the env does -- records
          of 152 bytes (padded: the dword staging path) and of 150 bytes (the byte path).  Each inside a captured graph of 200
          launches (the same launch gap for all), all alternating in one process; us per launch, event timing.
  batch   one training batch, 128 transitions x N = 2 (256 rows, launch-bound): train_step_feeds(env="checkers") with
          target_actor and actor end to end (`run` = preallocated answers for the critics) against the same call without them,
          where `run` plays the two actor ops with a torch network (conv2d, five matmuls, softmax, mixing, torch.multinomial);
          host wall time per call, synchronised.

    python tools/actor_checkers_rows_timing.py [rows] [batch] [--out FILE] [--isa FILE]
        (default: both modes, FILE = profiles/r20_actor_checkers_rows.txt; --isa: a text file -- the result of tools/isa_diff.py --all
         on the actor_checkers / policy_checkers translation units against the parent commit -- copied in behind the measurements)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, LAUNCHES, INNER = 7, 200, 10
PRECISIONS = ("f32", "f16x3", "bf16")


def _weights(N, rng):
    import numpy as np
    Lo = 2 * max(N - 1, 1)
    shapes = {"conv/Conv/weights": (3, 3, 3, 6), "conv/Conv/biases": (6,), "conv_linear/kernel": (150, 32), "conv_linear/bias": (32,),
              "branch_self/kernel": (43, 256), "branch_self/bias": (256,), "W_self_h2": (256, 256),
              "stage-2/branch_others/kernel": (Lo, 256), "stage-2/branch_others/bias": (256,), "stage-2/W_others_h2": (256, 256),
              "b": (256,), "actor_out/kernel": (256, 5), "actor_out/bias": (5,)}
    return {k: (rng.standard_normal(s) / np.sqrt(max(s[0], 4))).astype(np.float32) for k, s in shapes.items()}


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
    from cm3_amd.actor import CheckersActor
    N, E = 2, 8192
    R, Lo = E * N, 2
    rng = np.random.default_rng(0)
    t = lambda a, dt: torch.as_tensor(a, dtype=dt, device=dev)  # noqa: E731
    raw150 = t(rng.integers(-1, 2, (E, 75 * N)), torch.int8)
    raw152 = torch.zeros(E, 152, dtype=torch.int8, device=dev)
    raw152[:, :150] = raw150
    v = t(rng.uniform(-0.5, 1.0, (E, N, 4)), torch.float64)
    oo = t(rng.uniform(-1, 1, (E, N, Lo)), torch.float64)
    goals = t(rng.integers(0, 2, (E, N)), torch.uint8)
    prev = t(rng.integers(0, 5, (E, N)), torch.int32)
    steps, episode = t(rng.integers(0, 33, E), torch.int32), t(rng.integers(0, 1 << 20, E), torch.int32)
    narrow_t, wide_t = raw150.view(R, 75), raw150.view(R, 75).double()
    wide_g = torch.nn.functional.one_hot(goals.view(R).long(), 2).contiguous()
    act_out = torch.empty(E, N, dtype=torch.int32, device=dev)
    actions = torch.empty(R, dtype=torch.int32, device=dev)
    probs = torch.empty(R, 5, dtype=torch.float32, device=dev)
    out = {"mode": "rows", "rows": R, "agents": N, "launches_per_graph": LAUNCHES, "replays": INNER, "repeats": REPS}
    graphs = {}
    actors = []
    for precision in PRECISIONS:
        actor = CheckersActor(_weights(N, np.random.default_rng(1)), N, stage=2, device=dev, precision=precision)
        actors.append(actor)

        def rows_graph(ot, vg, outputs, actor=actor):
            def enqueue(stream):
                for _ in range(LAUNCHES):
                    actor.enqueue_rows(R, ot, v.view(R, 4), oo.view(R, Lo), prev.view(R), vg, 0.3, stream=stream, **outputs)
            return _lib.capture_graph(dev, enqueue)

        def act_graph(raw, stride, actor=actor):
            def enqueue(stream):
                for _ in range(LAUNCHES):
                    actor.enqueue(E, raw, stride, v, oo, goals, prev, steps, episode, act_out, 0.3, stream=stream)
            return _lib.capture_graph(dev, enqueue)
        graphs[precision + "_rows_probs_narrow"] = rows_graph(narrow_t, goals.view(R), {"probs": probs})
        graphs[precision + "_rows_probs_wide"] = rows_graph(wide_t, wide_g, {"probs": probs})
        graphs[precision + "_rows_actions_narrow"] = rows_graph(narrow_t, goals.view(R), {"actions": actions})
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
    from cm3_amd.actor import CheckersActor
    from cm3_amd.batch import train_step_feeds
    from cm3_amd.checkers import VecCheckersEnv
    from cm3_amd.replay import DeviceReplayBuffer
    from cm3_amd.rollout import CheckersRollout
    N, E, T, B, gamma, eps, calls = 2, 64, 8, 128, 0.99, 0.3, 50
    out = {"mode": "batch", "transitions": B, "agents": N, "calls_per_repeat": calls, "repeats": REPS}
    cfg = cm3_amd.load_config("checkers_stage2")
    z = lambda n: torch.zeros(n, 1, dtype=torch.float64, device=dev)                                # noqa: E731
    answers = {"Q_global_target": z(B * N), "Q_global": z(B * N), "Q_credit_target": z(B * N * N), "V_target": z(B * N), "V": z(B * N),
               "Q_credit": z(B * N * N * 5)}
    for precision in ("f32", "f16x3"):
        main = CheckersActor(_weights(N, np.random.default_rng(0)), N, stage=2, device=dev, precision=precision)
        target = CheckersActor(_weights(N, np.random.default_rng(1)), N, stage=2, device=dev, precision=precision)
        env = VecCheckersEnv(cfg["init"], N, 33, E, device=dev, seed=12341, auto_reset=True)
        ro = CheckersRollout(env, n_ticks=T)
        ro.collect(np.eye(2), policy=main, epsilon=eps)
        buf = DeviceReplayBuffer(size=E * T, device=dev)
        buf.add_rollout(ro)
        cols = buf.sample_batch(B, generator=torch.Generator(device=dev).manual_seed(0))

        def run_device(ops, feed):
            return [answers.get(op) for op in ops]

        def torch_probs(w, feed):
            f32 = torch.float32
            conv_w = w["conv_w"].permute(3, 2, 0, 1)                              # HWIO -> OIHW
            x = feed["obs_self_t"].to(f32).permute(0, 3, 1, 2)
            c = torch.relu(torch.nn.functional.conv2d(x, conv_w, w["conv_b"], padding=1)).permute(0, 2, 3, 1).reshape(x.shape[0], -1)
            lin = torch.relu(c @ w["lin_w"] + w["lin_b"])
            cat = torch.cat([lin, feed["obs_self_v"].to(f32), feed["actions_prev"].to(f32), feed["v_goal"].to(f32)], dim=1)
            hs = torch.relu(cat @ w["self_w"] + w["self_b"])
            ho = torch.relu(feed["obs_others"].to(f32) @ w["others_w"] + w["others_b"])
            h2 = torch.relu(hs @ w["w_self_h2"] + ho @ w["w_others_h2"] + w["b_h2"])
            return (1.0 - eps) * torch.softmax(h2 @ w["out_w"] + w["out_b"], dim=1) + eps / 5.0

        def run_torch(ops, feed):
            if ops == ["action_samples_target"]:
                return [torch.multinomial(torch_probs(target.w, feed), 1).reshape(-1)]
            if ops == ["probs"]:
                return [torch_probs(main.w, feed)]
            return run_device(ops, feed)

        paths = {"device_actors": lambda: train_step_feeds(cols, run_device, gamma, eps, env="checkers", target_actor=target, actor=main),
                 "torch_actors_in_run": lambda: train_step_feeds(cols, run_torch, gamma, eps, env="checkers")}
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
    args = sys.argv[1:]
    opts = {"--out": os.path.join(ROOT, "profiles", "r20_actor_checkers_rows.txt"), "--isa": None}
    for name in opts:
        if name in args:
            k = args.index(name)
            opts[name] = args[k + 1]
            del args[k:k + 2]
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    modes = {"rows": mode_rows, "batch": mode_batch}
    lines = []
    for m in args or ["rows", "batch"]:
        lines.append(json.dumps(modes[m](dev)))
        print(lines[-1], flush=True)
    with open(opts["--out"], "w") as fh:
        fh.write("# tools/actor_checkers_rows_timing.py on %s; us, min / median / max over %d repeats\n"
                 % (torch.cuda.get_device_name(dev), REPS))
        fh.write("\n".join(lines) + "\n")
        if opts["--isa"]:
            fh.write("# instruction streams against the parent commit (tools/isa_diff.py --all)\n" + open(opts["--isa"]).read())


if __name__ == "__main__":
    main()
