#!/usr/bin/env python
"""Timing of the counted actor rows launches and of an on-policy phase with device actors inside OnPolicyPhasePlan
(profiles/r23_rows_counter.txt), one JSON line per mode.

  launch  the actor rows SAMPLING launch (actions only) at 16 384 rows, particle N = 4 and Checkers N = 2 (int8 windows), every
          precision: the uncounted launch (an integer draw), and -- where the tree has cm3_amd.actor.RowsDrawCounter -- the counted
          one (the launches of a graph share one counter; they are ordered by the captured stream).  us per launch from event timing
          over replays of a captured graph of LAUNCHES launches.  The uncounted figure is the one to compare with the parent: run
          this mode on both trees ALTERNATELY, five processes each (--tree names the checkout whose cm3_amd is imported; the
          parent's has no counted launch, which is then left out), and compare the branch's medians with the parent's min-max over
          its processes.
  phase   one phase end to end -- collect 330 ticks, draw and export 24 minibatches of 128, every feed of 24 train_steps with BOTH
          actor evaluations on the device -- at C2 (particle, 4096 envs x 4 agents, actors f16x3) and C3 (Checkers, 8192 envs x 2
          agents, actors f16x3), in three arrangements: plan_actors (OnPolicyPhasePlan(target_actor=, actor=): one graph replay per
          train_step, the sampling launch counted), eager_actors (on_policy_phase + train_step_feeds(target_actor=, actor=) per
          minibatch, the host draw counter) and plan_stub (OnPolicyPhasePlan without actors, `run` answering the two actor ops from
          preallocated tensors).  Wall time per phase, synchronised; this tree only.

    python tools/rows_counter_timing.py [launch] [phase] [--tree PATH] [--tag NAME]
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPS, LAUNCHES, INNER = 5, 200, 10
PRECISIONS = ("f32", "f16x3", "bf16")
ROWS = 16384


def _stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def _time_graph(graph, dev):
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


def _particle_weights(N, rng):
    import numpy as np
    L = 4 * (N - 1)
    f = lambda *s: (rng.standard_normal(s) * 0.1).astype(np.float32)  # noqa: E731
    return {"actor_branch_self/kernel": f(6, 64), "actor_branch_self/bias": f(64), "W_branch_self_h2": f(64, 64), "b": f(64),
            "actor_out/kernel": f(64, 5), "actor_out/bias": f(5), "stage-2/actor_others/kernel": f(L, 128),
            "stage-2/actor_others/bias": f(128), "stage-2/W_others_h2": f(128, 64)}


def _checkers_weights(N, rng):
    import numpy as np
    Lo = 2 * max(N - 1, 1)
    shapes = {"conv/Conv/weights": (3, 3, 3, 6), "conv/Conv/biases": (6,), "conv_linear/kernel": (150, 32), "conv_linear/bias": (32,),
              "branch_self/kernel": (43, 256), "branch_self/bias": (256,), "W_self_h2": (256, 256),
              "stage-2/branch_others/kernel": (Lo, 256), "stage-2/branch_others/bias": (256,), "stage-2/W_others_h2": (256, 256),
              "b": (256,), "actor_out/kernel": (256, 5), "actor_out/bias": (5,)}
    return {k: (rng.standard_normal(s) / np.sqrt(max(s[0], 4))).astype(np.float32) for k, s in shapes.items()}


def mode_launch(dev):
    import numpy as np
    import torch
    from cm3_amd import _lib
    from cm3_amd import actor as A
    counted = hasattr(A, "RowsDrawCounter")
    rng = np.random.default_rng(0)
    R = ROWS
    t = lambda a, dt: torch.as_tensor(a, dtype=dt, device=dev)  # noqa: E731
    p_in = (t(rng.standard_normal((R, 12)), torch.float32), t(rng.standard_normal((R, 4)), torch.float32),
            t(rng.uniform(-1, 1, (R, 2)), torch.float32))
    c_in = (t(rng.integers(-1, 2, (R, 75)), torch.int8), t(rng.uniform(-0.5, 1.0, (R, 4)), torch.float64),
            t(rng.uniform(-1, 1, (R, 2)), torch.float64), t(rng.integers(0, 5, R), torch.int32), t(rng.integers(0, 2, R), torch.uint8))
    actions = torch.empty(R, dtype=torch.int32, device=dev)
    graphs, keep = {}, []
    for precision in PRECISIONS:
        for env, actor, inputs in (("particle_n4", A.ParticleActor(_particle_weights(4, np.random.default_rng(1)), 4, stage=2, device=dev,
                                                                   precision=precision), p_in),
                                   ("checkers_n2", A.CheckersActor(_checkers_weights(2, np.random.default_rng(1)), 2, stage=2, device=dev,
                                                                   precision=precision), c_in)):
            keep.append(actor)
            draws = {"uncounted": 3}
            if counted:
                draws["counted"] = A.RowsDrawCounter(dev, 3)
            for name, draw in draws.items():
                def enqueue(stream, actor=actor, inputs=inputs, draw=draw):
                    for _ in range(LAUNCHES):
                        actor.enqueue_rows(R, *inputs, 0.3, actions=actions, draw=draw, stream=stream)
                graphs["%s_%s_%s" % (env, precision, name)] = _lib.capture_graph(dev, enqueue)
    for g in graphs.values():
        _time_graph(g, dev)
    times = {k: [] for k in graphs}
    for _ in range(REPS):
        for k, g in graphs.items():
            times[k].append(_time_graph(g, dev))
    torch.cuda.synchronize()
    for g in graphs.values():
        _lib.lib().cm3_graph_destroy(g)
    out = {"mode": "launch", "rows": R, "launches_per_graph": LAUNCHES, "replays": INNER, "repeats": REPS, "unit": "us per launch"}
    out.update({k: _stats(v) for k, v in times.items()})
    return out


def _answers(B, N, dev):
    import torch
    z = lambda n: torch.zeros(n, 1, dtype=torch.float64, device=dev)                                # noqa: E731
    ans = {"Q_global_target": z(B * N), "Q_global": z(B * N), "Q_credit_target": z(B * N * N), "V_target": z(B * N), "V": z(B * N),
           "Q_credit": z(B * N * N * 5), "action_samples_target": torch.zeros(B * N, dtype=torch.int64, device=dev),
           "probs": torch.full((B * N, 5), 0.2, dtype=torch.float64, device=dev)}
    return lambda ops, feed: [ans.get(op) for op in ops]


def _wall_ms(fn, dev):
    import torch
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def _phase(dev, env_name, ro, N, main, target):
    import torch
    from cm3_amd import batch as BR
    M, B, eps = 24, 128, 0.3
    run = _answers(B, N, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    kw = {"env": env_name}
    plan_a = BR.OnPolicyPhasePlan(ro, run, 0.99, eps, epochs=M, batch_size=B, target_actor=target, actor=main)
    plan_s = BR.OnPolicyPhasePlan(ro, run, 0.99, eps, epochs=M, batch_size=B)

    def planned(plan):
        def fn():
            ro.collect()
            plan.refresh(gen)
            for k in range(M):
                plan.step(k)
        return fn

    def eager_actors():
        ro.collect()
        for cols, static in ro.on_policy_phase(M, B, gen):
            BR.train_step_feeds(cols, run, 0.99, eps, static=static, target_actor=target, actor=main, **kw)
    paths = {"plan_actors": planned(plan_a), "eager_actors": eager_actors, "plan_stub": planned(plan_s), "collect_only": lambda: ro.collect()}
    for fn in paths.values():
        for _ in range(2):
            _wall_ms(fn, dev)
    times = {k: [] for k in paths}
    for _ in range(7):
        for k, fn in paths.items():
            times[k].append(_wall_ms(fn, dev))
    draws = plan_a.draw_counter.value()
    plan_a.close()
    plan_s.close()
    out = {k + "_ms": _stats(v) for k, v in times.items()}
    out["plan_actors_draws"] = draws                      # one per step(k): (2 + 7) phases x 24
    return out


def mode_phase(dev):
    import numpy as np
    import cm3_amd
    from cm3_amd import actor as A
    from cm3_amd.checkers import VecCheckersEnv
    from cm3_amd.particle import VecParticleEnv
    from cm3_amd.rollout import CheckersRollout, ParticleRollout
    import torch
    out = {"mode": "phase", "ticks": 330, "minibatches": 24, "transitions": 128, "actors": "f16x3", "unit": "ms per phase"}
    env = VecParticleEnv(cm3_amd.load_config("particle_stage2_antipodal"), 4, 0.2, 33, 4096, device=dev, dtype=torch.float32,
                         auto_reset=True, seed=12341)
    env.reset()
    ro = ParticleRollout(env, n_ticks=330)
    ro.collect()
    mk = lambda s: A.ParticleActor(_particle_weights(4, np.random.default_rng(s)), 4, stage=2, device=dev, precision="f16x3")  # noqa: E731
    out["C2_particle_4096x4"] = _phase(dev, "particle", ro, 4, mk(1), mk(2))
    ro.close()
    cfg = cm3_amd.load_config("checkers_stage2")
    cenv = VecCheckersEnv(cfg["init"], 2, 33, 8192, device=dev, seed=12341, auto_reset=True)
    cro = CheckersRollout(cenv, n_ticks=330)
    cro.collect(np.eye(2))
    mk = lambda s: A.CheckersActor(_checkers_weights(2, np.random.default_rng(s)), 2, stage=2, device=dev, precision="f16x3")  # noqa: E731
    out["C3_checkers_8192x2"] = _phase(dev, "checkers", cro, 2, mk(1), mk(2))
    cro.close()
    return out


def main():
    args = sys.argv[1:]
    tag, tree = None, os.path.dirname(HERE)
    for flag in ("--tag", "--tree"):
        if flag in args:
            k = args.index(flag)
            if flag == "--tag":
                tag = args[k + 1]
            else:
                tree = os.path.abspath(args[k + 1])
            del args[k:k + 2]
    sys.path.insert(0, tree)
    import torch
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    modes = {"launch": mode_launch, "phase": mode_phase}
    for m in args or list(modes):
        res = modes[m](dev)
        if tag:
            res["tag"] = tag
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
