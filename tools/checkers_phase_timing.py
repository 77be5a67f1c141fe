#!/usr/bin/env python
"""Timing of the data side of a Checkers on-policy phase (profiles/r21_checkers_phase.txt), one JSON line per mode.  Runs on this
commit and on its parent (copy this file into a checkout of the parent: what the parent lacks is measured as the eager path only);
run the two alternately, one process each, and take the median over the processes.

  feeds   cm3_amd.batch.train_step_feeds(env="checkers") with its defaults: one call at 128 transitions x 2 agents, `run` =
          preallocated answers; host wall time per call, synchronised.
  static  the static set of a phase of 24 x 128 transitions at N = 2: checkers_static_feeds_device (three tiling launches) against
          the same tensors from the torch composition (process_batch_checkers, rep_rows, gather_others, one_hot, eye); wall time
          per set, synchronised.  (This commit only.)
  phase   one phase end to end at C3 (8192 envs, 330 ticks, continuous): collect, draw and export 24 minibatches of 128, every feed
          of 24 train_steps.  eager: on_policy_minibatches + train_step_feeds per minibatch; plan: OnPolicyPhasePlan (refresh + 24
          graph replays; this commit only).  Wall time per phase, synchronised.
  rows    cm3_rows_tile on ONE CM3_TILE_COPY column, 61 440 destination rows (24 x 128 x 2 x 2 x 5) <- 6144 source rows, row sizes
          16 .. 600 bytes; us per launch from event timing over a captured graph of 50 launches.  Run once per library build
          (CM3_AMD_LIB = a build of tools/variants/build_tile_threshold.sh) to compare the row path with the element path.

    python tools/checkers_phase_timing.py [feeds] [static] [phase] [rows] [--tag NAME]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 7
ROW_SIZES = (16, 32, 48, 64, 80, 96, 128, 216, 432, 600)


def _stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}


def _wall(fn, calls, dev):
    import torch
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e6 / calls


def _answers(B, N, dev):
    import torch
    z = lambda n: torch.zeros(n, 1, dtype=torch.float64, device=dev)                                # noqa: E731
    ans = {"Q_global_target": z(B * N), "Q_global": z(B * N), "Q_credit_target": z(B * N * N), "V_target": z(B * N), "V": z(B * N),
           "Q_credit": z(B * N * N * 5), "action_samples_target": torch.zeros(B * N, dtype=torch.int64, device=dev),
           "probs": torch.full((B * N, 5), 0.2, dtype=torch.float64, device=dev)}
    return lambda ops, feed: [ans.get(op) for op in ops]


def _rollout(dev, E, T):
    import numpy as np
    import cm3_amd
    from cm3_amd.checkers import VecCheckersEnv
    from cm3_amd.rollout import CheckersRollout
    cfg = cm3_amd.load_config("checkers_stage2")
    env = VecCheckersEnv(cfg["init"], 2, 33, E, device=dev, seed=12341, auto_reset=True)
    ro = CheckersRollout(env, n_ticks=T)
    ro.collect(np.eye(2))
    return ro


def mode_feeds(dev):
    import torch
    from cm3_amd.batch import train_step_feeds
    B, N, calls = 128, 2, 50
    ro = _rollout(dev, 64, 8)
    cols = ro.sample_batch(B, generator=torch.Generator(device=dev).manual_seed(0), numpy=False)
    run = _answers(B, N, dev)
    fn = lambda: train_step_feeds(cols, run, 0.99, 0.3, env="checkers")                             # noqa: E731
    _wall(fn, 10, dev)
    times = [_wall(fn, calls, dev) for _ in range(REPS)]
    ro.close()
    return {"mode": "feeds", "transitions": B, "agents": N, "calls_per_repeat": calls, "us_per_call": _stats(times),
            "all": [round(t, 1) for t in times]}


def _static_composition(cols, l_action=5):
    """the tensors of checkers_static_feeds_device as train_step_feeds composes them without the tiling kernel"""
    import torch
    from cm3_amd import batch as BR
    N = cols["vec"].shape[1]
    (_, state_env, vec, _, ot, ov, prev1, a1, ao, _, r_local, state_env_next, vec_next, _, ot_next, ov_next, done,
     goals) = BR.process_batch_checkers(cols, l_action)
    goals_self, _ = BR.process_goals(goals)
    one, others, _ = BR.process_global_state(vec)
    one_next, others_next, _ = BR.process_global_state(vec_next)
    rep_m, rep_n, rep_a = (lambda x: BR.rep_rows(x, N)), (lambda x: BR.repeat_indexed_by_n(x, N)), (lambda x: BR.rep_rows(x, l_action))
    S = dict(state_env=state_env, state_env_next=state_env_next, a1=a1, ao=ao, prev1=prev1, done_rep=done,
             not_done=-(done.to(torch.int64) - 1), others=others, others_next=others_next, goals_self_rep=rep_n(goals_self),
             one_next_rep_n=rep_n(one_next), one_next_rep_m=rep_m(one_next), others_next_rep_n=rep_n(others_next),
             r_rep=rep_n(r_local.reshape(-1, 1)).reshape(-1), nd_rep=-(rep_n(done.reshape(-1, 1).to(torch.int64)).reshape(-1) - 1),
             s_n_rep=rep_n(one), s_m_rep=rep_m(one), s_others_rep=rep_n(others), a1_rep_m=rep_m(a1),
             env_next_rep=rep_m(state_env_next), ot_next_rep=rep_m(ot_next), ov_next_rep=rep_m(ov_next),
             env_rep=rep_m(state_env), ot_rep=rep_m(ot), ov_rep=rep_m(ov))
    S.update(cf_s_n=rep_a(S["s_n_rep"]), cf_goals=rep_a(S["goals_self_rep"]),
             cf_eye=torch.eye(l_action, dtype=torch.float64, device=vec.device).repeat(S["s_n_rep"].shape[0], 1),
             cf_s_m=rep_a(S["s_m_rep"]), cf_s_others=rep_a(S["s_others_rep"]), cf_env=rep_a(S["env_rep"]), cf_ot=rep_a(S["ot_rep"]),
             cf_ov=rep_a(S["ov_rep"]))
    return S


def mode_static(dev):
    import torch
    from cm3_amd import _lib
    from cm3_amd import batch as BR
    M, B, calls = 24, 128, 20
    ro = _rollout(dev, 512, 33)
    cols = ro.sample_batch(M * B, generator=torch.Generator(device=dev).manual_seed(0), numpy=False)
    S = BR.checkers_static_feeds_device(cols)
    want = _static_composition(cols)
    assert sorted(S) == sorted(want) and all(torch.equal(S[k], want[k]) for k in S)
    paths = {"tiling_fresh": lambda: BR.checkers_static_feeds_device(cols), "tiling_into_out": lambda: BR.checkers_static_feeds_device(cols, out=S),
             "composition": lambda: _static_composition(cols)}
    for fn in paths.values():
        _wall(fn, 5, dev)
    times = {k: [] for k in paths}
    for _ in range(REPS):
        for k, fn in paths.items():
            times[k].append(_wall(fn, calls, dev))
    # ... and the three launches alone: event time over a captured graph of 20 sets
    def enqueue(stream):
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)):
            for _ in range(20):
                BR.checkers_static_feeds_device(cols, out=S)
    graph = _lib.capture_graph(dev, enqueue)
    dev_times = []
    for _ in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(_lib.lib().cm3_graph_launch(graph, torch.cuda.current_stream(dev).cuda_stream))
        b.record()
        b.synchronize()
        dev_times.append(a.elapsed_time(b) * 1e3 / 20)
    _lib.lib().cm3_graph_destroy(graph)
    ro.close()
    out = {"mode": "static", "transitions": M * B, "agents": 2, "bytes_written": sum(t.numel() * t.element_size() for t in S.values()),
           "device_us_per_set": _stats(dev_times[1:])}
    out.update({k + "_us": _stats(v) for k, v in times.items()})
    return out


def mode_phase(dev):
    import numpy as np
    import torch
    from cm3_amd import batch as BR
    M, B, N = 24, 128, 2
    ro = _rollout(dev, 8192, 330)
    run = _answers(B, N, dev)
    gen = torch.Generator(device=dev).manual_seed(1)

    def eager():
        ro.collect()
        for cols in ro.on_policy_minibatches(M, B, gen):
            BR.train_step_feeds(cols, run, 0.99, 0.3, env="checkers")

    paths = {"eager": eager}
    plan = None
    if hasattr(BR, "checkers_static_feeds_device"):
        plan = BR.OnPolicyPhasePlan(ro, run, 0.99, 0.3, epochs=M, batch_size=B)

        def planned():
            ro.collect()
            plan.refresh(gen)
            for k in range(M):
                plan.step(k)
        paths["plan"] = planned

        def feeds_only():
            plan.refresh(gen)
            for k in range(M):
                plan.step(k)
        paths["plan_without_collect"] = feeds_only

    def eager_feeds_only():
        for cols in ro.on_policy_minibatches(M, B, gen):
            BR.train_step_feeds(cols, run, 0.99, 0.3, env="checkers")
    paths["eager_without_collect"] = eager_feeds_only
    paths["collect_only"] = lambda: ro.collect()
    for fn in paths.values():
        _wall(fn, 2, dev)
    times = {k: [] for k in paths}
    for _ in range(REPS):
        for k, fn in paths.items():
            times[k].append(_wall(fn, 1, dev) / 1e3)
    if plan is not None:
        plan.close()
    ro.close()
    out = {"mode": "phase", "envs": 8192, "ticks": 330, "minibatches": M, "transitions": B, "unit": "ms per phase"}
    out.update({k + "_ms": _stats(v) for k, v in times.items()})
    return out


def mode_rows(dev):
    import torch
    from cm3_amd import _lib
    from cm3_amd.batch import _Tiler
    src_rows, rep, launches = 6144, 10, 50
    out = {"mode": "rows", "dst_rows": src_rows * rep, "launches_per_graph": launches, "lib": os.environ.get("CM3_AMD_LIB") or "product"}
    graphs, keep = {}, []
    for rb in ROW_SIZES:
        src = torch.rand(src_rows, rb // 8, dtype=torch.float64, device=dev)
        dst = torch.empty(src_rows * rep, rb // 8, dtype=torch.float64, device=dev)
        keep.append((src, dst))

        def enqueue(stream, src=src, dst=dst):
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)):
                for _ in range(launches):
                    t = _Tiler(dev)
                    t.add(src, dst.shape[0], src.shape[1], src.dtype, _lib.TILE_COPY, terms=((rep, 0, 1), (1, 0, 0)), out=dst)
                    t.run()
        graphs[rb] = _lib.capture_graph(dev, enqueue)
        t = _Tiler(dev)
        got = t.add(src, dst.shape[0], src.shape[1], src.dtype, _lib.TILE_COPY, terms=((rep, 0, 1), (1, 0, 0)))
        t.run()
        assert torch.equal(got, src.repeat_interleave(rep, dim=0))
    s = torch.cuda.current_stream(dev).cuda_stream
    times = {rb: [] for rb in ROW_SIZES}
    for r in range(REPS + 1):
        for rb, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(_lib.lib().cm3_graph_launch(g, s))
            b.record()
            b.synchronize()
            if r:
                times[rb].append(a.elapsed_time(b) * 1e3 / launches)
    for g in graphs.values():
        _lib.lib().cm3_graph_destroy(g)
    out["us_per_launch"] = {str(rb): _stats(v) for rb, v in times.items()}
    return out


def main():
    import torch
    args = sys.argv[1:]
    tag = None
    if "--tag" in args:
        k = args.index("--tag")
        tag = args[k + 1]
        del args[k:k + 2]
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    modes = {"feeds": mode_feeds, "static": mode_static, "phase": mode_phase, "rows": mode_rows}
    for m in args or list(modes):
        res = modes[m](dev)
        if tag:
            res["tag"] = tag
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
