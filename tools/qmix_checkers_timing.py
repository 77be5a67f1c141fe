#!/usr/bin/env python
"""us per tick of policy-driven Checkers collection with the QMIX agent (CheckersQmixAgent: an agent launch and a step launch per
tick inside one hipGraph) next to the CM3 Checkers actor in the same launch mode (CheckersActor, policy_mode="tick"), f32 and f16x3
each, and the two f16x3 policies once more as ONE launch per rollout (policy_mode="episode": qmix_f16x3_episode,
cm3_actor_f16x3_episode), in one process, at C3 (config_checkers_stage2: 8192 envs x 2 agents): 33-tick continuous rollouts with
full trajectory storage, epsilon 0.1, random weights of the reference's shapes.  Timed with events over collect() calls (graph
replays, or the one launch), alternating the six policies over several repeats; prints one JSON line.
--agent-only [f32|f16x3]: launch only the QMIX agent at C3, 200 times (for rocprofv3 --kernel-trace --stats)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E, N, T = 8192, 2, 33


def _policies(dev, only=None):
    import numpy as np
    from cm3_amd.actor import CheckersActor
    from cm3_amd.qmix import CheckersQmixAgent
    from oracle import actor_checkers_oracle as AO
    from tests import qmix_checkers_ref as QC
    w_actor = AO.init_weights(np.random.default_rng(0), N, stage=2)
    w_qmix = QC.init_weights(np.random.default_rng(1), N)
    out = {}                                           # name -> (policy, policy_mode)
    for prec in ("f32", "f16x3"):
        if only is None:
            out["cm3_actor_%s_tick" % prec] = (CheckersActor(w_actor, N, stage=2, device=dev, precision=prec), "tick")
        if only in (None, prec):
            out["qmix_%s" % prec] = (CheckersQmixAgent(w_qmix, N, device=dev, precision=prec), "tick")
    if only is None:
        out["qmix_f16x3_episode"] = (out["qmix_f16x3"][0], "episode")
        out["cm3_actor_f16x3_episode"] = (out["cm3_actor_f16x3_tick"][0], "episode")
    return out


def _env(dev, auto_reset):
    import cm3_amd
    from cm3_amd.checkers import VecCheckersEnv
    cfg = cm3_amd.load_config("checkers_stage2")
    return VecCheckersEnv(cfg["init"], N, 33, E, device=dev, auto_reset=auto_reset)


def main():
    import numpy as np
    import torch
    from cm3_amd.rollout import CheckersRollout
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    if len(sys.argv) > 1 and sys.argv[1] == "--agent-only":
        prec = sys.argv[2] if len(sys.argv) > 2 else "f16x3"
        env = _env(dev, False)
        env.reset(np.eye(2))
        agent = _policies(dev, only=prec)["qmix_%s" % prec][0]
        for _ in range(200):
            agent.act(env, 0.1)
        torch.cuda.synchronize()
        print(json.dumps({"agent_only": "c3", "precision": prec, "launches": 200}))
        return
    reps, inner = 5, 20
    pols = _policies(dev)
    ros = {}
    for name, (pol, mode) in pols.items():
        ros[name] = CheckersRollout(_env(dev, True), n_ticks=T, use_graph=True, policy_mode=mode)
        for _ in range(3):
            ros[name].collect(np.eye(2), policy=pol, epsilon=0.1)
    torch.cuda.synchronize()
    times = {name: [] for name in pols}
    for _ in range(reps):
        for name, (pol, _) in pols.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                ros[name].collect(policy=pol, epsilon=0.1)
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / (inner * T))
    out = {"c3": {"envs": E, "agents": N, "ticks": T,
                  **{name + "_us_per_tick_median": sorted(v)[len(v) // 2] for name, v in times.items()},
                  **{name + "_us_per_tick_all": [round(x, 3) for x in v] for name, v in times.items()}}}
    for ro in ros.values():
        ro.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
