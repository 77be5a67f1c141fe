#!/usr/bin/env python
"""us per tick of policy-driven collection with the QMIX agent (ParticleQmixAgent: an agent launch and a step launch per tick
inside one hipGraph) next to the CM3 actor in the same launch mode (ParticleActor(precision="f32"), policy_mode="tick"), in one
process, at C2 (4096 envs x 4 agents, particle_stage2_antipodal) and C5 (8192 envs x 8 agents, particle_merge8): 33-tick
continuous rollouts with full trajectory storage, epsilon 0.1, random weights of the reference's shapes.  Timed with events over
graph replays (collect() replays the captured graph), alternating the two policies over several repeats; prints one JSON line.
--agent-only W: launch only the QMIX agent at workload W, 200 times (for rocprofv3 --kernel-trace --stats)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {"c2": ("particle_stage2_antipodal", 4096, 4), "c5": ("particle_merge8", 8192, 8)}


def _policies(N, dev):
    import numpy as np
    from cm3_amd.actor import ParticleActor
    from cm3_amd.qmix import ParticleQmixAgent
    rng = np.random.default_rng(0)
    L = 4 * max(N - 1, 1)
    f = lambda *s: (rng.standard_normal(s) * 0.1).astype(np.float32)  # noqa: E731
    actor = ParticleActor({"actor_branch_self/kernel": f(6, 64), "actor_branch_self/bias": f(64), "W_branch_self_h2": f(64, 64),
                           "stage-2/actor_others/kernel": f(L, 128), "stage-2/actor_others/bias": f(128),
                           "stage-2/W_others_h2": f(128, 64), "b": f(64), "actor_out/kernel": f(64, 5), "actor_out/bias": f(5)},
                          N, stage=2, device=dev, precision="f32")
    qmix = ParticleQmixAgent({"Agent_main/h/kernel": f(L + 6, 64), "Agent_main/h/bias": f(64), "Agent_main/h2/kernel": f(64, 64),
                              "Agent_main/h2/bias": f(64), "Agent_main/out/kernel": f(64, 5), "Agent_main/out/bias": f(5)},
                             N, device=dev)
    return {"cm3_actor_f32_tick": actor, "qmix": qmix}


def main():
    import torch
    import cm3_amd
    from cm3_amd.particle import VecParticleEnv
    from cm3_amd.rollout import ParticleRollout
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    if len(sys.argv) > 2 and sys.argv[1] == "--agent-only":
        cfg, E, N = WORKLOADS[sys.argv[2]]
        env = VecParticleEnv(cm3_amd.load_config(cfg), N, 0.2, 33, E, device=dev)
        env.reset()
        agent = _policies(N, dev)["qmix"]
        for _ in range(200):
            agent.act(env, 0.1)
        torch.cuda.synchronize()
        print(json.dumps({"agent_only": sys.argv[2], "launches": 200}))
        return
    T, reps, inner = 33, 5, 20
    out = {}
    for wl, (cfg, E, N) in WORKLOADS.items():
        pols = _policies(N, dev)
        ros = {}
        for name, pol in pols.items():
            env = VecParticleEnv(cm3_amd.load_config(cfg), N, 0.2, 33, E, device=dev, auto_reset=True)
            env.reset()
            ros[name] = ParticleRollout(env, n_ticks=T, use_graph=True, policy_mode="tick")
            for _ in range(3):
                ros[name].collect(policy=pol, epsilon=0.1, reset=False)
        torch.cuda.synchronize()
        times = {name: [] for name in pols}
        for _ in range(reps):
            for name, pol in pols.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(inner):
                    ros[name].collect(policy=pol, epsilon=0.1, reset=False)
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b) * 1e3 / (inner * T))
        out[wl] = {"envs": E, "agents": N, "ticks": T,
                   **{name + "_us_per_tick_median": sorted(v)[len(v) // 2] for name, v in times.items()},
                   **{name + "_us_per_tick_all": [round(x, 3) for x in v] for name, v in times.items()}}
        for ro in ros.values():
            ro.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
