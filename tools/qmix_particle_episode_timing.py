#!/usr/bin/env python
"""us per tick of particle collection driven by the QMIX agent as launch pairs (an agent launch and a step launch per tick inside one
hipGraph, policy_mode="tick") and as ONE launch per rollout (ParticleQmixAgent(..., episode_kernel=True), policy_mode="episode":
k_policy_rollout_qmix), next to the CM3 actor's one-launch rollout at f16x3 (k_policy_rollout), in one process, on float32 envs:
    c2   4096 envs x 4 agents (particle_stage2_antipodal)      c5   8192 envs x 8 agents (particle_merge8)
    big  65536 envs x 4 agents (particle_stage2_antipodal)
33-tick continuous (auto-reset) rollouts with full trajectory storage, epsilon 0.1, random weights of the reference's shapes, no env
reset between collects.  After 3 warm-up collects per arm the three arms alternate over ROUNDS rounds; a round is INNER collects, each
between two events, and counts as the sum of its collects over INNER * 33 ticks.  Prints one JSON line: median, min and max of the
rounds per arm and size, and every round."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {"c2": ("particle_stage2_antipodal", 4096, 4, 20), "c5": ("particle_merge8", 8192, 8, 20),
             "big": ("particle_stage2_antipodal", 65536, 4, 5)}
T, ROUNDS, SEED = 33, 7, 12341


def _arms(N, dev):
    """name -> (policy, policy_mode)"""
    import numpy as np
    from cm3_amd.actor import ParticleActor
    from cm3_amd.qmix import ParticleQmixAgent
    rng = np.random.default_rng(0)
    L = 4 * max(N - 1, 1)
    f = lambda *s: (rng.standard_normal(s) * 0.1).astype(np.float32)  # noqa: E731
    actor = ParticleActor({"actor_branch_self/kernel": f(6, 64), "actor_branch_self/bias": f(64), "W_branch_self_h2": f(64, 64),
                           "stage-2/actor_others/kernel": f(L, 128), "stage-2/actor_others/bias": f(128),
                           "stage-2/W_others_h2": f(128, 64), "b": f(64), "actor_out/kernel": f(64, 5), "actor_out/bias": f(5)},
                          N, stage=2, device=dev, seed=SEED, precision="f16x3")
    qmix = ParticleQmixAgent({"Agent_main/h/kernel": f(L + 6, 64), "Agent_main/h/bias": f(64), "Agent_main/h2/kernel": f(64, 64),
                              "Agent_main/h2/bias": f(64), "Agent_main/out/kernel": f(64, 5), "Agent_main/out/bias": f(5)},
                             N, device=dev, seed=SEED, episode_kernel=True)
    return {"qmix_pairs": (qmix, "tick"), "qmix_episode": (qmix, "episode"), "cm3_actor_f16x3_episode": (actor, "episode")}


def main():
    import torch
    import cm3_amd
    from cm3_amd import _lib
    from cm3_amd.particle import VecParticleEnv
    from cm3_amd.rollout import ParticleRollout
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    only = sys.argv[1:] or list(WORKLOADS)
    out = {}
    for wl in only:
        cfg, E, N, inner = WORKLOADS[wl]
        arms = _arms(N, dev)
        ros, kernels = {}, {}
        for name, (pol, mode) in arms.items():
            env = VecParticleEnv(cm3_amd.load_config(cfg), N, 0.2, 33, E, device=dev, seed=SEED, auto_reset=True)
            env.reset()
            ros[name] = ParticleRollout(env, n_ticks=T, use_graph=True, policy_mode=mode)
            for _ in range(3):
                ros[name].collect(policy=pol, epsilon=0.1, reset=False)
            kernels[name] = _lib.last_kernel_variant()
        torch.cuda.synchronize()
        rounds = {name: [] for name in arms}
        for _ in range(ROUNDS):
            for name, (pol, _) in arms.items():
                events = []
                for _ in range(inner):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    ros[name].collect(policy=pol, epsilon=0.1, reset=False)
                    b.record()
                    events.append((a, b))
                events[-1][1].synchronize()
                rounds[name].append(sum(a.elapsed_time(b) for a, b in events) * 1e3 / (inner * T))
        out[wl] = {"envs": E, "agents": N, "ticks": T, "collects_per_round": inner, "kernels": kernels}
        for name, v in rounds.items():
            s = sorted(v)
            out[wl][name] = {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3),
                             "rounds": [round(x, 3) for x in v]}
        for ro in ros.values():
            ro.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
