#!/usr/bin/env python
"""us per tick of policy-driven particle collection at the agent counts whose 16-row wave tiles are padded (3, 5, 6, 7, 9, 10), as ONE
launch per rollout (ParticleRollout(..., partial_tiles=True, policy_mode="episode"): k_policy_rollout) and as launch pairs (an actor
launch and a step launch per tick inside one hipGraph, policy_mode="tick"), in one process:
    4096 float32 envs of particle_ring10 per agent count, CM3 actor at f16x3, random weights of the reference's shapes
33-tick continuous (auto-reset) rollouts with full trajectory storage, epsilon 0.1, no env reset between collects.  After 3 warm-up
collects per arm the arms alternate over ROUNDS rounds; a round is INNER collects, each between two events, and counts as the sum of
its collects over INNER * 33 ticks.  At ten agents the one launch is also timed with the row tiles per workgroup forced to 1, 2 and 4
(cm3_policy_force_row_tiles).  Prints a table -- median (min - max) and every round per arm -- then one JSON line.
Usage: policy_partial_tiles_timing.py [--envs E] [--rt-sweep] [n_agents ...]     (--rt-sweep: the forced row tiles at every agent count)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AGENTS = (3, 5, 6, 7, 9, 10)
T, ROUNDS, INNER, SEED = 33, 7, 20, 12341


def _actor(N, dev):
    import numpy as np
    from cm3_amd.actor import ParticleActor
    rng = np.random.default_rng(0)
    L = 4 * (N - 1)
    f = lambda *s: (rng.standard_normal(s) * 0.1).astype(np.float32)  # noqa: E731
    return ParticleActor({"actor_branch_self/kernel": f(6, 64), "actor_branch_self/bias": f(64), "W_branch_self_h2": f(64, 64),
                          "stage-2/actor_others/kernel": f(L, 128), "stage-2/actor_others/bias": f(128),
                          "stage-2/W_others_h2": f(128, 64), "b": f(64), "actor_out/kernel": f(64, 5), "actor_out/bias": f(5)},
                         N, stage=2, device=dev, seed=SEED, precision="f16x3")


def main():
    import torch
    import cm3_amd
    from cm3_amd import _lib
    from cm3_amd.particle import VecParticleEnv
    from cm3_amd.rollout import ParticleRollout
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    force = lambda rt: _lib.check(_lib.lib().cm3_policy_force_row_tiles(rt))  # noqa: E731
    out = {}
    args = sys.argv[1:]
    E = int(args.pop(args.index("--envs") + 1)) if "--envs" in args else 4096
    sweep_all = "--rt-sweep" in args
    args = [a for a in args if not a.startswith("--")]
    for N in [int(a) for a in args] or AGENTS:
        actor = _actor(N, dev)
        # name -> (ParticleRollout keywords, forced row tiles; 0 = the launcher's rule)
        arms = {"pairs": (dict(policy_mode="tick"), 0), "one_launch": (dict(policy_mode="episode", partial_tiles=True), 0)}
        if N == 10 or sweep_all:
            for rt in (1, 2, 4):
                arms["one_launch_rt%d" % rt] = (dict(policy_mode="episode", partial_tiles=True), rt)
        ros, kernels = {}, {}
        for name, (kw, rt) in arms.items():
            env = VecParticleEnv(cm3_amd.load_config("particle_ring10"), N, 0.2, 33, E, device=dev, seed=SEED, auto_reset=True)
            env.reset()
            ros[name] = ParticleRollout(env, n_ticks=T, use_graph=True, **kw)
            force(rt)
            for _ in range(3):
                ros[name].collect(policy=actor, epsilon=0.1, reset=False)
            kernels[name] = _lib.last_kernel_variant()
        torch.cuda.synchronize()
        rounds = {name: [] for name in arms}
        for _ in range(ROUNDS):
            for name, (_, rt) in arms.items():
                force(rt)
                events = []
                for _ in range(INNER):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    ros[name].collect(policy=actor, epsilon=0.1, reset=False)
                    b.record()
                    events.append((a, b))
                events[-1][1].synchronize()
                rounds[name].append(sum(a.elapsed_time(b) for a, b in events) * 1e3 / (INNER * T))
        force(0)
        out[N] = {"envs": E, "agents": N, "ticks": T, "collects_per_round": INNER, "kernels": kernels}
        print("%d envs x %d agents (particle_ring10), %d collects per round" % (E, N, INNER))
        for name, v in rounds.items():
            s = sorted(v)
            out[N][name] = {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3),
                            "rounds": [round(x, 3) for x in v]}
            print("  %-16s median %7.3f   min %7.3f   max %7.3f   (%s)   %s" % (
                name, s[len(s) // 2], s[0], s[-1], " ".join("%.3f" % x for x in v), kernels[name]))
        # the criterion of profiles/r18_qmix_particle_episode.txt: the one launch's slowest round against the pairs' fastest round
        out[N]["one_launch_wins"] = out[N]["one_launch"]["max"] < out[N]["pairs"]["min"]
        print("  one launch's slowest round %s the pairs' fastest round" % ("beats" if out[N]["one_launch_wins"] else "DOES NOT beat"))
        sys.stdout.flush()
        for ro in ros.values():
            ro.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
