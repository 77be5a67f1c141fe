#!/usr/bin/env python
"""Timing of the particle QMIX learner (profiles/r31_qmix_learner.txt), one JSON line per mode.

  launches  the learner's launches at 128 x 4 and 16 384 x 4 transitions x agents, each group inside a captured graph of 50 repeats,
            alternating in one process; us per group, event timing: "grad" = the five launches of
            cm3_qmix_learner_particle_grad_f32 (k_learner_agent_fwd, k_learner_mixer, k_learner_agent_bwd, k_learner_xtd,
            k_qmix_learner_reduce), "adam" = k_adam_step over the eleven tensors, "repack" = the two pack launches.  The split of
            "grad" by kernel comes from running this mode under a kernel trace.
  step      one ParticleQmixLearner.step and one train_step at 128 x 4 and 128 x 8, as host time per call (synchronised at the end
            of 50 calls) and as device time (a captured graph of the call, replayed), against a torch composition of the same step:
            the same weights as leaf tensors, autograd on the device, and tf.train.AdamOptimizer's formula written in torch -- what a
            user had to write before.  No time is a pass criterion.

    python tools/qmix_learner_timing.py [launches] [step] [--out FILE]     (default: both modes, FILE = profiles/r31_qmix_learner.txt)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from qmix_mixer_timing import _agent_weights, _cols, _mixer_weights, _stats      # noqa: E402

REPS, REPEATS_PER_GRAPH, INNER, CALLS = 7, 50, 4, 50


def _time_graph(graph, dev, per_graph):
    import torch
    from cm3_amd import _lib
    s = torch.cuda.current_stream(dev).cuda_stream
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        _lib.check(_lib.lib().cm3_graph_launch(graph, s))
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / (INNER * per_graph)


def _nets(N, rng, dev, max_batch):
    from cm3_amd.qmix import ParticleQmixAgent, ParticleQmixLearner, ParticleQmixMixer
    agent = ParticleQmixAgent(_agent_weights(N, rng), N, device=dev)
    mixer = ParticleQmixMixer(_mixer_weights(N, rng), N, device=dev)
    return agent, mixer, ParticleQmixLearner(agent, mixer, max_batch=max_batch)


def _capture(dev, body, repeats):
    import torch
    from cm3_amd import _lib

    def enqueue(stream):
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)):
            for _ in range(repeats):
                body()
    return _lib.capture_graph(dev, enqueue)


def _alternate(graphs, dev):
    import torch
    from cm3_amd import _lib
    for g, n in graphs.values():
        _time_graph(g, dev, n)
    times = {k: [] for k in graphs}
    for _ in range(REPS):
        for k, (g, n) in graphs.items():
            times[k].append(_time_graph(g, dev, n))
    torch.cuda.synchronize()
    for g, _ in graphs.values():
        _lib.lib().cm3_graph_destroy(g)
    return times


def mode_launches(dev):
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    N, graphs, hold = 4, {}, []
    for B in (128, 16384):
        agent, mixer, learner = _nets(N, rng, dev, B)
        c = _cols(B, N, rng, dev)
        td = torch.as_tensor(rng.standard_normal(B), device=dev)
        keep = []
        staged = learner._stage(c, td, keep)
        loss, q_tot = torch.empty(1, device=dev), torch.empty(B, device=dev)
        hold.append((agent, mixer, learner, c, td, keep, loss, q_tot))
        graphs["grad_%d" % B] = (_capture(dev, lambda l=learner, s=staged, a=loss, b=q_tot: l.enqueue_gradients(*s, a, b), REPEATS_PER_GRAPH),
                                 REPEATS_PER_GRAPH)
        graphs["adam_%d" % B] = (_capture(dev, learner.enqueue_adam, REPEATS_PER_GRAPH), REPEATS_PER_GRAPH)
        graphs["repack_%d" % B] = (_capture(dev, lambda a=agent, m=mixer: (a.repack(), m.repack()), REPEATS_PER_GRAPH), REPEATS_PER_GRAPH)
    times = _alternate(graphs, dev)
    return {"mode": "launches", "agents": N, "repeats_per_graph": REPEATS_PER_GRAPH, "replays": INNER, "repeats": REPS,
            **{k + "_us": _stats(v) for k, v in times.items()}}


def _torch_learner(agent, mixer, N, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """the same step in torch: autograd on leaf copies of the weights, TF-form Adam with the powers on the device"""
    import torch
    w = {k: v.clone().requires_grad_(True) for k, v in list(agent.w.items()) + list(mixer.w.items())}
    m = {k: torch.zeros_like(v) for k, v in w.items()}
    v2 = {k: torch.zeros_like(v) for k, v in w.items()}
    powers = torch.tensor([b1, b2], device=agent.device)

    def step(cols, td):
        B = cols["v_global"].shape[0]
        x = torch.cat([cols["obs_others"].reshape(B * N, -1), cols["v_local"].reshape(B * N, 4), cols["goals"].reshape(B * N, 2)], dim=1)
        h = torch.relu(torch.relu(x @ w["h/kernel"] + w["h/bias"]) @ w["h2/kernel"] + w["h2/bias"])
        q = (h @ w["out/kernel"] + w["out/bias"]).gather(1, cols["actions"].reshape(-1, 1)).reshape(B, 1, N)
        xm = torch.cat([cols["v_global"].reshape(B, -1), cols["goals"].reshape(B, -1)], dim=1)
        b_final = torch.relu(xm @ w["b_final_l1"]) @ w["b_final"]
        hidden = torch.nn.functional.elu(q @ torch.abs(xm @ w["w1"]).reshape(B, N, 64) + (xm @ w["b1"]).reshape(B, 1, 64))
        q_tot = (hidden @ torch.abs(xm @ w["w_final"]).reshape(B, 64, 1) + b_final.reshape(B, 1, 1)).reshape(B)
        loss = torch.mean((td.float() - q_tot) ** 2)
        grads = torch.autograd.grad(loss, list(w.values()))
        with torch.no_grad():
            lr_t = lr * torch.sqrt(1 - powers[1]) / (1 - powers[0])
            for (k, p), g in zip(w.items(), grads):
                m[k].mul_(b1).add_(g, alpha=1 - b1)
                v2[k].mul_(b2).addcmul_(g, g, value=1 - b2)
                p.sub_(lr_t * m[k] / (v2[k].sqrt() + eps))
            powers.mul_(torch.tensor([b1, b2], device=powers.device))
        return loss
    return step


def mode_step(dev):
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    B, gamma, tau = 128, 0.99, 0.01
    out = {"mode": "step", "transitions": B, "calls_per_repeat": CALLS, "repeats": REPS, "repeats_per_graph": 10}
    for N in (4, 8):
        agent, mixer, learner = _nets(N, rng, dev, B)
        t_agent, t_mixer, _ = _nets(N, rng, dev, B)
        c = _cols(B, N, rng, dev)
        td = torch.as_tensor(rng.standard_normal(B), device=dev)
        torch_step = _torch_learner(agent, mixer, N)
        paths = {"step": lambda: learner.step(c, td), "train_step": lambda: learner.train_step(c, gamma, t_agent, t_mixer, tau),
                 "torch_autograd_adam": lambda: torch_step(c, td)}
        for fn in paths.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        host = {k: [] for k in paths}
        for _ in range(REPS):
            for k, fn in paths.items():
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    fn()
                torch.cuda.synchronize()
                host[k].append((time.perf_counter() - t0) * 1e6 / CALLS)
        # device time: the learner's calls replayed from a graph; the torch composition between two events (it is not captured)
        keep = []
        graphs = {"step": (_capture(dev, lambda: learner.step(c, td, keep=keep), 10), 10),
                  "train_step": (_capture(dev, lambda: learner.train_step(c, gamma, t_agent, t_mixer, tau, keep=keep), 10), 10)}
        device = _alternate(graphs, dev)
        device["torch_autograd_adam"] = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                torch_step(c, td)
            b.record()
            b.synchronize()
            device["torch_autograd_adam"].append(a.elapsed_time(b) * 1e3 / CALLS)
        for k in paths:
            out["n%d_%s_host_us" % (N, k)] = _stats(host[k])
            out["n%d_%s_device_us" % (N, k)] = _stats(device[k])
    return out


def main():
    import torch
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "r31_qmix_learner.txt")
    if "--out" in args:
        k = args.index("--out")
        out = args[k + 1]
        del args[k:k + 2]
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    modes = {"launches": mode_launches, "step": mode_step}
    lines = []
    for m in args or ["launches", "step"]:
        lines.append(json.dumps(modes[m](dev)))
        print(lines[-1], flush=True)
    with open(out, "w") as fh:
        fh.write("# tools/qmix_learner_timing.py on %s; us, min / median / max over %d repeats\n" % (torch.cuda.get_device_name(dev), REPS))
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
