#!/usr/bin/env python
"""Timing of the Checkers QMIX learner (profiles/r32_qmix_learner_checkers.txt), one JSON line: the sibling of
tools/qmix_learner_timing.py for cm3_amd.qmix.CheckersQmixLearner.

At 128 transitions (the batch size the Checkers stages train with, configs/rollout.json) of 2 agents, in one process:
  grad / adam / repack   the learner's launch groups, each inside a captured graph of 20 repeats, alternating; us per group, event
                         timing: "grad" = the fourteen launches of cm3_qmix_learner_checkers_grad_f32, "adam" = k_adam_step over the
                         twenty tensors, "repack" = the two pack launches
  step                   one CheckersQmixLearner.step as device time (a captured graph of the call, replayed) and as host time per call
                         (synchronised at the end of 50 calls)
  torch_autograd_adam    a torch composition of the same step on the same GPU -- the same weights as leaf tensors, conv2d / matmul
                         autograd in float32, tf.train.AdamOptimizer's formula written in torch -- between two events and as host time
No time is a pass criterion.  The shares of the error bound measured by tests/test_gpu_qmix_learner_checkers.py are kept in the same
file, below the timing line, by hand.

    python tools/qmix_learner_checkers_timing.py [--agents N] [--batch B] [--out FILE]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from qmix_learner_timing import CALLS, REPS, _alternate, _capture      # noqa: E402
from qmix_mixer_timing import _stats      # noqa: E402

REPEATS_PER_GRAPH = 20


def _weights(N, rng):
    """(Agent_main, Mixer_main) weights under the TF variable names, scaled by 1 / sqrt(fan-in)"""
    import numpy as np
    lo, k = 2 * max(N - 1, 1), 108 + 6 * N
    f = lambda fan, *s: (rng.standard_normal(s) / np.sqrt(fan)).astype(np.float32)      # noqa: E731
    agent = {"conv/Conv/weights": f(27, 3, 3, 3, 6), "conv/Conv/biases": f(4, 6), "conv_linear/kernel": f(150, 150, 32),
             "conv_linear/bias": f(4, 32), "branch_self/kernel": f(43, 43, 256), "branch_self/bias": f(4, 256), "W_self_h2": f(256, 256, 256),
             "branch_others/kernel": f(lo, lo, 256), "branch_others/bias": f(4, 256), "W_others_h2": f(256, 256, 256), "b": f(4, 256),
             "Qmix_single_out/kernel": f(16, 256, 5), "Qmix_single_out/bias": f(4, 5)}
    mixer = {"conv/Conv/weights": f(60, 3, 5, 2, 4), "conv/Conv/biases": f(16, 4), "hyper_w_1": f(4 * k, k, 128 * N),
             "hyper_w_final": f(4 * k, k, 128), "hyper_b_1": f(4 * k, k, 128), "hyper_b_final_l1/kernel": f(4 * k, k, 128),
             "hyper_b_final/kernel": f(512, 128, 1)}
    return agent, mixer


def _cols(B, N, rng, dev):
    """the columns a step reads, in the compact ring's forms: int8 windows and grids, uint8 index goals, float64 vectors"""
    import numpy as np
    import torch
    lo = 2 * max(N - 1, 1)
    t = lambda a: torch.as_tensor(a, device=dev)      # noqa: E731
    return {"obs_self_t": t(rng.integers(-1, 2, (B, N, 5, 5, 3)).astype(np.int8)), "obs_self_v": t(rng.uniform(-1, 1, (B, N, 4))),
            "obs_others": t(rng.uniform(-1, 1, (B, N, lo))), "actions_prev": t(rng.integers(0, 5, (B, N)).astype(np.int32)),
            "actions": t(rng.integers(0, 5, (B, N)).astype(np.int32)), "goals": t(rng.integers(0, 2, (B, N)).astype(np.uint8)),
            "grid": t(rng.integers(0, 2, (B, 3, 9, 2)).astype(np.int8)), "vec": t(rng.uniform(-2, 2, (B, N, 4)))}


def _torch_learner(agent, mixer, N, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """the same step in torch: autograd on leaf copies of the weights, TF-form Adam with the powers on the device"""
    import torch
    F = torch.nn.functional
    w = {"agent/" + k: v.clone().requires_grad_(True) for k, v in agent.w.items()}
    w.update({"mixer/" + k: v.clone().requires_grad_(True) for k, v in mixer.w.items()})
    m = {k: torch.zeros_like(v) for k, v in w.items()}
    v2 = {k: torch.zeros_like(v) for k, v in w.items()}
    powers = torch.tensor([b1, b2], device=agent.device)
    A = lambda k: w["agent/" + k]      # noqa: E731
    M = lambda k: w["mixer/" + k]      # noqa: E731

    def step(cols, td):
        B = cols["vec"].shape[0]
        R = B * N
        f32 = lambda t: t.to(torch.float32)      # noqa: E731
        win = f32(cols["obs_self_t"]).reshape(R, 5, 5, 3).permute(0, 3, 1, 2)
        c1 = torch.relu(F.conv2d(win, A("conv_w").permute(3, 2, 0, 1), A("conv_b"), padding=1)).permute(0, 2, 3, 1).reshape(R, 150)
        goal = F.one_hot(cols["goals"].long().reshape(R), 2).to(torch.float32)
        xs = torch.cat([torch.relu(c1 @ A("lin_w") + A("lin_b")), f32(cols["obs_self_v"]).reshape(R, 4),
                        F.one_hot(cols["actions_prev"].long().reshape(R), 5).to(torch.float32), goal], dim=1)
        hs = torch.relu(xs @ A("self_w") + A("self_b"))
        ho = torch.relu(f32(cols["obs_others"]).reshape(R, -1) @ A("others_w") + A("others_b"))
        h2 = torch.relu(hs @ A("w_self_h2") + ho @ A("w_others_h2") + A("b_h2"))
        q = (h2 @ A("out_w") + A("out_b")).gather(1, cols["actions"].long().reshape(-1, 1)).reshape(B, 1, N)
        grid = f32(cols["grid"]).permute(0, 3, 1, 2)
        cm = torch.relu(F.conv2d(grid, M("conv_w").permute(3, 2, 0, 1), M("conv_b"), padding=(1, 2))).permute(0, 2, 3, 1).reshape(B, 108)
        xm = torch.cat([cm, f32(cols["vec"]).reshape(B, -1), goal.reshape(B, -1)], dim=1)
        b_final = torch.relu(xm @ M("hyper_b_final_l1")) @ M("hyper_b_final")
        hidden = F.elu(q @ torch.abs(xm @ M("hyper_w_1")).reshape(B, N, 128) + (xm @ M("hyper_b_1")).reshape(B, 1, 128))
        q_tot = (hidden @ torch.abs(xm @ M("hyper_w_final")).reshape(B, 128, 1) + b_final.reshape(B, 1, 1)).reshape(B)
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


def measure(dev, N, B):
    import numpy as np
    import torch
    from cm3_amd.qmix import CheckersQmixAgent, CheckersQmixLearner, CheckersQmixMixer
    rng = np.random.default_rng(0)
    wa, wm = _weights(N, rng)
    agent, mixer = CheckersQmixAgent(wa, N, device=dev), CheckersQmixMixer(wm, N, device=dev)
    learner = CheckersQmixLearner(agent, mixer, max_batch=B)
    c = _cols(B, N, rng, dev)
    td = torch.as_tensor(rng.standard_normal(B), device=dev)
    torch_step = _torch_learner(agent, mixer, N)
    paths = {"step": lambda: learner.step(c, td), "torch_autograd_adam": lambda: torch_step(c, td)}
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
    keep = []
    staged = learner._stage(c, td, keep)
    loss, q_tot = torch.empty(1, device=dev), torch.empty(B, device=dev)
    graphs = {"grad": (_capture(dev, lambda: learner.enqueue_gradients(*staged, loss, q_tot), REPEATS_PER_GRAPH), REPEATS_PER_GRAPH),
              "adam": (_capture(dev, learner.enqueue_adam, REPEATS_PER_GRAPH), REPEATS_PER_GRAPH),
              "repack": (_capture(dev, lambda: (agent.repack(), mixer.repack()), REPEATS_PER_GRAPH), REPEATS_PER_GRAPH),
              "step": (_capture(dev, lambda: learner.step(c, td, keep=keep), 10), 10)}
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
    out = {"mode": "step", "env": "checkers", "agents": N, "transitions": B, "repeats": REPS, "calls_per_repeat": CALLS}
    out.update({k + "_device_us": _stats(v) for k, v in device.items()})
    out.update({k + "_host_us": _stats(v) for k, v in host.items()})
    return out


def main():
    import torch
    args = sys.argv[1:]
    opts = {"--agents": "2", "--batch": "128", "--out": os.path.join(ROOT, "profiles", "r32_qmix_learner_checkers.txt")}
    for name in list(opts):
        if name in args:
            k = args.index(name)
            opts[name] = args[k + 1]
            del args[k:k + 2]
    if args:
        raise SystemExit("usage: qmix_learner_checkers_timing.py [--agents N] [--batch B] [--out FILE]")
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    line = json.dumps(measure(dev, int(opts["--agents"]), int(opts["--batch"])))
    print(line, flush=True)
    with open(opts["--out"], "w") as fh:
        fh.write("# python tools/qmix_learner_checkers_timing.py %s on %s; us, min / median / max over %d repeats\n"
                 % (" ".join(sys.argv[1:]), torch.cuda.get_device_name(dev), REPS))
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
