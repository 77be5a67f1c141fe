"""TEST INFRASTRUCTURE ONLY -- restatement of the particle QMIX mixer in a chosen dtype (the mixer's counterpart of tests/critic_ref.py;
test helper, not a test module).

  networks.Qmix_mixer   alg/networks.py:640-685, x = concat(state [4N], goals_all [2N])
      l1      = relu(x . hyper_b_final_l1/kernel)           b_final = l1 . hyper_b_final/kernel         (no biases)
      w1      = |x . hyper_w_1| viewed [N][64]              b1      = x . hyper_b_1
      hidden  = elu(agent_qs . w1 + b1)                     w_final = |x . hyper_w_final|
      q_tot   = hidden . w_final + b_final

order="matmul" writes every contraction as the NumPy matmul the oracle shim evaluates (in float32 the fixture's own operations);
order="kernel" writes the sums after the hyper-network in the order of csrc/mixer.hip: the sum over agents a chain in ascending n
started by the product for n = 0 with b1 added last; hidden * |w_final| and l1 * hyper_b_final summed SEPARATELY over the 64
embedding units, each as a pairwise tree inside every 16 units (pairs, fours, eights, sixteen), then the four sixteens left to right;
q_tot = the first sum + the second.  (The hyper-network itself is a k-ordered chain per output on the device, a matmul here.)
"""
import numpy as np

NAMES = ("hyper_w_1", "hyper_w_final", "hyper_b_1", "hyper_b_final_l1/kernel", "hyper_b_final/kernel")
PREFIXES = ("Mixer_main/", "Mixer_target/")
EMBED = 64


def canon(name):
    name = name.split(":")[0]
    for prefix in PREFIXES:
        if name.startswith(prefix):
            name = name[len(prefix):]
    return name


def shapes(n_agents):
    k = 6 * n_agents
    return {"hyper_w_1": (k, EMBED * n_agents), "hyper_w_final": (k, EMBED), "hyper_b_1": (k, EMBED),
            "hyper_b_final_l1/kernel": (k, EMBED), "hyper_b_final/kernel": (EMBED, 1)}


def init_weights(rng, n_agents, scale=0.5, scope=None):
    """Random float32 weights under the reference's variable names, scaled by scale / sqrt(fan_in), in the order the reference
    creates them.  scope: e.g. "Mixer_target" prefixes the names."""
    f = lambda shape: (rng.standard_normal(shape) * scale / np.sqrt(shape[0])).astype(np.float32)  # noqa: E731
    w = {name: f(shape) for name, shape in shapes(n_agents).items()}
    return w if scope is None else {scope + "/" + k: v for k, v in w.items()}


def _sum64(v):
    """[rows, 64] -> [rows]: the device's tree over the embedding units"""
    s = v.reshape(v.shape[0], 4, 8, 2)
    s = s[..., 0] + s[..., 1]                      # pairs                 [rows, 4, 8]
    s = s.reshape(v.shape[0], 4, 4, 2)
    s = s[..., 0] + s[..., 1]                      # fours                 [rows, 4, 4]
    s = s.reshape(v.shape[0], 4, 2, 2)
    s = s[..., 0] + s[..., 1]                      # eights                [rows, 4, 2]
    s = s[..., 0] + s[..., 1]                      # sixteens              [rows, 4]
    return ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]


def q_tot(w, agent_qs, state, goals_all, dtype=np.float64, order="matmul"):
    """q_tot [rows, 1] of Qmix_mixer from agent_qs [rows, N], state [rows, 4N] (or [rows, N, 4]) and goals_all [rows, 2N] (or
    [rows, N, 2])."""
    w = {canon(k): v for k, v in w.items()}
    f = np.dtype(dtype).type
    W = lambda k: np.asarray(w[k], dtype=f)  # noqa: E731
    q = np.asarray(agent_qs, dtype=f)
    rows, n = q.shape
    x = np.concatenate([np.asarray(state).reshape(rows, -1), np.asarray(goals_all).reshape(rows, -1)], axis=1).astype(f)
    l1 = np.maximum(x @ W("hyper_b_final_l1/kernel"), f(0))
    w1 = np.abs(x @ W("hyper_w_1")).reshape(rows, n, EMBED)
    b1 = x @ W("hyper_b_1")
    w_final = np.abs(x @ W("hyper_w_final"))
    elu = lambda h: np.where(h > 0, h, np.expm1(np.minimum(h, f(0))))  # noqa: E731
    if order == "matmul":
        b_final = l1 @ W("hyper_b_final/kernel")
        hidden = elu(q.reshape(rows, 1, n) @ w1 + b1.reshape(rows, 1, EMBED))
        y = hidden @ w_final.reshape(rows, EMBED, 1) + b_final.reshape(rows, 1, 1)
        return y.reshape(rows, 1)
    assert order == "kernel", order
    t = q[:, 0:1] * w1[:, 0]
    for k in range(1, n):
        t = t + q[:, k:k + 1] * w1[:, k]
    hidden = elu(t + b1)
    y = _sum64(hidden * w_final) + _sum64(l1 * W("hyper_b_final/kernel").reshape(1, EMBED))
    return y.reshape(rows, 1).astype(f)


def torch_mixer(w, agent_qs, state, goals_all):
    """The network in torch float32 on the tensors' device, from the short-named TF-shaped tensors of a ParticleQmixMixer (mixer.w):
    what plays sess.run(mixer_target) inside `run`.  Any dtype in (a tf.float32 placeholder rounds its feed); float32 [rows, 1] out."""
    import torch
    f32 = lambda t: t.to(torch.float32)  # noqa: E731
    q = f32(agent_qs)
    rows, n = q.shape
    x = torch.cat([f32(state).reshape(rows, -1), f32(goals_all).reshape(rows, -1)], dim=1)
    l1 = torch.relu(x @ w["b_final_l1"])
    b_final = l1 @ w["b_final"]
    w1 = torch.abs(x @ w["w1"]).reshape(rows, n, EMBED)
    b1 = (x @ w["b1"]).reshape(rows, 1, EMBED)
    hidden = torch.nn.functional.elu(q.reshape(rows, 1, n) @ w1 + b1)
    w_final = torch.abs(x @ w["w_final"]).reshape(rows, EMBED, 1)
    return (hidden @ w_final + b_final.reshape(rows, 1, 1)).reshape(rows, 1)
