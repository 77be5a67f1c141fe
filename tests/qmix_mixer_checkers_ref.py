"""TEST INFRASTRUCTURE ONLY -- restatement of the Checkers QMIX mixer in a chosen dtype (the Checkers counterpart of
tests/qmix_mixer_ref.py; test helper, not a test module).

  networks.Qmix_mixer_checkers   alg/networks.py:688-734 at Q_conv_f 4, Q_conv_k [3, 5] (config_checkers_stage{1,2}.json)
      conv    = relu(conv2d SAME [3][5][2][4] over state_env[3][9][2] + biases)  flattened NHWC -> 108   (networks.convnet_1 :67-75)
      x       = concat(conv [108], state [4N], goals_all [2N])
      l1      = relu(x . hyper_b_final_l1/kernel)           b_final = l1 . hyper_b_final/kernel         (no biases)
      w1      = |x . hyper_w_1| viewed [N][128]             b1      = x . hyper_b_1
      hidden  = elu(agent_qs . w1 + b1)                     w_final = |x . hyper_w_final|
      q_tot   = hidden . w_final + b_final

order="matmul" writes every contraction as the NumPy matmul the oracle shim evaluates; order="kernel" writes the sums after the
hyper-network in the order of csrc/mixer.hip (k_ck_qmix_mixer_rows): the sum over agents a chain in ascending n started by the product
for n = 0 with b1 added last; hidden * |w_final| and l1 * hyper_b_final summed SEPARATELY over the 128 embedding units, each as a
pairwise tree inside every 16 units (pairs, fours, eights, sixteen), then the eight sixteens left to right; q_tot = the first sum + the
second.  (The convolution and the hyper-network are one chain per output on the device, NumPy's conv_same / matmul here.)
"""
import numpy as np

from tests.critic_checkers_ref import conv_same

NAMES = ("conv/Conv/weights", "conv/Conv/biases", "hyper_w_1", "hyper_w_final", "hyper_b_1", "hyper_b_final_l1/kernel",
         "hyper_b_final/kernel")
PREFIXES = ("Mixer_main/", "Mixer_target/")
EMBED = 128
CONV_OUT = 108


def canon(name):
    name = name.split(":")[0]
    for prefix in PREFIXES:
        if name.startswith(prefix):
            name = name[len(prefix):]
    return name


def shapes(n_agents):
    k = CONV_OUT + 6 * n_agents
    return {"conv/Conv/weights": (3, 5, 2, 4), "conv/Conv/biases": (4,), "hyper_w_1": (k, EMBED * n_agents), "hyper_w_final": (k, EMBED),
            "hyper_b_1": (k, EMBED), "hyper_b_final_l1/kernel": (k, EMBED), "hyper_b_final/kernel": (EMBED, 1)}


def init_weights(rng, n_agents, scale=0.5, scope=None):
    """Random float32 weights under the reference's variable names, scaled by scale / sqrt(fan_in) (a conv kernel's fan-in is
    kh * kw * in; the biases: sqrt(4)), in the order the reference creates them.  scope: e.g. "Mixer_target" prefixes the names."""
    def f(shape):
        fan = int(np.prod(shape[:-1])) if len(shape) > 1 else 4
        return (rng.standard_normal(shape) * scale / np.sqrt(fan)).astype(np.float32)
    w = {name: f(shape) for name, shape in shapes(n_agents).items()}
    return w if scope is None else {scope + "/" + k: v for k, v in w.items()}


def _sum128(v):
    """[rows, 128] -> [rows]: the device's tree over the embedding units"""
    s = v.reshape(v.shape[0], 8, 8, 2)
    s = s[..., 0] + s[..., 1]                      # pairs                 [rows, 8, 8]
    s = s.reshape(v.shape[0], 8, 4, 2)
    s = s[..., 0] + s[..., 1]                      # fours                 [rows, 8, 4]
    s = s.reshape(v.shape[0], 8, 2, 2)
    s = s[..., 0] + s[..., 1]                      # eights                [rows, 8, 2]
    s = s[..., 0] + s[..., 1]                      # sixteens              [rows, 8]
    t = s[:, 0] + s[:, 1]
    for j in range(2, 8):
        t = t + s[:, j]
    return t


def q_tot(w, agent_qs, state_env, state, goals_all, dtype=np.float64, order="matmul"):
    """q_tot [rows, 1] of Qmix_mixer_checkers from agent_qs [rows, N], state_env [rows, 3, 9, 2] (or [rows, 54]), state [rows, 4N] (or
    [rows, N, 4]) and goals_all [rows, 2N] (or [rows, N, 2])."""
    w = {canon(k): v for k, v in w.items()}
    f = np.dtype(dtype).type
    W = lambda k: np.asarray(w[k], dtype=f)  # noqa: E731
    q = np.asarray(agent_qs, dtype=f)
    rows, n = q.shape
    conv = conv_same(np.asarray(state_env).reshape(rows, 3, 9, 2), W("conv/Conv/weights"), W("conv/Conv/biases"), dtype)
    x = np.concatenate([conv, np.asarray(state).reshape(rows, -1).astype(f), np.asarray(goals_all).reshape(rows, -1).astype(f)], axis=1)
    assert x.dtype == f and x.shape[1] == CONV_OUT + 6 * n, (x.dtype, x.shape)
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
    y = _sum128(hidden * w_final) + _sum128(l1 * W("hyper_b_final/kernel").reshape(1, EMBED))
    return y.reshape(rows, 1).astype(f)


def torch_mixer(w, agent_qs, state_env, state, goals_all):
    """The network in torch float32 on the tensors' device, from the short-named TF-shaped tensors of a CheckersQmixMixer (mixer.w):
    what plays sess.run(mixer_target) inside `run`.  Any dtype in (a tf.float32 placeholder rounds its feed); float32 [rows, 1] out."""
    import torch
    f32 = lambda t: t.to(torch.float32)  # noqa: E731
    q = f32(agent_qs)
    rows, n = q.shape
    grid = f32(state_env).reshape(rows, 3, 9, 2).permute(0, 3, 1, 2)                                  # NHWC -> NCHW
    kernel = w["conv_w"].permute(3, 2, 0, 1)                                                          # [kh][kw][C][F] -> [F][C][kh][kw]
    conv = torch.relu(torch.nn.functional.conv2d(grid, kernel, w["conv_b"], padding=(1, 2)))         # SAME for 3 x 5, stride 1
    conv = conv.permute(0, 2, 3, 1).reshape(rows, CONV_OUT)                                          # NHWC flatten
    x = torch.cat([conv, f32(state).reshape(rows, -1), f32(goals_all).reshape(rows, -1)], dim=1)
    l1 = torch.relu(x @ w["hyper_b_final_l1"])
    b_final = l1 @ w["hyper_b_final"]
    w1 = torch.abs(x @ w["hyper_w_1"]).reshape(rows, n, EMBED)
    b1 = (x @ w["hyper_b_1"]).reshape(rows, 1, EMBED)
    hidden = torch.nn.functional.elu(q.reshape(rows, 1, n) @ w1 + b1)
    w_final = torch.abs(x @ w["hyper_w_final"]).reshape(rows, EMBED, 1)
    return (hidden @ w_final + b_final.reshape(rows, 1, 1)).reshape(rows, 1)


# ---- the cases of the GPU tests, built once and left unchanged (tests/test_qmix_mixer_checkers_oracle.py checks on the CPU how much of
# the bound the float32 restatement alone uses on them) -------------------------------------------------------------------------------
GPU_AGENTS = (1, 2, 3, 5, 8)
GPU_BATCHES = (1, 3, 13, 67)
GPU_SCALE = 0.5                    # init_weights(scale=...): |q_tot| runs from 0.1 to 145 over the cases
_CACHE = {}


def gpu_weights(n_agents):
    """the Mixer_target weights of the GPU tests' mixer for this agent count"""
    if ("w", n_agents) not in _CACHE:
        _CACHE[("w", n_agents)] = init_weights(np.random.default_rng(700 + n_agents), n_agents, scale=GPU_SCALE, scope="Mixer_target")
    return _CACHE[("w", n_agents)]


def gpu_case(n_agents, batch):
    """the columns of `batch` transitions as NumPy arrays in the compact forms: grid int8 [B, 3, 9, 2] in {0, 1}, vec float64
    [B, N, 4] in +-2, goals uint8 index [B, N], agent_qs float32 [B, N] in +-5, local_rewards float32 [B, N] in +-1, done bool [B]"""
    key = ("case", n_agents, batch)
    if key not in _CACHE:
        rng = np.random.default_rng(9000 + 131 * n_agents + batch)
        B, N = batch, n_agents
        _CACHE[key] = {"grid": rng.integers(0, 2, (B, 3, 9, 2)).astype(np.int8), "vec": rng.uniform(-2, 2, (B, N, 4)),
                       "goals": rng.integers(0, 2, (B, N)).astype(np.uint8), "agent_qs": rng.uniform(-5, 5, (B, N)).astype(np.float32),
                       "local_rewards": rng.uniform(-1, 1, (B, N)).astype(np.float32), "done": rng.random(B) < 0.4}
    return _CACHE[key]


def gpu_ref(n_agents, batch, dtype=np.float64, order="matmul"):
    """the restatement [B] on gpu_case with gpu_weights"""
    key = ("ref", n_agents, batch, np.dtype(dtype).name, order)
    if key not in _CACHE:
        c = gpu_case(n_agents, batch)
        _CACHE[key] = q_tot(gpu_weights(n_agents), c["agent_qs"], c["grid"], c["vec"], np.eye(2)[c["goals"]], dtype=dtype,
                            order=order).reshape(-1)
    return _CACHE[key]
