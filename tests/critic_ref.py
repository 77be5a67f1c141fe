"""TEST INFRASTRUCTURE ONLY -- restatement of the CM3 particle critics in a chosen dtype (the critics' counterpart of
tests/qmix_ref.py; test helper, not a test module).

  networks.Q_global_1output   alg/networks.py:97-122
  networks.Q_credit           alg/networks.py:186-211
      branch1 = relu(concat(s_n[4], g_n[2], a[5]) . Q_branch1/kernel + Q_branch1/bias)
      branch2 = relu(x2 . stage-2/Q_branch2/kernel + stage-2/Q_branch2/bias)                    (stage 2)
         global: x2 = concat(s_others[4(N-1)], a_others[5(N-1)]);  credit: x2 = concat(s_m[4], s_others[4(N-1)])
      h2  = relu(branch1 . W_branch1_h2 + branch2 . stage-2/W_branch2_h2),  out = h2 . Q_out/kernel   (no biases)

The functions take the TILED feeds the reference's train_step builds (the placeholders' arrays), so a test that evaluates them
on the feeds of cm3_amd.batch.train_step_feeds checks the device kernel's row decoding independently of it.
"""
import numpy as np

NAMES = ("Q_branch1/kernel", "Q_branch1/bias", "W_branch1_h2", "stage-2/Q_branch2/kernel", "stage-2/Q_branch2/bias",
         "stage-2/W_branch2_h2", "Q_out/kernel")
PREFIXES = ("Q_global_main/", "Q_global_target/", "Q_credit_main/", "Q_credit_target/")


def canon(name):
    name = name.split(":")[0]
    for prefix in PREFIXES:
        if name.startswith(prefix):
            name = name[len(prefix):]
    return name


def k2(n_agents, kind):
    return 9 * (n_agents - 1) if kind == "global" else 4 * n_agents


def init_weights(rng, n_agents, kind, scale=0.5, scope=None):
    """Random float32 weights under the reference's variable names, scaled by scale / sqrt(fan_in) (biases: sqrt(4)); the three
    stage-2 tensors only with more than one agent.  scope: e.g. "Q_credit_main" prefixes the names."""
    f = lambda *shape: (rng.standard_normal(shape) * scale / np.sqrt(shape[0] if len(shape) > 1 else 4)).astype(np.float32)  # noqa: E731
    w = {"Q_branch1/kernel": f(11, 64), "Q_branch1/bias": f(64), "W_branch1_h2": f(64, 64)}
    if n_agents > 1:
        w.update({"stage-2/Q_branch2/kernel": f(k2(n_agents, kind), 128), "stage-2/Q_branch2/bias": f(128),
                  "stage-2/W_branch2_h2": f(128, 64)})
    w["Q_out/kernel"] = f(64, 1)
    return w if scope is None else {scope + "/" + k: v for k, v in w.items()}


def _net(w, x1, x2, dtype):
    w = {canon(k): v for k, v in w.items()}
    f = np.dtype(dtype).type
    W = lambda k: np.asarray(w[k], dtype=f)  # noqa: E731
    b1 = np.maximum(x1 @ W("Q_branch1/kernel") + W("Q_branch1/bias"), f(0))
    h = b1 @ W("W_branch1_h2")
    if x2 is not None:
        b2 = np.maximum(x2 @ W("stage-2/Q_branch2/kernel") + W("stage-2/Q_branch2/bias"), f(0))
        h = h + b2 @ W("stage-2/W_branch2_h2")
    return np.maximum(h, f(0)) @ W("Q_out/kernel")


def _cat(parts, dtype):
    return np.concatenate([np.asarray(p).reshape(np.asarray(p).shape[0], -1) for p in parts], axis=1).astype(dtype)


def q_global(w, s_n, g_n, a_n, s_others=None, a_others=None, stage=2, dtype=np.float64):
    """Q [rows, 1] of Q_global_1output; a_others is [rows, N-1, 5] or flat."""
    x2 = _cat([s_others, a_others], dtype) if stage > 1 else None
    return _net(w, _cat([s_n, g_n, a_n], dtype), x2, dtype)


def q_credit(w, s_n, g_n, a_m, s_m, s_others, dtype=np.float64):
    """Q [rows, 1] of Q_credit (stage 2)."""
    return _net(w, _cat([s_n, g_n, a_m], dtype), _cat([s_m, s_others], dtype), dtype)
