"""TEST INFRASTRUCTURE ONLY -- float64 restatement of the QMIX baseline's Checkers agent network (the QMIX counterpart of
oracle/actor_checkers_oracle.py; test helper, not a test module).

  networks.Qmix_single_checkers      alg/networks.py:617-637 (widths: the actor's nn block, alg_qmix_checkers.py:84-88)
      conv (convnet_1: 3x3 SAME, 6 filters, relu) -> dense 32 relu ("conv_linear")
      -> concat(conv_linear, v_obs_self[4], a_prev[5], v_goal[2]) -> dense 256 relu ("branch_self") -> x W_self_h2
      v_obs_others -> dense 256 relu ("branch_others") -> x W_others_h2          (at EVERY agent count: 2 inputs at N = 1)
      h2 = relu(sum + b) -> dense 5 ("Qmix_single_out"): Q values, no softmax
  alg_qmix_checkers.Alg.run_actor    alg/alg_qmix_checkers.py:153-182
      per agent: with probability epsilon a uniform action, else argmax Q (tf.argmax: the first index on ties)

The exploration stream is the particle agent's (tests/qmix_ref.py: explore_words / epsilon_greedy), keyed with the Checkers env's
episode and step counters.
"""
import numpy as np

from oracle.actor_checkers_oracle import conv_same_3x3
from tests.qmix_ref import canon, epsilon_greedy, explore_words  # noqa: F401  (the shared exploration stream)

CONV_F, CONV_LIN, H1, H2, N_ACTIONS = 6, 32, 256, 256, 5
# the thirteen variables of networks.Qmix_single_checkers, by the names the reference's code creates under "Agent_main/"
NAMES = ("conv/Conv/weights", "conv/Conv/biases", "conv_linear/kernel", "conv_linear/bias", "branch_self/kernel",
         "branch_self/bias", "W_self_h2", "branch_others/kernel", "branch_others/bias", "W_others_h2", "b",
         "Qmix_single_out/kernel", "Qmix_single_out/bias")


def shapes(n_agents):
    lo = 2 * max(n_agents - 1, 1)
    return {"conv/Conv/weights": (3, 3, 3, CONV_F), "conv/Conv/biases": (CONV_F,), "conv_linear/kernel": (25 * CONV_F, CONV_LIN),
            "conv_linear/bias": (CONV_LIN,), "branch_self/kernel": (CONV_LIN + 4 + N_ACTIONS + 2, H1), "branch_self/bias": (H1,),
            "W_self_h2": (H1, H2), "branch_others/kernel": (lo, H1), "branch_others/bias": (H1,), "W_others_h2": (H1, H2),
            "b": (H2,), "Qmix_single_out/kernel": (H2, N_ACTIONS), "Qmix_single_out/bias": (N_ACTIONS,)}


def init_weights(rng, n_agents, scale=1.0):
    """Random weights under the reference's variable names (Agent_main scope, alg_qmix_checkers.py:84-85).  (Larger than the
    reference's initialisers, so that the Q values are spread.)"""
    fan = {"conv/Conv/weights": 27, "conv/Conv/biases": 4, "conv_linear/bias": 4, "branch_self/bias": 4,
           "branch_others/bias": 4, "b": 4, "Qmix_single_out/kernel": 16, "Qmix_single_out/bias": 4}
    out = {}
    for name, shape in shapes(n_agents).items():
        f = fan.get(name, shape[0])
        out["Agent_main/" + name] = (rng.standard_normal(shape) * scale / np.sqrt(f)).astype(np.float32)
    return out


def q_values(w, a_prev, obs_self_t, obs_self_v, obs_others, goals_onehot, dtype=np.float64):
    """Q [rows, 5] in `dtype` (float64: the reference the device agent is measured against).  a_prev int [rows];
    obs_self_t [rows, 5, 5, 3]; obs_self_v [rows, 4]; obs_others [rows, 2 max(N-1, 1)]; goals_onehot [rows, 2]."""
    w = {canon(k): v for k, v in w.items()}
    f = np.dtype(dtype).type
    W = lambda k: np.asarray(w[k], dtype=f)  # noqa: E731
    relu = lambda v: np.maximum(v, f(0))  # noqa: E731
    rows = obs_self_t.shape[0]
    conv = relu(conv_same_3x3(np.asarray(obs_self_t).astype(f), w["conv/Conv/weights"], w["conv/Conv/biases"], dtype=f))
    lin = relu(conv.reshape(rows, -1) @ W("conv_linear/kernel") + W("conv_linear/bias"))
    a1 = np.zeros((rows, N_ACTIONS), f)
    a1[np.arange(rows), np.asarray(a_prev).reshape(-1)] = 1
    x = np.concatenate([lin, np.asarray(obs_self_v).astype(f), a1, np.asarray(goals_onehot).astype(f)], axis=1)
    h_self = relu(x @ W("branch_self/kernel") + W("branch_self/bias"))
    h_oth = relu(np.asarray(obs_others).astype(f) @ W("branch_others/kernel") + W("branch_others/bias"))
    h2 = relu(h_self @ W("W_self_h2") + h_oth @ W("W_others_h2") + W("b"))
    return h2 @ W("Qmix_single_out/kernel") + W("Qmix_single_out/bias")
