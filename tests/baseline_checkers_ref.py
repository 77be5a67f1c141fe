"""TEST INFRASTRUCTURE ONLY -- restatement of the Checkers IAC / COMA baseline critics in a chosen dtype (the Checkers counterpart of
tests/baseline_ref.py; test helper, not a test module).

  networks.V_checkers_local    alg/networks.py:415-435   conv = relu(conv2d SAME [3][3][3][6] over t_obs[5][5][3])  -> 150
      x1 = concat(conv, v_obs_self[4], v_goal[2]) [156] -> branch_self 256;  x2 = v_obs_others [2(N-1)] -> stage-2/branch_others 32
  networks.V_checkers_global   alg/networks.py:438-458   conv = relu(conv2d SAME [3][5][2][4] over s_grid[3][9][2]) -> 108
      x1 = concat(conv, s_n[4], g_n[2]) [114] -> V_branch1 256;              x2 = s_others [4(N-1)] -> stage-2/V_branch2 32
      h2 = relu(branch1 . W + branch2 . stage-2 W) (no bias),  out = h2 . out/kernel + out/bias
  networks.Q_coma_checkers     alg/networks.py:293-306
      x = concat(conv_s(s_grid)[108], s_agents[4N], a_others[5(N-1)], g_n[2], g_others[2(N-1)], labels[N], conv_o(t_obs)[150], v_obs[4])
      out = fc3: relu(x . h1 + b) -> relu(. h2 + b) -> . out + b          (256, 256, 5)

The functions take the TILED feeds the reference's train_step builds (the placeholders' arrays), so a test that evaluates them on
the feeds of cm3_amd.batch.baseline_train_step_feeds(env="checkers") checks the device kernels' row decoding independently of it.
"""
import os

import numpy as np

from tests.critic_checkers_ref import conv_same

PREFIXES = ("V_main/", "V_target/", "Q_main/", "Q_target/")
VALUE_NAMES = {"local": ("branch_self", "W_self_h2", "stage-2/branch_others", "stage-2/W_others_h2", "V_checkers_out"),
               "global": ("V_branch1", "W_branch1_h2", "stage-2/V_branch2", "stage-2/W_branch2_h2", "V_out")}
VALUE_CONV = {"local": ((3, 3, 3, 6), (5, 5, 3), 156), "global": ((3, 5, 2, 4), (3, 9, 2), 114)}
Q = "stage-2/Q_coma_checkers/"
H1_1, H1_2, H2, UNITS = 256, 32, 256, 256
CASES = ("local_n1", "local_n3", "global_n2", "global_n8", "coma_n2", "coma_n5")


def canon(name):
    name = name.split(":")[0]
    for prefix in PREFIXES:
        if name.startswith(prefix):
            name = name[len(prefix):]
    return name


def value_k2(n_agents, kind):
    return (2 if kind == "local" else 4) * (n_agents - 1)


def _rand(rng, scale):
    """shape -> float32 weights scaled by scale / sqrt(fan_in) (a conv kernel's fan-in is kh * kw * in; biases: sqrt(4))"""
    def f(*shape):
        fan = int(np.prod(shape[:-1])) if len(shape) > 1 else 4
        return (rng.standard_normal(shape) * scale / np.sqrt(fan)).astype(np.float32)
    return f


def init_value_weights(rng, n_agents, kind, scale=1.5, scope=None):
    """Random float32 weights under the reference's variable names; the three stage-2 tensors only with more than one agent.
    scope: e.g. "V_main" prefixes the names."""
    f = _rand(rng, scale)
    b1, w1, b2, w2, out = VALUE_NAMES[kind]
    conv, _, k1 = VALUE_CONV[kind]
    w = {"conv/Conv/weights": f(*conv), "conv/Conv/biases": f(conv[-1]), b1 + "/kernel": f(k1, H1_1), b1 + "/bias": f(H1_1),
         w1: f(H1_1, H2)}
    if n_agents > 1:
        w.update({b2 + "/kernel": f(value_k2(n_agents, kind), H1_2), b2 + "/bias": f(H1_2), w2: f(H1_2, H2)})
    w[out + "/kernel"] = f(H2, 1)
    w[out + "/bias"] = f(1)
    return w if scope is None else {scope + "/" + k: v for k, v in w.items()}


def init_coma_weights(rng, n_agents, scale=1.5, scope=None):
    f = _rand(rng, scale)
    w = {"conv_s/Conv/weights": f(3, 5, 2, 4), "conv_s/Conv/biases": f(4), "conv_o/Conv/weights": f(3, 3, 3, 6), "conv_o/Conv/biases": f(6),
         Q + "h1/kernel": f(257 + 12 * n_agents, UNITS), Q + "h1/bias": f(UNITS), Q + "h2/kernel": f(UNITS, UNITS), Q + "h2/bias": f(UNITS),
         Q + "out/kernel": f(UNITS, 5), Q + "out/bias": f(5)}
    return w if scope is None else {scope + "/" + k: v for k, v in w.items()}


def _cat(parts, dtype):
    return np.concatenate([np.asarray(p).reshape(np.asarray(p).shape[0], -1) for p in parts], axis=1).astype(dtype)


def _value(w, kind, image, vec_parts, x2, dtype):
    w = {canon(k): v for k, v in w.items()}
    f = np.dtype(dtype).type
    W = lambda k: np.asarray(w[k], dtype=f)  # noqa: E731
    b1, w1, b2, w2, out = VALUE_NAMES[kind]
    rows = np.asarray(vec_parts[0]).shape[0]
    conv = conv_same(np.asarray(image).reshape((rows,) + VALUE_CONV[kind][1]), W("conv/Conv/weights"), W("conv/Conv/biases"), dtype)
    x1 = _cat([conv] + list(vec_parts), dtype)
    h = np.maximum(x1 @ W(b1 + "/kernel") + W(b1 + "/bias"), f(0)) @ W(w1)
    if x2 is not None:
        h = h + np.maximum(_cat([x2], dtype) @ W(b2 + "/kernel") + W(b2 + "/bias"), f(0)) @ W(w2)
    return np.maximum(h, f(0)) @ W(out + "/kernel") + W(out + "/bias")


def v_local(w, obs_self_t, obs_self_v, obs_others, v_goal, stage=2, dtype=np.float64):
    """V [rows, 1] of V_checkers_local"""
    return _value(w, "local", obs_self_t, [obs_self_v, v_goal], obs_others if stage > 1 else None, dtype)


def v_global(w, state_env, v_state_one_agent, v_goal, v_state_other_agents=None, stage=2, dtype=np.float64):
    """V [rows, 1] of V_checkers_global"""
    return _value(w, "global", state_env, [v_state_one_agent, v_goal], v_state_other_agents if stage > 1 else None, dtype)


def q_coma(w, state_env, v_state, action_others, v_goal, v_goal_others, v_labels, obs_self_t, obs_self_v, dtype=np.float64):
    """Q [rows, 5] of Q_coma_checkers; action_others is [rows, N-1, 5] or flat."""
    w = {canon(k): v for k, v in w.items()}
    f = np.dtype(dtype).type
    W = lambda k: np.asarray(w[k], dtype=f)  # noqa: E731
    rows = np.asarray(v_goal).shape[0]
    conv_s = conv_same(np.asarray(state_env).reshape(rows, 3, 9, 2), W("conv_s/Conv/weights"), W("conv_s/Conv/biases"), dtype)
    conv_o = conv_same(np.asarray(obs_self_t).reshape(rows, 5, 5, 3), W("conv_o/Conv/weights"), W("conv_o/Conv/biases"), dtype)
    x = _cat([conv_s, v_state, action_others, v_goal, v_goal_others, v_labels, conv_o, obs_self_v], dtype)
    h1 = np.maximum(x @ W(Q + "h1/kernel") + W(Q + "h1/bias"), f(0))
    h2 = np.maximum(h1 @ W(Q + "h2/kernel") + W(Q + "h2/bias"), f(0))
    return h2 @ W(Q + "out/kernel") + W(Q + "out/bias")


def load_case(golden_dir, tag):
    """(weights, inputs, output) of tests/golden/baseline_checkers_<tag>.npz"""
    z = np.load(os.path.join(golden_dir, "baseline_checkers_%s.npz" % tag))
    w = {str(k): z["w/" + str(k)] for k in z["names"]}
    x = {k[3:]: z[k] for k in z.files if k.startswith("in/")}
    return w, x, z["out"]


def eval_feed(kind, n, w, x, dtype):
    """the restatement on a dict keyed by the reference's placeholder names (a fixture case's inputs, or a train_step feed)"""
    stage = 1 if int(n) == 1 else 2
    if kind == "local":
        return v_local(w, x["obs_self_t"], x["obs_self_v"], x["obs_others"], x["v_goal"], stage=stage, dtype=dtype)
    if kind == "global":
        return v_global(w, x["state_env"], x["v_state_one_agent"], x["v_goal"], x["v_state_other_agents"], stage=stage, dtype=dtype)
    return q_coma(w, x["state_env"], x["v_state"], x["action_others"], x["v_goal"], x["v_goal_others"], x["v_labels"], x["obs_self_t"],
                  x["obs_self_v"], dtype=dtype)


def eval_case(tag, w, x, dtype):
    kind, n = tag.split("_n")
    return eval_feed(kind, n, w, x, dtype)


# ---- the fixture's rows as decodings of base columns -------------------------------------------------------------------------------
def fixture_base_columns(tag, x):
    """The base columns of `rows` time steps, one per fixture row, such that fixture row i is row (i, n_i), n_i = i % N, of the launch:
    returns (cols, pick) with cols = dict(grid, vec, goals, actions, obs_self_t, obs_self_v, obs_others) as float64 / int64 NumPy arrays
    and pick = the index of fixture row i among the launch's rows.  Agents a fixture row does not read get zeros, goal 0, action 0."""
    kind, N = tag.split("_n")
    N = int(N)
    R = x["v_goal"].shape[0]
    ni = np.arange(R) % N
    c = dict(grid=np.zeros((R, 3, 9, 2)), vec=np.zeros((R, N, 4)), goals=np.zeros((R, N, 2), np.int64), actions=np.zeros((R, N), np.int64),
             obs_self_t=np.zeros((R, N, 5, 5, 3)), obs_self_v=np.zeros((R, N, 4)), obs_others=np.zeros((R, N, 2 * max(N - 1, 1))))
    c["goals"][:, :, 0] = 1
    for r in range(R):
        me, others = ni[r], [j for j in range(N) if j != ni[r]]
        c["goals"][r, me] = x["v_goal"][r]
        if kind == "local":
            c["obs_self_t"][r, me], c["obs_self_v"][r, me] = x["obs_self_t"][r], x["obs_self_v"][r]
            if N > 1:
                c["obs_others"][r, me] = x["obs_others"][r]
        elif kind == "global":
            c["grid"][r], c["vec"][r, me] = x["state_env"][r], x["v_state_one_agent"][r]
            if N > 1:
                c["vec"][r, others] = x["v_state_other_agents"][r].reshape(N - 1, 4)
        else:
            assert np.array_equal(x["v_labels"][r], np.eye(N, dtype=np.float32)[me])
            c["grid"][r], c["vec"][r] = x["state_env"][r], x["v_state"][r].reshape(N, 4)
            c["obs_self_t"][r, me], c["obs_self_v"][r, me] = x["obs_self_t"][r], x["obs_self_v"][r]
            c["goals"][r, others] = x["v_goal_others"][r].reshape(N - 1, 2)
            c["actions"][r, others] = x["action_others"][r].reshape(N - 1, 5).argmax(1)
    return c, np.arange(R) * N + ni
