"""TEST INFRASTRUCTURE ONLY -- restatement of the IAC / COMA baseline critics of the particle env in a chosen dtype (the counterpart of
tests/critic_ref.py; test helper, not a test module).

  networks.V_particle_local    alg/networks.py:356-374      x1 = concat(v_obs[4], v_goal[2]),           x2 = obs_others [4(N-1)]
  networks.V_particle_global   alg/networks.py:377-402      x1 = concat(v_state_one_agent[4], v_goal[2]),
                                                            x2 = concat(v_state_other_agents[4(N-1)], v_goal_others[2(N-1)])
      branch1 = relu(x1 . kernel + bias)      branch2 = relu(x2 . stage-2 kernel + bias)    (stage 2)
      h2 = relu(branch1 . W + branch2 . stage-2 W),  out = h2 . V_particle_out/kernel        (no biases)
  networks.Q_global            alg/networks.py:84-94        x = concat(v_state[4N], action_others[5(N-1)], v_goal[2], v_goal_others[2(N-1)],
                                                                       agent_labels[N], v_obs[4])
      out = fc3: relu(x . h1 + b) -> relu(. h2 + b) -> . out + b          (256, 256, 5)

The functions take the TILED feeds the reference's train_step builds (the placeholders' arrays), so a test that evaluates them on
the feeds of cm3_amd.batch.baseline_train_step_feeds checks the device kernels' row decoding independently of it.
"""
import numpy as np

PREFIXES = ("V_main/", "V_target/", "Q_main/", "Q_target/")
VALUE_NAMES = {"local": ("V_particle_branch_self", "W_branch_self_out", "stage-2/V_local_others", "stage-2/W_others_out"),
               "global": ("V_particle_branch1", "W_branch1_h2", "stage-2/V_particle_branch2", "stage-2/W_branch2_h2")}
Q = "stage-2/Q_goals/"


def canon(name):
    name = name.split(":")[0]
    for prefix in PREFIXES:
        if name.startswith(prefix):
            name = name[len(prefix):]
    return name


def value_k2(n_agents, kind):
    return (4 if kind == "local" else 6) * (n_agents - 1)


def _rand(rng, scale):
    return lambda *shape: (rng.standard_normal(shape) * scale / np.sqrt(shape[0] if len(shape) > 1 else 4)).astype(np.float32)


def init_value_weights(rng, n_agents, kind, scale=0.5, scope=None):
    """Random float32 weights under the reference's variable names, scaled by scale / sqrt(fan_in) (biases: sqrt(4)); the three
    stage-2 tensors only with more than one agent.  scope: e.g. "V_main" prefixes the names."""
    f = _rand(rng, scale)
    b1, w1, b2, w2 = VALUE_NAMES[kind]
    w = {b1 + "/kernel": f(6, 64), b1 + "/bias": f(64), w1: f(64, 64)}
    if n_agents > 1:
        w.update({b2 + "/kernel": f(value_k2(n_agents, kind), 128), b2 + "/bias": f(128), w2: f(128, 64)})
    w["V_particle_out/kernel"] = f(64, 1)
    return w if scope is None else {scope + "/" + k: v for k, v in w.items()}


def init_coma_weights(rng, n_agents, scale=0.5, scope=None):
    f = _rand(rng, scale)
    w = {Q + "h1/kernel": f(12 * n_agents - 1, 256), Q + "h1/bias": f(256), Q + "h2/kernel": f(256, 256), Q + "h2/bias": f(256),
         Q + "out/kernel": f(256, 5), Q + "out/bias": f(5)}
    return w if scope is None else {scope + "/" + k: v for k, v in w.items()}


def _cat(parts, dtype):
    return np.concatenate([np.asarray(p).reshape(np.asarray(p).shape[0], -1) for p in parts], axis=1).astype(dtype)


def _value(w, kind, x1, x2, dtype):
    w = {canon(k): v for k, v in w.items()}
    f = np.dtype(dtype).type
    W = lambda k: np.asarray(w[k], dtype=f)  # noqa: E731
    b1, w1, b2, w2 = VALUE_NAMES[kind]
    h = np.maximum(x1 @ W(b1 + "/kernel") + W(b1 + "/bias"), f(0)) @ W(w1)
    if x2 is not None:
        h = h + np.maximum(x2 @ W(b2 + "/kernel") + W(b2 + "/bias"), f(0)) @ W(w2)
    return np.maximum(h, f(0)) @ W("V_particle_out/kernel")


def v_local(w, obs_others, v_obs, v_goal, stage=2, dtype=np.float64):
    """V [rows, 1] of V_particle_local"""
    return _value(w, "local", _cat([v_obs, v_goal], dtype), _cat([obs_others], dtype) if stage > 1 else None, dtype)


def v_global(w, v_state_one_agent, v_goal, v_state_other_agents=None, v_goal_others=None, stage=2, dtype=np.float64):
    """V [rows, 1] of V_particle_global"""
    x2 = _cat([v_state_other_agents, v_goal_others], dtype) if stage > 1 else None
    return _value(w, "global", _cat([v_state_one_agent, v_goal], dtype), x2, dtype)


def q_coma(w, v_state, action_others, v_goal, v_goal_others, v_labels, v_obs, dtype=np.float64):
    """Q [rows, 5] of Q_global; action_others is [rows, N-1, 5] or flat."""
    w = {canon(k): v for k, v in w.items()}
    f = np.dtype(dtype).type
    W = lambda k: np.asarray(w[Q + k], dtype=f)  # noqa: E731
    x = _cat([v_state, action_others, v_goal, v_goal_others, v_labels, v_obs], dtype)
    h1 = np.maximum(x @ W("h1/kernel") + W("h1/bias"), f(0))
    h2 = np.maximum(h1 @ W("h2/kernel") + W("h2/bias"), f(0))
    return h2 @ W("out/kernel") + W("out/bias")


def load_case(golden_dir, tag):
    """(weights, inputs, output) of fixture case `tag` of tests/golden/baseline_particle{,_coma}.npz"""
    import os
    for name in ("baseline_particle.npz", "baseline_particle_coma.npz"):
        z = np.load(os.path.join(golden_dir, name))
        if tag + "/out" in z.files:
            w = {str(k): z["%s/w/%s" % (tag, k)] for k in z[tag + "/names"]}
            x = {k.split("/in/")[1]: z[k] for k in z.files if k.startswith(tag + "/in/")}
            return w, x, z[tag + "/out"]
    raise KeyError(tag)


VALUE_CASES = tuple("%s_n%d" % (k, n) for n in (1, 2, 4, 10) for k in ("local", "global"))
COMA_CASES = ("coma_n2", "coma_n4", "coma_n10")


def eval_case(tag, w, x, dtype):
    """the restatement on a fixture case's placeholder inputs"""
    kind, n = tag.split("_n")
    stage = 1 if int(n) == 1 else 2
    if kind == "local":
        return v_local(w, x["obs_others"], x["v_obs"], x["v_goal"], stage=stage, dtype=dtype)
    if kind == "global":
        return v_global(w, x["v_state_one_agent"], x["v_goal"], x["v_state_other_agents"], x["v_goal_others"], stage=stage, dtype=dtype)
    return q_coma(w, x["v_state"], x["action_others"], x["v_goal"], x["v_goal_others"], x["v_labels"], x["v_obs"], dtype=dtype)
