"""TEST INFRASTRUCTURE ONLY -- restatement of the CM3 Checkers critics in a chosen dtype (the Checkers counterpart of
tests/critic_ref.py; test helper, not a test module).

  networks.Q_global_checkers   alg/networks.py:155-183
  networks.Q_credit_checkers   alg/networks.py:244-272     (widths of config_checkers_stage{1,2}.json)
      conv    = relu(conv2d SAME [3][5][2][4] over s_grid[3][9][2] + biases)  flattened NHWC -> 108     (networks.convnet_1 :67-75)
      conv_o  = relu(conv2d SAME [3][3][3][6] over t_obs[5][5][3] + biases)                  -> 150
      branch1 = relu(concat(conv, s_n[4], g_n[2], a[5], conv_o, v_obs[4]) . Q_branch1/kernel + Q_branch1/bias)
      branch2 = relu(x2 . stage-2/Q_branch2/kernel + stage-2/Q_branch2/bias)                           (stage 2)
         global: x2 = concat(s_others[4(N-1)], a_others[5(N-1)]);  credit: x2 = concat(s_m[4], s_others[4(N-1)])
      h2  = relu(branch1 . W_branch1_h2 + branch2 . stage-2/W_branch2_h2),  out = h2 . Q_out/kernel + Q_out/bias

The functions take the TILED feeds the reference's train_step builds (the placeholders' arrays), so a test that evaluates them
on the feeds of cm3_amd.batch.train_step_feeds checks the device kernel's row decoding independently of it.
"""
import numpy as np

NAMES = ("conv/Conv/weights", "conv/Conv/biases", "conv_o/Conv/weights", "conv_o/Conv/biases", "Q_branch1/kernel", "Q_branch1/bias",
         "W_branch1_h2", "stage-2/Q_branch2/kernel", "stage-2/Q_branch2/bias", "stage-2/W_branch2_h2", "Q_out/kernel", "Q_out/bias")
PREFIXES = ("Q_global_main/", "Q_global_target/", "Q_credit_main/", "Q_credit_target/")
H1_1, H1_2, H2 = 256, 32, 256


def canon(name):
    name = name.split(":")[0]
    for prefix in PREFIXES:
        if name.startswith(prefix):
            name = name[len(prefix):]
    return name


def k2(n_agents, kind):
    return 9 * (n_agents - 1) if kind == "global" else 4 * n_agents


def init_weights(rng, n_agents, kind, scale=1.5, scope=None):
    """Random float32 weights under the reference's variable names, scaled by scale / sqrt(fan_in) (a conv kernel's fan-in is
    kh * kw * in; biases: sqrt(4)); the three stage-2 tensors only with more than one agent.  scope: e.g. "Q_credit_main" prefixes
    the names."""
    def f(*shape):
        fan = int(np.prod(shape[:-1])) if len(shape) > 1 else 4
        return (rng.standard_normal(shape) * scale / np.sqrt(fan)).astype(np.float32)
    w = {"conv/Conv/weights": f(3, 5, 2, 4), "conv/Conv/biases": f(4), "conv_o/Conv/weights": f(3, 3, 3, 6), "conv_o/Conv/biases": f(6),
         "Q_branch1/kernel": f(273, H1_1), "Q_branch1/bias": f(H1_1), "W_branch1_h2": f(H1_1, H2)}
    if n_agents > 1:
        w.update({"stage-2/Q_branch2/kernel": f(k2(n_agents, kind), H1_2), "stage-2/Q_branch2/bias": f(H1_2),
                  "stage-2/W_branch2_h2": f(H1_2, H2)})
    w["Q_out/kernel"] = f(H2, 1)
    w["Q_out/bias"] = f(1)
    return w if scope is None else {scope + "/" + k: v for k, v in w.items()}


def conv_same(x, kernel, bias, dtype):
    """relu(conv2d SAME, stride 1) of x [rows, H, W, C] with kernel [kh, kw, C, F], flattened NHWC to [rows, H * W * F]"""
    f = np.dtype(dtype).type
    x, kernel, bias = np.asarray(x, dtype=f), np.asarray(kernel, dtype=f), np.asarray(bias, dtype=f)
    rows, H, W, C = x.shape
    kh, kw, _, F = kernel.shape
    xp = np.zeros((rows, H + kh - 1, W + kw - 1, C), dtype=f)
    xp[:, kh // 2:kh // 2 + H, kw // 2:kw // 2 + W] = x
    out = np.zeros((rows, H, W, F), dtype=f)
    for dr in range(kh):
        for dc in range(kw):
            out += xp[:, dr:dr + H, dc:dc + W] @ kernel[dr, dc]
    return np.maximum(out + bias, f(0)).reshape(rows, H * W * F)


def _cat(parts, dtype):
    return np.concatenate([np.asarray(p).reshape(np.asarray(p).shape[0], -1) for p in parts], axis=1).astype(dtype)


def _net(w, s_grid, t_obs, mid, v_obs, x2, dtype):
    w = {canon(k): v for k, v in w.items()}
    f = np.dtype(dtype).type
    W = lambda k: np.asarray(w[k], dtype=f)  # noqa: E731
    rows = np.asarray(v_obs).shape[0]
    conv = conv_same(np.asarray(s_grid).reshape(rows, 3, 9, 2), W("conv/Conv/weights"), W("conv/Conv/biases"), dtype)
    conv_o = conv_same(np.asarray(t_obs).reshape(rows, 5, 5, 3), W("conv_o/Conv/weights"), W("conv_o/Conv/biases"), dtype)
    x1 = _cat([conv] + list(mid) + [conv_o, v_obs], dtype)
    b1 = np.maximum(x1 @ W("Q_branch1/kernel") + W("Q_branch1/bias"), f(0))
    h = b1 @ W("W_branch1_h2")
    if x2 is not None:
        b2 = np.maximum(x2 @ W("stage-2/Q_branch2/kernel") + W("stage-2/Q_branch2/bias"), f(0))
        h = h + b2 @ W("stage-2/W_branch2_h2")
    return np.maximum(h, f(0)) @ W("Q_out/kernel") + W("Q_out/bias")


def q_global(w, s_grid, s_n, g_n, a_n, s_others, a_others, t_obs, v_obs, stage=2, dtype=np.float64):
    """Q [rows, 1] of Q_global_checkers; a_others is [rows, N-1, 5] or flat."""
    x2 = _cat([s_others, a_others], dtype) if stage > 1 else None
    return _net(w, s_grid, t_obs, [s_n, g_n, a_n], v_obs, x2, dtype)


def q_credit(w, s_grid, s_n, g_n, a_m, s_m, s_others, t_obs, v_obs, dtype=np.float64):
    """Q [rows, 1] of Q_credit_checkers (stage 2)."""
    return _net(w, s_grid, t_obs, [s_n, g_n, a_m], v_obs, _cat([s_m, s_others], dtype), dtype)


def q_from_feed(w, kind, feed, stage=2, dtype=np.float64):
    """Q [rows, 1] from a feed dict keyed by the reference's placeholder attribute names (what train_step_feeds hands to `run`)"""
    a = lambda k: np.asarray(feed[k].detach().cpu().numpy() if hasattr(feed[k], "detach") else feed[k])  # noqa: E731
    if kind == "global":
        return q_global(w, a("state_env"), a("v_state_one_agent"), a("v_goal"), a("action_one"),
                        a("v_state_other_agents") if stage > 1 else None, a("action_others") if stage > 1 else None,
                        a("obs_self_t"), a("obs_self_v"), stage=stage, dtype=dtype)
    return q_credit(w, a("state_env"), a("v_state_one_agent"), a("v_goal"), a("action_one"), a("v_state_m"),
                    a("v_state_other_agents"), a("obs_self_t"), a("obs_self_v"), dtype=dtype)


# ---- the fixture's rows as decodings of base columns -------------------------------------------------------------------------------
def pair_agents(rows, n_agents):
    """(n, m) of fixture row i, as tools/gen_golden_critic_checkers.py lays them out: n = i % N, m = (i // N) % N"""
    i = np.arange(rows)
    return i % n_agents, (i // n_agents) % n_agents


def fixture_base_columns(kind, n_agents, x):
    """The base columns of `rows` time steps, one per fixture row, such that fixture row i is row (i, n_i) of the ROWS form (global)
    or row (i, m_i, n_i) of the PAIRS form (credit): returns (cols, pick) with cols = dict(grid, vec, goals, actions, obs_self_t,
    obs_self_v) as float64 / int64 NumPy arrays and pick = the index of fixture row i among the launch's rows.  Agents a fixture row
    does not read get zeros (state, window), goal 0 and action 0."""
    N = n_agents
    rows = x["s_n"].shape[0]
    n, m = pair_agents(rows, N)
    if kind == "global":
        m = n
    vec = np.zeros((rows, N, 4))
    goals = np.zeros((rows, N, 2), np.int64)
    goals[:, :, 0] = 1
    actions = np.zeros((rows, N), np.int64)
    win = np.zeros((rows, N, 5, 5, 3))
    vobs = np.zeros((rows, N, 4))
    for i in range(rows):
        others = [j for j in range(N) if j != n[i]]
        vec[i, n[i]] = x["s_n"][i]
        if N > 1:
            vec[i, others] = x["s_others"][i].reshape(N - 1, 4)
        goals[i, n[i]] = x["g_n"][i]
        if kind == "global":
            actions[i, n[i]] = int(np.argmax(x["a_n"][i]))
            if N > 1:
                actions[i, others] = np.argmax(x["a_others"][i].reshape(N - 1, 5), axis=1)
        else:
            actions[i, m[i]] = int(np.argmax(x["a_m"][i]))
            assert np.array_equal(vec[i, m[i]].astype(np.float32), x["s_m"][i])
        win[i, m[i]] = x["t_obs"][i]
        vobs[i, m[i]] = x["v_obs"][i]
    i = np.arange(rows)
    pick = i * N + n if kind == "global" else (i * N + m) * N + n
    cols = dict(grid=x["s_grid"].astype(np.float64), vec=vec, goals=goals, actions=actions, obs_self_t=win, obs_self_v=vobs)
    return cols, pick
