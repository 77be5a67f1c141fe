"""TEST INFRASTRUCTURE ONLY -- restatement of mixer_op of the Checkers QMIX learner in a chosen dtype (helper of
tests/test_qmix_learner_checkers_oracle.py and tests/test_gpu_qmix_learner_checkers.py; not a test module).

  alg_qmix_checkers.py:184-190   loss = mean((td_target - q_tot)^2), q_tot = Qmix_mixer_checkers(reduce_sum(Q * actions_1hot),
                                 state_env, v_state, v_goal_all), Q = Qmix_single_checkers(actions_prev, obs_self_t, obs_self_v,
                                 obs_others, v_goal), minimised by tf.train.AdamOptimizer(lr)

loss_and_grads is the forward pass of tests/qmix_checkers_ref.py and tests/qmix_mixer_checkers_ref.py with every pre-activation kept
(both SAME convolutions written as patches . kernel; tests/test_qmix_learner_checkers_oracle.py holds it to those two), and a backward
pass written by hand with TensorFlow's conventions at the kinks: ReluGrad passes where the input is > 0 (an input of exactly 0 passes
nothing), d|x|/dx = sign(x) (0 at 0), EluGrad below zero is elu + 1.  The td_target placeholder is tf.float32: td is rounded to
float32 before it is used.

Gradients are discontinuous where a relu or abs argument crosses zero, so a parity case keeps every float64 pre-activation of the
agent conv, conv_linear, branch_self, branch_others, h2, the mixer conv, hyper_w_1, hyper_w_final and hyper_b_final_l1 at least MARGIN
from zero; loss_and_grads asserts it (check_margin) and excludes nothing.  A pre-activation that is EXACTLY zero is on no side of the
kink in any precision (an all-zero window under a zero bias): the margin is taken over the others, which is what lets a test pin
"> 0, not >= 0".  MARGIN = 3e-5 is 14 times the largest deviation of a float32 NumPy forward pass from float64 measured under
case()'s recipe (2.03e-6 over 300 seeds at each of eight shapes); the particle learner's 1e-4 leaves no seed at all above about
40 000 pre-activations.  CASES are seeds that satisfy it.

The twenty tensors go under the names of CheckersQmixLearner.grads: "agent/<short name of CK_NAMES>", "mixer/<short name of
CK_MIXER_NAMES>".  adam_state / adam_step are tests/qmix_learner_ref.py's; trajectory is that module's loop on this module's
loss_and_grads.
"""
import numpy as np

from tests import critic_checkers_feeds as CCF
from tests import qmix_checkers_ref as QC
from tests import qmix_mixer_checkers_ref as MC
from tests.qmix_learner_ref import adam_state, adam_step  # noqa: F401

MARGIN = 3e-5
CASES = [(1, 1, 1), (2, 3, 0), (3, 13, 0), (5, 7, 1), (8, 2, 3), (8, 9, 9), (2, 40, 265)]      # (N, B, seed)
# short name -> TF variable (cm3_amd.qmix.CK_NAMES / CK_MIXER_NAMES, restated: a helper of CPU tests imports no device module)
AGENT = {"conv_w": "conv/Conv/weights", "conv_b": "conv/Conv/biases", "lin_w": "conv_linear/kernel", "lin_b": "conv_linear/bias",
         "self_w": "branch_self/kernel", "self_b": "branch_self/bias", "w_self_h2": "W_self_h2", "others_w": "branch_others/kernel",
         "others_b": "branch_others/bias", "w_others_h2": "W_others_h2", "b_h2": "b", "out_w": "Qmix_single_out/kernel",
         "out_b": "Qmix_single_out/bias"}
MIXER = {"conv_w": "conv/Conv/weights", "conv_b": "conv/Conv/biases", "hyper_w_1": "hyper_w_1", "hyper_w_final": "hyper_w_final",
         "hyper_b_1": "hyper_b_1", "hyper_b_final_l1": "hyper_b_final_l1/kernel", "hyper_b_final": "hyper_b_final/kernel"}
NAMES = tuple("agent/" + k for k in AGENT) + tuple("mixer/" + k for k in MIXER)
EMBED = MC.EMBED


def case(N, B, seed):
    """(agent weights, mixer weights, columns of the batch as torch tensors, td [B] float64)"""
    rng = np.random.default_rng(seed)
    wa = QC.init_weights(rng, N)
    wm = MC.init_weights(rng, N, scale=0.5)
    cols = CCF.make_cols(B, N, seed)
    td = rng.uniform(-5, 5, B)
    return wa, wm, cols, td


def short_weights(wa, wm):
    """the twenty tensors under the names of a learner's grads"""
    a = {QC.canon(k): np.asarray(v) for k, v in wa.items()}
    m = {MC.canon(k): np.asarray(v) for k, v in wm.items()}
    w = {"agent/" + short: a[name] for short, name in AGENT.items()}
    w.update({"mixer/" + short: m[name] for short, name in MIXER.items()})
    return w


def patches(x, kh, kw):
    """[rows, H, W, C] -> [rows, H W, kh kw C]: the SAME-padded (zeros) kh x kw neighbourhood of every position, in the order of a TF
    conv kernel [kh][kw][C][F] flattened over its first three axes"""
    rows, H, W, C = x.shape
    ph, pw = kh // 2, kw // 2
    xp = np.zeros((rows, H + 2 * ph, W + 2 * pw, C), dtype=x.dtype)
    xp[:, ph:ph + H, pw:pw + W] = x
    out = np.stack([xp[:, dr:dr + H, dc:dc + W] for dr in range(kh) for dc in range(kw)], axis=3)      # [rows, H, W, kh kw, C]
    return out.reshape(rows, H * W, kh * kw * C)


def arrays(cols):
    """the columns as float64 / int64 NumPy arrays: windows [R, 5, 5, 3], obs_self_v [R, 4], obs_others [R, Lo], a_prev [R],
    goals one-hot [R, 2], actions [R], grid [B, 3, 9, 2], vec [B, 4 N]"""
    g = lambda k: cols[k].detach().cpu().numpy() if hasattr(cols[k], "detach") else np.asarray(cols[k])      # noqa: E731
    vec = g("vec")
    B, N = vec.shape[0], vec.shape[1]
    R = B * N
    goals = g("goals")
    if goals.shape == (B, N):
        goals = np.eye(2)[goals.astype(np.int64)]
    f = np.float64
    return {"win": g("obs_self_t").reshape(R, 5, 5, 3).astype(f), "sv": g("obs_self_v").reshape(R, 4).astype(f),
            "oth": g("obs_others").reshape(R, -1).astype(f), "ap": g("actions_prev").reshape(R).astype(np.int64),
            "goal": goals.reshape(R, 2).astype(f), "act": g("actions").reshape(R).astype(np.int64),
            "grid": g("grid").reshape(B, 3, 9, 2).astype(f), "vec": vec.reshape(B, 4 * N).astype(f), "B": B, "N": N}


def _margin(pre):
    """the smallest |pre-activation| that is not exactly zero"""
    best = np.inf
    for a in pre:
        a = np.abs(np.asarray(a, dtype=np.float64))
        a = a[a != 0]
        if a.size:
            best = min(best, float(a.min()))
    return best


def loss_and_grads(w, cols, td, dtype=np.float64, check_margin=True, pass_at_zero=False):
    """{"loss": scalar, "q_tot": [B], "q_sel": [B, N], "grads": {name: array}, "margin": float, "pre": the kinked pre-activations} of
    the twenty tensors `w` (names of NAMES) on the batch, every operation in `dtype`.  pass_at_zero=True is NOT TensorFlow's ReluGrad:
    both convolutions pass the gradient at an input of exactly 0 (>= 0), which is what the kink case must tell apart."""
    f = np.dtype(dtype).type
    A = {k: np.asarray(w["agent/" + k], dtype=f) for k in AGENT}
    M = {k: np.asarray(w["mixer/" + k], dtype=f) for k in MIXER}
    c = arrays(cols)
    B, N = c["B"], c["N"]
    R = B * N
    relu = lambda v: np.maximum(v, f(0))      # noqa: E731
    conv_mask = (lambda z: z >= 0) if pass_at_zero else (lambda z: z > 0)      # noqa: E731
    # ---- forward: the agent network ----
    pa = patches(c["win"].astype(f), 3, 3)                                   # [R, 25, 27]
    z_c = pa @ A["conv_w"].reshape(27, 6) + A["conv_b"]                      # [R, 25, 6]: NHWC
    c1 = relu(z_c).reshape(R, 150)
    z_l = c1 @ A["lin_w"] + A["lin_b"]
    a1 = np.zeros((R, 5), f)
    a1[np.arange(R), c["ap"]] = 1
    xs = np.concatenate([relu(z_l), c["sv"].astype(f), a1, c["goal"].astype(f)], axis=1)
    z_s = xs @ A["self_w"] + A["self_b"]
    hs = relu(z_s)
    xo = c["oth"].astype(f)
    z_o = xo @ A["others_w"] + A["others_b"]
    ho = relu(z_o)
    z_2 = hs @ A["w_self_h2"] + ho @ A["w_others_h2"] + A["b_h2"]
    h2 = relu(z_2)
    Q = h2 @ A["out_w"] + A["out_b"]
    q = Q[np.arange(R), c["act"]].reshape(B, N)
    # ---- forward: the mixer ----
    pm = patches(c["grid"].astype(f), 3, 5)                                  # [B, 27, 30]
    z_m = pm @ M["conv_w"].reshape(30, 4) + M["conv_b"]                      # [B, 27, 4]
    xm = np.concatenate([relu(z_m).reshape(B, 108), c["vec"].astype(f), c["goal"].reshape(B, 2 * N).astype(f)], axis=1)
    z_l1 = xm @ M["hyper_b_final_l1"]
    l1 = relu(z_l1)
    z_w1 = (xm @ M["hyper_w_1"]).reshape(B, N, EMBED)
    w1 = np.abs(z_w1)
    z_wf = xm @ M["hyper_w_final"]
    wf = np.abs(z_wf)
    h = np.einsum("bn,bne->be", q, w1) + xm @ M["hyper_b_1"]
    hidden = np.where(h > 0, h, np.expm1(np.minimum(h, f(0))))
    q_tot = np.sum(hidden * wf, axis=1) + (l1 @ M["hyper_b_final"])[:, 0]
    td32 = np.asarray(td, np.float64).astype(np.float32).astype(f)
    loss = np.mean((td32 - q_tot) ** 2)
    pre = {"conv": z_c, "conv_linear": z_l, "branch_self": z_s, "branch_others": z_o, "h2": z_2, "mixer_conv": z_m, "hyper_w_1": z_w1,
           "hyper_w_final": z_wf, "hyper_b_final_l1": z_l1}
    margin = _margin(pre.values())
    if check_margin:
        assert margin >= MARGIN, "a pre-activation is %.3g from a kink: not a parity case" % margin
    # ---- backward: the mixer ----
    dq = (f(2) * (q_tot - td32) / f(B))[:, None]
    G = {}
    d_l1 = dq * M["hyper_b_final"][:, 0][None, :] * (z_l1 > 0)
    d_wf = dq * hidden * np.sign(z_wf)
    dh = dq * wf * np.where(h > 0, f(1), hidden + f(1))
    d_w1 = (dh[:, None, :] * q[:, :, None] * np.sign(z_w1)).reshape(B, N * EMBED)
    G["mixer/hyper_b_final"] = l1.T @ dq
    G["mixer/hyper_b_final_l1"] = xm.T @ d_l1
    G["mixer/hyper_w_final"] = xm.T @ d_wf
    G["mixer/hyper_b_1"] = xm.T @ dh
    G["mixer/hyper_w_1"] = xm.T @ d_w1
    dxm = d_l1 @ M["hyper_b_final_l1"].T + d_wf @ M["hyper_w_final"].T + dh @ M["hyper_b_1"].T + d_w1 @ M["hyper_w_1"].T
    d_m = dxm[:, :108].reshape(B, 27, 4) * conv_mask(z_m)
    G["mixer/conv_w"] = (pm.reshape(B * 27, 30).T @ d_m.reshape(B * 27, 4)).reshape(3, 5, 2, 4)
    G["mixer/conv_b"] = d_m.reshape(B * 27, 4).sum(axis=0)
    # ---- backward: the agent network ----
    dqsel = np.einsum("be,bne->bn", dh, w1).reshape(R)
    dQ = np.zeros_like(Q)
    dQ[np.arange(R), c["act"]] = dqsel
    G["agent/out_w"], G["agent/out_b"] = h2.T @ dQ, dQ.sum(axis=0)
    d2 = (dQ @ A["out_w"].T) * (z_2 > 0)
    G["agent/w_self_h2"], G["agent/w_others_h2"], G["agent/b_h2"] = hs.T @ d2, ho.T @ d2, d2.sum(axis=0)
    ds = (d2 @ A["w_self_h2"].T) * (z_s > 0)
    do = (d2 @ A["w_others_h2"].T) * (z_o > 0)
    G["agent/self_w"], G["agent/self_b"] = xs.T @ ds, ds.sum(axis=0)
    G["agent/others_w"], G["agent/others_b"] = xo.T @ do, do.sum(axis=0)
    dl = (ds @ A["self_w"].T)[:, :32] * (z_l > 0)
    G["agent/lin_w"], G["agent/lin_b"] = c1.T @ dl, dl.sum(axis=0)
    dc = (dl @ A["lin_w"].T).reshape(R, 25, 6) * conv_mask(z_c)
    G["agent/conv_w"] = (pa.reshape(R * 25, 27).T @ dc.reshape(R * 25, 6)).reshape(3, 3, 3, 6)
    G["agent/conv_b"] = dc.reshape(R * 25, 6).sum(axis=0)
    grads = {k: G[k].reshape(np.shape(w[k])) for k in NAMES}
    return {"loss": loss, "q_tot": q_tot, "q_sel": q, "grads": grads, "margin": margin, "pre": pre}


def trajectory(w, cols, td, steps, lr=1e-3, dtype=np.float64):
    """the losses of `steps` Adam steps on one fixed batch (tests/qmix_learner_ref.trajectory on this module's loss_and_grads; no margin
    condition: the loss is continuous across the kinks)"""
    m, v, p = adam_state(w, dtype=dtype)
    losses = []
    for _ in range(steps):
        out = loss_and_grads(w, cols, td, dtype=dtype, check_margin=False)
        losses.append(float(out["loss"]))
        w, m, v, p = adam_step(w, out["grads"], m, v, p, lr=lr, dtype=dtype)
    return losses


KINK = (2, 3, 0)      # (N, B, seed) of kink_case: satisfies MARGIN after the changes below


def kink_case():
    """case(*KINK) with both conv biases 0.0, agent row 0's window all zero and transition 0's grid all zero: those conv
    pre-activations are exactly 0 in any precision, where ReluGrad passes nothing."""
    wa, wm, cols, td = case(*KINK)
    wa = {k: (np.zeros_like(v) if k.endswith("conv/Conv/biases") else v) for k, v in wa.items()}
    wm = {k: (np.zeros_like(v) if k.endswith("conv/Conv/biases") else v) for k, v in wm.items()}
    cols = dict(cols)
    cols["obs_self_t"] = cols["obs_self_t"].clone()
    cols["obs_self_t"][0, 0] = 0
    cols["grid"] = cols["grid"].clone()
    cols["grid"][0] = 0
    return wa, wm, cols, td


# ---- the cases, built once and left unchanged -------------------------------------------------------------------------------------------
_CACHE = {}


def cached_case(N, B, seed):
    """case() and its float64 reference, shared by the tests: (wa, wm, cols, td, short weights, loss_and_grads in float64)"""
    key = (N, B, seed)
    if key not in _CACHE:
        wa, wm, cols, td = case(N, B, seed)
        w = short_weights(wa, wm)
        _CACHE[key] = (wa, wm, cols, td, w, loss_and_grads(w, cols, td))
    return _CACHE[key]
