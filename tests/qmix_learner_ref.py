"""TEST INFRASTRUCTURE ONLY -- restatement of mixer_op of the particle QMIX learner in a chosen dtype (helper of
tests/test_qmix_learner_oracle.py and tests/test_gpu_qmix_learner.py; not a test module).

  alg_qmix.py:186-192   loss = mean((td_target - q_tot)^2), q_tot = Qmix_mixer(reduce_sum(Q * actions_1hot), state, goals_all),
                        Q = Qmix_single_particle(obs_others, v_obs, v_goal), minimised by tf.train.AdamOptimizer(lr)

loss_and_grads is the forward pass of tests/qmix_ref.py and tests/qmix_mixer_ref.py with every pre-activation kept, and a backward pass
written by hand with TensorFlow's conventions at the kinks: ReluGrad passes where the input is > 0, d|x|/dx = sign(x) (0 at 0),
EluGrad below zero is elu + 1.  The td_target placeholder is tf.float32: td is rounded to float32 before it is used.

Gradients are discontinuous where a relu or abs argument crosses zero, so a parity case must keep every float64 pre-activation of h,
h2, hyper_w_1, hyper_w_final and hyper_b_final_l1 at least MARGIN from zero -- 50 times the forward error of a float32 evaluation
here; loss_and_grads asserts it (check_margin) and excludes nothing.  CASES are seeds that satisfy it under case()'s recipe.

adam_step is tf.train.AdamOptimizer's update (TF1: epsilon outside the bias correction) on dicts of arrays, in a chosen dtype.
"""
import numpy as np

from tests import critic_feeds as CF
from tests import qmix_mixer_ref as MR
from tests import qmix_ref as QR

MARGIN = 1e-4
CASES = [(1, 1, 0), (2, 3, 1), (3, 13, 0), (4, 37, 111), (5, 16, 26), (8, 17, 200), (10, 19, 291)]      # (N, B, seed)
AGENT = QR.NAMES
# short name of ParticleQmixMixer.w -> TF variable
MIXER = {"w1": "hyper_w_1", "w_final": "hyper_w_final", "b1": "hyper_b_1", "b_final_l1": "hyper_b_final_l1/kernel",
         "b_final": "hyper_b_final/kernel"}
NAMES = AGENT + tuple(MIXER)
EMBED = MR.EMBED


def case(N, B, seed):
    """(agent weights, mixer weights, columns of the batch as torch tensors, td [B] float64)"""
    rng = np.random.default_rng(seed)
    wa = QR.init_weights(rng, N)
    wm = MR.init_weights(rng, N, scale=0.5)
    cols = CF.make_cols(B, N, seed=seed)
    td = rng.uniform(-5, 5, B)
    return wa, wm, cols, td


def short_weights(wa, wm):
    """the eleven tensors under the short names of a learner's grads"""
    w = {QR.canon(k): np.asarray(v) for k, v in wa.items()}
    m = {MR.canon(k): np.asarray(v) for k, v in wm.items()}
    w.update({short: m[name] for short, name in MIXER.items()})
    return w


def arrays(cols):
    """(x [B N, L + 6], actions [B N], xm [B, 6 N]) float64 / int64 from the columns"""
    g = lambda k: cols[k].detach().cpu().numpy() if hasattr(cols[k], "detach") else np.asarray(cols[k])      # noqa: E731
    vg = g("v_global")
    B, N = vg.shape[0], vg.shape[1]
    x = np.concatenate([g("obs_others").reshape(B * N, -1), g("v_local").reshape(B * N, 4), g("goals").reshape(B * N, 2)], axis=1)
    xm = np.concatenate([vg.reshape(B, -1), g("goals").reshape(B, -1)], axis=1)
    return x.astype(np.float64), g("actions").reshape(-1).astype(np.int64), xm.astype(np.float64)


def loss_and_grads(w, cols, td, dtype=np.float64, check_margin=True):
    """{"loss": scalar, "q_tot": [B], "q_sel": [B, N], "grads": {short name: array}, "margin": float} of the eleven tensors `w` (short
    names) on the batch, every operation in `dtype`."""
    f = np.dtype(dtype).type
    W = {k: np.asarray(v, dtype=f) for k, v in w.items()}
    x, act, xm = arrays(cols)
    x, xm = x.astype(f), xm.astype(f)
    B, R = xm.shape[0], x.shape[0]
    N = R // B
    # ---- forward ----
    z1 = x @ W["h/kernel"] + W["h/bias"]
    h1 = np.maximum(z1, f(0))
    z2 = h1 @ W["h2/kernel"] + W["h2/bias"]
    h2 = np.maximum(z2, f(0))
    Q = h2 @ W["out/kernel"] + W["out/bias"]
    q = Q[np.arange(R), act].reshape(B, N)
    z_l1 = xm @ W["b_final_l1"]
    l1 = np.maximum(z_l1, f(0))
    z_w1 = (xm @ W["w1"]).reshape(B, N, EMBED)
    w1 = np.abs(z_w1)
    z_wf = xm @ W["w_final"]
    wf = np.abs(z_wf)
    h = np.einsum("bn,bne->be", q, w1) + xm @ W["b1"]
    hidden = np.where(h > 0, h, np.expm1(np.minimum(h, f(0))))
    q_tot = np.sum(hidden * wf, axis=1) + (l1 @ W["b_final"])[:, 0]
    td32 = np.asarray(td, np.float64).astype(np.float32).astype(f)
    loss = np.mean((td32 - q_tot) ** 2)
    margin = min(float(np.abs(a).min()) for a in (z1, z2, z_w1, z_wf, z_l1))
    if check_margin:
        assert margin >= MARGIN, "a pre-activation is %.3g from a kink: not a parity case" % margin
    # ---- backward ----
    dq = (f(2) * (q_tot - td32) / f(B))[:, None]
    G = {}
    G["b_final"] = l1.T @ dq
    G["b_final_l1"] = xm.T @ (dq * W["b_final"][:, 0][None, :] * (z_l1 > 0))
    G["w_final"] = xm.T @ (dq * hidden * np.sign(z_wf))
    dh = dq * wf * np.where(h > 0, f(1), hidden + f(1))
    G["b1"] = xm.T @ dh
    G["w1"] = xm.T @ (dh[:, None, :] * q[:, :, None] * np.sign(z_w1)).reshape(B, N * EMBED)
    dqsel = np.einsum("be,bne->bn", dh, w1).reshape(R)
    dQ = np.zeros_like(Q)
    dQ[np.arange(R), act] = dqsel
    G["out/kernel"], G["out/bias"] = h2.T @ dQ, dQ.sum(axis=0)
    d2 = (dQ @ W["out/kernel"].T) * (z2 > 0)
    G["h2/kernel"], G["h2/bias"] = h1.T @ d2, d2.sum(axis=0)
    d1 = (d2 @ W["h2/kernel"].T) * (z1 > 0)
    G["h/kernel"], G["h/bias"] = x.T @ d1, d1.sum(axis=0)
    return {"loss": loss, "q_tot": q_tot, "q_sel": q, "grads": {k: G[k] for k in NAMES}, "margin": margin}


def adam_state(w, beta1=0.9, beta2=0.999, dtype=np.float64):
    """(m, v, powers) as tf.train.AdamOptimizer creates them: zeros, and beta1_power / beta2_power at beta1 / beta2"""
    f = np.dtype(dtype).type
    zeros = lambda: {k: np.zeros(np.shape(v), dtype=f) for k, v in w.items()}      # noqa: E731
    return zeros(), zeros(), np.array([beta1, beta2], dtype=f)


def adam_step(w, g, m, v, powers, lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, dtype=np.float64):
    """One step on every tensor; returns (w, m, v, powers) new, in `dtype` (every product and sum an operation of its own)."""
    f = np.dtype(dtype).type
    lr, beta1, beta2, epsilon = f(lr), f(beta1), f(beta2), f(epsilon)
    p = np.asarray(powers, dtype=f)
    lr_t = lr * np.sqrt(f(1) - p[1]) / (f(1) - p[0])
    W, M, V = {}, {}, {}
    for k in w:
        gk = np.asarray(g[k], dtype=f)
        M[k] = beta1 * np.asarray(m[k], dtype=f) + (f(1) - beta1) * gk
        V[k] = beta2 * np.asarray(v[k], dtype=f) + (f(1) - beta2) * (gk * gk)
        W[k] = np.asarray(w[k], dtype=f) - (lr_t * M[k]) / (np.sqrt(V[k]) + epsilon)
    return W, M, V, np.array([p[0] * beta1, p[1] * beta2], dtype=f)


def trajectory(w, cols, td, steps, lr=1e-3, dtype=np.float64):
    """the losses of `steps` Adam steps on one fixed batch (no margin condition: the loss is continuous across the kinks)"""
    m, v, p = adam_state(w, dtype=dtype)
    losses = []
    for _ in range(steps):
        out = loss_and_grads(w, cols, td, dtype=dtype, check_margin=False)
        losses.append(float(out["loss"]))
        w, m, v, p = adam_step(w, out["grads"], m, v, p, lr=lr, dtype=dtype)
    return losses
