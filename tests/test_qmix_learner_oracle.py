"""CPU: tests/qmix_learner_ref.py -- the hand-written backward pass of the particle QMIX learner -- against torch autograd in float64
on the same inputs, the kink margin of the parity cases, the float32 restatement's share of the project's bound, and the Adam
restatement against a two-step example worked out with scalars."""
import math

import numpy as np
import pytest
import torch

from tests import critic_feeds as CF
from tests import qmix_learner_ref as LR


def _autograd(w, cols, td):
    """loss and gradients by torch autograd in float64 (relu, abs, elu of torch: the same conventions away from the kinks)"""
    x, act, xm = LR.arrays(cols)
    W = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in w.items()}
    x, xm, act = torch.tensor(x), torch.tensor(xm), torch.tensor(act)
    B, R = xm.shape[0], x.shape[0]
    N = R // B
    h1 = torch.relu(x @ W["h/kernel"] + W["h/bias"])
    h2 = torch.relu(h1 @ W["h2/kernel"] + W["h2/bias"])
    Q = h2 @ W["out/kernel"] + W["out/bias"]
    q = (Q * torch.nn.functional.one_hot(act, 5)).sum(dim=1).reshape(B, 1, N)
    l1 = torch.relu(xm @ W["b_final_l1"])
    w1 = torch.abs(xm @ W["w1"]).reshape(B, N, LR.EMBED)
    hidden = torch.nn.functional.elu(q @ w1 + (xm @ W["b1"]).reshape(B, 1, LR.EMBED))
    q_tot = (hidden @ torch.abs(xm @ W["w_final"]).reshape(B, LR.EMBED, 1) + (l1 @ W["b_final"]).reshape(B, 1, 1)).reshape(B)
    td32 = torch.tensor(np.asarray(td, np.float64).astype(np.float32).astype(np.float64))
    loss = torch.mean((td32 - q_tot) ** 2)
    loss.backward()
    return float(loss.detach()), q_tot.detach().numpy(), {k: W[k].grad.numpy() for k in W}


@pytest.mark.parametrize("N,B,seed", LR.CASES)
def test_hand_written_backward_is_autograd_in_float64(N, B, seed):
    wa, wm, cols, td = LR.case(N, B, seed)
    w = LR.short_weights(wa, wm)
    got = LR.loss_and_grads(w, cols, td)                       # asserts the margin
    assert got["margin"] >= LR.MARGIN
    loss, q_tot, grads = _autograd(w, cols, td)
    assert abs(got["loss"] - loss) <= 1e-13 * max(1.0, abs(loss))
    assert np.allclose(got["q_tot"], q_tot, rtol=1e-13, atol=1e-13)
    assert sorted(grads) == sorted(LR.NAMES)
    for k in LR.NAMES:
        assert got["grads"][k].shape == np.shape(w[k]), k
        scale = max(1.0, float(np.abs(grads[k]).max()))
        assert float(np.abs(got["grads"][k] - grads[k]).max()) <= 1e-12 * scale, k
    # q_tot is the mixer's restatement on the selected Q values
    from tests import qmix_mixer_ref as MR
    x, _, xm = LR.arrays(cols)
    ref = MR.q_tot(wm, got["q_sel"], xm[:, :4 * N], xm[:, 4 * N:], dtype=np.float64).reshape(-1)
    assert np.allclose(got["q_tot"], ref, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("N,B,seed", LR.CASES)
def test_float32_restatement_stays_far_inside_the_bound(N, B, seed):
    wa, wm, cols, td = LR.case(N, B, seed)
    w = LR.short_weights(wa, wm)
    ref = LR.loss_and_grads(w, cols, td)
    f32 = LR.loss_and_grads(w, cols, td, dtype=np.float32, check_margin=False)
    for k in LR.NAMES:
        scale = CF.BOUND * max(1.0, float(np.abs(ref["grads"][k]).max()))
        assert float(np.abs(f32["grads"][k] - ref["grads"][k]).max()) <= 0.1 * scale, k
    assert abs(float(f32["loss"]) - ref["loss"]) <= 0.1 * CF.BOUND * max(1.0, abs(ref["loss"]))
    # five Adam steps on the fixed batch: the whole bound (Adam divides by sqrt(v), so the steps amplify rounding where the gradient
    # is small; the float32 restatement uses 0.04 .. 0.83 of it over the cases, the most at N = 1, B = 1 where the loss falls to 0.075)
    a, b = LR.trajectory(w, cols, td, 5, dtype=np.float32), LR.trajectory(w, cols, td, 5)
    used = max(abs(x - y) / (CF.BOUND * max(1.0, abs(y))) for x, y in zip(a, b))
    print("five losses N=%d B=%d: share of the bound used by the float32 restatement %.3f" % (N, B, used))
    assert used <= 1.0


def test_a_case_on_a_kink_is_refused():
    wa, wm, cols, td = LR.case(2, 3, 1)
    w = LR.short_weights(wa, wm)
    w["h/bias"] = w["h/bias"].copy()
    x, _, _ = LR.arrays(cols)
    w["h/bias"][0] -= np.float32((x @ w["h/kernel"].astype(np.float64) + w["h/bias"])[0, 0])      # unit 0 of row 0 at ~0
    with pytest.raises(AssertionError, match="not a parity case"):
        LR.loss_and_grads(w, cols, td)


def test_adam_is_tensorflows_two_steps_by_hand():
    lr, b1, b2, eps = 0.1, 0.9, 0.999, 1e-8
    var, g1, g2 = 1.0, 0.5, -0.25
    # step 1: powers beta1, beta2
    lr_t = lr * math.sqrt(1 - b2) / (1 - b1)
    m1 = (1 - b1) * g1
    v1 = (1 - b2) * g1 * g1
    var1 = var - lr_t * m1 / (math.sqrt(v1) + eps)
    assert abs(var1 - 0.9) < 1e-6                               # the first Adam step moves by lr against the gradient's sign
    # step 2: powers beta1^2, beta2^2
    lr_t2 = lr * math.sqrt(1 - b2 * b2) / (1 - b1 * b1)
    m2 = b1 * m1 + (1 - b1) * g2
    v2 = b2 * v1 + (1 - b2) * g2 * g2
    var2 = var1 - lr_t2 * m2 / (math.sqrt(v2) + eps)
    w = {"x": np.array([var, var])}
    m, v, p = LR.adam_state(w, b1, b2)
    assert np.array_equal(p, [b1, b2]) and not m["x"].any() and not v["x"].any()
    w, m, v, p = LR.adam_step(w, {"x": np.array([g1, 0.0])}, m, v, p, lr=lr, beta1=b1, beta2=b2, epsilon=eps)
    assert np.allclose(w["x"], [var1, var], rtol=1e-15, atol=0) and np.allclose(p, [b1 * b1, b2 * b2], rtol=1e-15)
    assert np.allclose(m["x"], [m1, 0.0], rtol=1e-15) and np.allclose(v["x"], [v1, 0.0], rtol=1e-15)
    w, m, v, p = LR.adam_step(w, {"x": np.array([g2, 0.0])}, m, v, p, lr=lr, beta1=b1, beta2=b2, epsilon=eps)
    assert np.allclose(w["x"], [var2, var], rtol=1e-15, atol=0) and np.allclose(p, [b1 ** 3, b2 ** 3], rtol=1e-15)
    assert np.allclose(m["x"], [m2, 0.0], rtol=1e-15) and np.allclose(v["x"], [v2, 0.0], rtol=1e-15)
    # epsilon sits OUTSIDE the bias correction: torch.optim.Adam's formula gives another number when v is tiny
    tiny = {"x": np.array([1.0])}
    m, v, p = LR.adam_state(tiny, b1, b2)
    w_tf, _, _, _ = LR.adam_step(tiny, {"x": np.array([1e-9])}, m, v, p, lr=lr, beta1=b1, beta2=b2, epsilon=eps)
    t = torch.nn.Parameter(torch.tensor([1.0], dtype=torch.float64))
    opt = torch.optim.Adam([t], lr=lr, betas=(b1, b2), eps=eps)
    t.grad = torch.tensor([1e-9], dtype=torch.float64)
    opt.step()
    assert abs(float(w_tf["x"][0]) - float(t.detach()[0])) > 1e-3
