"""CPU: tests/qmix_learner_checkers_ref.py -- the hand-written backward pass of the Checkers QMIX learner -- against torch autograd in
float64 on the same inputs, its forward pass against the two restatements the device networks are held to, the kink margin of the
parity cases against the float32 forward deviation measured here, and the float32 restatement's share of the project's bound.

Shares of the bound 2e-5 max(1, max|ref|) used by torch autograd in float32 against float64, measured on this CPU over CASES: at most
0.053 of a gradient's (hyper_w_1 at (1, 1, 1)); of the five-step trajectory's (the float32 NumPy restatement against float64) at most 0.390 ((2, 3, 0)), printed by the tests."""
import numpy as np
import pytest
import torch

from tests import critic_feeds as CF
from tests import qmix_checkers_ref as QC
from tests import qmix_learner_checkers_ref as LR
from tests import qmix_mixer_checkers_ref as MC


def _autograd(w, cols, td, dtype=torch.float64):
    """loss, q_tot and gradients by torch autograd in `dtype` (conv2d, relu, abs, elu of torch: relu's gradient at 0 is 0 and abs's is
    sign(0) = 0, TensorFlow's conventions)"""
    c = LR.arrays(cols)
    B, N = c["B"], c["N"]
    R = B * N
    t = lambda a: torch.tensor(np.asarray(a, np.float64)).to(dtype)      # noqa: E731
    W = {k: t(v).requires_grad_(True) for k, v in w.items()}
    A = lambda k: W["agent/" + k]      # noqa: E731
    M = lambda k: W["mixer/" + k]      # noqa: E731
    F = torch.nn.functional
    conv = torch.relu(F.conv2d(t(c["win"]).permute(0, 3, 1, 2), A("conv_w").permute(3, 2, 0, 1), A("conv_b"), padding=1))
    c1 = conv.permute(0, 2, 3, 1).reshape(R, 150)
    lin = torch.relu(c1 @ A("lin_w") + A("lin_b"))
    xs = torch.cat([lin, t(c["sv"]), F.one_hot(torch.tensor(c["ap"]), 5).to(dtype), t(c["goal"])], dim=1)
    hs = torch.relu(xs @ A("self_w") + A("self_b"))
    ho = torch.relu(t(c["oth"]) @ A("others_w") + A("others_b"))
    h2 = torch.relu(hs @ A("w_self_h2") + ho @ A("w_others_h2") + A("b_h2"))
    Q = h2 @ A("out_w") + A("out_b")
    q = (Q * F.one_hot(torch.tensor(c["act"]), 5)).sum(dim=1).reshape(B, 1, N)
    cm = torch.relu(F.conv2d(t(c["grid"]).permute(0, 3, 1, 2), M("conv_w").permute(3, 2, 0, 1), M("conv_b"), padding=(1, 2)))
    xm = torch.cat([cm.permute(0, 2, 3, 1).reshape(B, 108), t(c["vec"]), t(c["goal"]).reshape(B, 2 * N)], dim=1)
    l1 = torch.relu(xm @ M("hyper_b_final_l1"))
    w1 = torch.abs(xm @ M("hyper_w_1")).reshape(B, N, LR.EMBED)
    hidden = F.elu(q @ w1 + (xm @ M("hyper_b_1")).reshape(B, 1, LR.EMBED))
    q_tot = (hidden @ torch.abs(xm @ M("hyper_w_final")).reshape(B, LR.EMBED, 1) + (l1 @ M("hyper_b_final")).reshape(B, 1, 1)).reshape(B)
    td32 = torch.tensor(np.asarray(td, np.float64).astype(np.float32)).to(dtype)
    loss = torch.mean((td32 - q_tot) ** 2)
    loss.backward()
    return float(loss.detach()), q_tot.detach().numpy().astype(np.float64), {k: W[k].grad.numpy().astype(np.float64) for k in W}


def _check_against_autograd(w, cols, td, got):
    loss, q_tot, grads = _autograd(w, cols, td)
    assert abs(got["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.allclose(got["q_tot"], q_tot, rtol=1e-12, atol=1e-12)
    assert sorted(grads) == sorted(LR.NAMES) and len(LR.NAMES) == 20
    for k in LR.NAMES:
        assert got["grads"][k].shape == np.shape(w[k]), k
        scale = max(1.0, float(np.abs(grads[k]).max()))
        assert float(np.abs(got["grads"][k] - grads[k]).max()) <= 1e-10 * scale, k


@pytest.mark.parametrize("N,B,seed", LR.CASES)
def test_hand_written_backward_is_autograd_in_float64(N, B, seed):
    wa, wm, cols, td, w, got = LR.cached_case(N, B, seed)                  # (loss_and_grads asserted the margin)
    assert got["margin"] >= LR.MARGIN
    _check_against_autograd(w, cols, td, got)
    # the forward pass is the two restatements the device networks are held to
    c = LR.arrays(cols)
    Q = QC.q_values(wa, c["ap"], c["win"], c["sv"], c["oth"], c["goal"])
    q_sel = Q[np.arange(B * N), c["act"]].reshape(B, N)
    assert np.allclose(got["q_sel"], q_sel, rtol=1e-12, atol=1e-12)
    ref = MC.q_tot(wm, got["q_sel"], c["grid"], c["vec"], c["goal"].reshape(B, 2 * N)).reshape(-1)
    assert np.allclose(got["q_tot"], ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("N,B,seed", LR.CASES)
def test_margin_is_ten_times_the_float32_forward_deviation(N, B, seed):
    _, _, cols, td, w, ref = LR.cached_case(N, B, seed)
    f32 = LR.loss_and_grads(w, cols, td, dtype=np.float32, check_margin=False)
    dev = max(float(np.abs(np.asarray(f32["pre"][k], np.float64) - ref["pre"][k]).max()) for k in ref["pre"])
    print("N=%d B=%d seed=%d: margin %.3g, float32 forward deviation %.3g" % (N, B, seed, ref["margin"], dev))
    assert LR.MARGIN >= 10 * dev


@pytest.mark.parametrize("N,B,seed", LR.CASES)
def test_float32_restatement_stays_far_inside_the_bound(N, B, seed):
    _, _, cols, td, w, ref = LR.cached_case(N, B, seed)
    loss32, _, g32 = _autograd(w, cols, td, dtype=torch.float32)
    worst = ("loss", abs(loss32 - ref["loss"]) / (CF.BOUND * max(1.0, abs(ref["loss"]))))
    for k in LR.NAMES:
        share = float(np.abs(g32[k] - ref["grads"][k]).max()) / (CF.BOUND * max(1.0, float(np.abs(ref["grads"][k]).max())))
        worst = max(worst, (k, share), key=lambda kv: kv[1])
    print("N=%d B=%d: largest share of the bound used by float32 autograd %.3f (%s)" % (N, B, worst[1], worst[0]))
    assert worst[1] <= 0.25, worst
    # five Adam steps on the fixed batch: half the bound at the most is the restatement's
    a, b = LR.trajectory(w, cols, td, 5, dtype=np.float32), LR.trajectory(w, cols, td, 5)
    used = max(abs(x - y) / (CF.BOUND * max(1.0, abs(y))) for x, y in zip(a, b))
    print("five losses N=%d B=%d: share of the bound used by the float32 restatement %.3f" % (N, B, used))
    assert used <= 0.5


def test_the_kink_case_has_exact_zeros_and_tells_the_conventions_apart():
    wa, wm, cols, td = LR.kink_case()
    w = LR.short_weights(wa, wm)
    got = LR.loss_and_grads(w, cols, td)                                   # the margin holds over what is not exactly zero
    assert int((got["pre"]["conv"][0] == 0).sum()) == 150 and int((got["pre"]["mixer_conv"][0] == 0).sum()) == 108
    _check_against_autograd(w, cols, td, got)
    other = LR.loss_and_grads(w, cols, td, pass_at_zero=True)
    for k in ("agent/conv_b", "mixer/conv_b"):                             # ">= 0" is far outside the bound of "> 0"
        bound = CF.BOUND * max(1.0, float(np.abs(got["grads"][k]).max()))
        assert float(np.abs(other["grads"][k] - got["grads"][k]).max()) > 1000 * bound, k


def test_a_case_on_a_kink_is_refused():
    wa, wm, cols, td = LR.case(2, 3, 0)
    w = LR.short_weights(wa, wm)
    pre = LR.loss_and_grads(w, cols, td)["pre"]["branch_self"]
    w["agent/self_b"] = w["agent/self_b"].copy()
    w["agent/self_b"][0] -= np.float32(pre[0, 0])                          # unit 0 of row 0 at ~0
    with pytest.raises(AssertionError, match="not a parity case"):
        LR.loss_and_grads(w, cols, td)
