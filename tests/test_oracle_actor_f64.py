"""CPU: the float64 path of the actor oracles (actor_probs(..., dtype=np.float64)), the reference the device actors are measured
against in tests/test_gpu_actor_f64.py and tests/test_gpu_actor_checkers_f64.py.  It must agree with the float32 path within the
parity budget on the golden rows and on random rows, agree with an independent PyTorch float64 evaluation of the same graph to
float64 rounding, and leave the float32 default -- pinned by the golden vectors -- as it was."""
import numpy as np
import pytest
import torch

from oracle import actor_checkers_oracle as CO
from oracle import actor_oracle as PO
from tests.test_oracle_actor_golden import load_cases


def _particle_torch64(w, oo, vo, vg):
    T = lambda k: torch.as_tensor(w[k], dtype=torch.float64)  # noqa: E731
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
    acc = torch.relu(torch.cat([d(vo), d(vg)], 1) @ T("actor_branch_self/kernel") + T("actor_branch_self/bias")) @ T("W_branch_self_h2")
    if "stage-2/W_others_h2" in w:
        acc = acc + torch.relu(d(oo) @ T("stage-2/actor_others/kernel") + T("stage-2/actor_others/bias")) @ T("stage-2/W_others_h2")
    return torch.softmax(torch.relu(acc + T("b")) @ T("actor_out/kernel") + T("actor_out/bias"), dim=1).numpy()


def _checkers_torch64(w, a_prev, t, v, oo, g):
    T = lambda k: torch.as_tensor(w[k], dtype=torch.float64)  # noqa: E731
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
    x = d(t).permute(0, 3, 1, 2)
    conv = torch.relu(torch.nn.functional.conv2d(x, T("conv/Conv/weights").permute(3, 2, 0, 1), T("conv/Conv/biases"), padding=1))
    lin = torch.relu(conv.permute(0, 2, 3, 1).reshape(x.shape[0], -1) @ T("conv_linear/kernel") + T("conv_linear/bias"))
    a1 = torch.nn.functional.one_hot(torch.as_tensor(np.asarray(a_prev)).long(), 5).double()
    acc = torch.relu(torch.cat([lin, d(v), a1, d(g)], 1) @ T("branch_self/kernel") + T("branch_self/bias")) @ T("W_self_h2")
    if "stage-2/W_others_h2" in w:
        acc = acc + torch.relu(d(oo) @ T("stage-2/branch_others/kernel") + T("stage-2/branch_others/bias")) @ T("stage-2/W_others_h2")
    return torch.softmax(torch.relu(acc + T("b")) @ T("actor_out/kernel") + T("actor_out/bias"), dim=1).numpy()


def _particle_rows(rng, rows, N):
    L = 4 * max(N - 1, 1)
    return (rng.uniform(-2, 2, (rows, L)).astype(np.float32), rng.uniform(-1.5, 1.5, (rows, 4)).astype(np.float32),
            rng.uniform(-1, 1, (rows, 2)).astype(np.float32))


def _checkers_rows(rng, rows, N):
    return (rng.integers(0, 5, rows), rng.integers(-1, 2, (rows, 5, 5, 3)).astype(np.float64), rng.uniform(-0.5, 1.0, (rows, 4)),
            rng.uniform(-0.5, 0.5, (rows, 2 * max(N - 1, 1))), np.eye(2)[rng.integers(0, 2, rows)])


@pytest.mark.parametrize("tag", ["n1_stage1", "n4_stage2", "n8_stage2"])
def test_particle_golden_rows_in_float64(tag):
    w, inp, probs = load_cases("actor_particle")[tag]
    args = (inp["obs_others"], inp["v_obs"], inp["v_goal"])
    p32, p64 = PO.actor_probs(w, *args), PO.actor_probs(w, *args, dtype=np.float64)
    assert p32.dtype == np.float32 and p64.dtype == np.float64
    assert np.abs(p32 - probs).max() < 1e-6                       # the float32 default still reproduces the golden vectors
    assert np.abs(p64 - probs).max() < 2e-5 and np.abs(p64 - p32).max() < 2e-5
    assert np.abs(p64 - _particle_torch64(w, *args)).max() < 1e-12


@pytest.mark.parametrize("tag", ["n1_stage1", "n2_stage2"])
def test_checkers_golden_rows_in_float64(tag):
    w, inp, probs = load_cases("actor_checkers")[tag]
    args = (inp["a_prev"], inp["obs_self_t"], inp["obs_self_v"], inp["obs_others"], inp["goals"])
    p32, p64 = CO.actor_probs(w, *args), CO.actor_probs(w, *args, dtype=np.float64)
    assert p32.dtype == np.float32 and p64.dtype == np.float64
    assert np.abs(p32 - probs).max() < 1e-6
    assert np.abs(p64 - probs).max() < 2e-5 and np.abs(p64 - p32).max() < 2e-5
    assert np.abs(p64 - _checkers_torch64(w, *args)).max() < 1e-12


@pytest.mark.parametrize("N", range(1, 11))
def test_particle_random_rows_float32_against_float64(N):
    """Every agent count the device actor accepts, at the test weight scale: the float32 oracle's own rounding stays well inside
    the 2e-5 parity budget (a few 1e-6, growing with the others input width), and the float64 path really is another evaluation."""
    rng = np.random.default_rng(40 + N)
    stage = 1 if N == 1 else 2
    w = PO.init_weights(rng, N, stage=stage)
    args = _particle_rows(rng, 4096, N)
    p32, p64 = PO.actor_probs(w, *args), PO.actor_probs(w, *args, dtype=np.float64)
    d = np.abs(p32 - p64).max()
    assert 0 < d < 2e-5, d
    assert np.abs(p64.sum(1) - 1).max() < 1e-12
    assert np.ptp(p64, axis=1).mean() > 0.05                      # the random policy is not uniform
    assert np.abs(p64[:256] - _particle_torch64(w, *(a[:256] for a in args))).max() < 1e-12


@pytest.mark.parametrize("N", range(1, 9))
def test_checkers_random_rows_float32_against_float64(N):
    rng = np.random.default_rng(60 + N)
    stage = 1 if N == 1 else 2
    w = CO.init_weights(rng, N, stage=stage)
    args = _checkers_rows(rng, 2048, N)
    p32, p64 = CO.actor_probs(w, *args), CO.actor_probs(w, *args, dtype=np.float64)
    d = np.abs(p32 - p64).max()
    assert 0 < d < 2e-5, d
    assert np.abs(p64.sum(1) - 1).max() < 1e-12
    assert np.abs(p64[:256] - _checkers_torch64(w, *(a[:256] for a in args))).max() < 1e-12


def test_conv_in_float64_is_the_float32_conv_without_its_rounding():
    rng = np.random.default_rng(3)
    x = rng.integers(-1, 2, (64, 5, 5, 3)).astype(np.float32)
    w = rng.standard_normal((3, 3, 3, 6)).astype(np.float32)
    b = rng.standard_normal(6).astype(np.float32)
    c32, c64 = CO.conv_same_3x3(x, w, b), CO.conv_same_3x3(x, w, b, dtype=np.float64)
    assert c32.dtype == np.float32 and c64.dtype == np.float64
    want = torch.nn.functional.conv2d(torch.as_tensor(x, dtype=torch.float64).permute(0, 3, 1, 2),
                                      torch.as_tensor(w, dtype=torch.float64).permute(3, 2, 0, 1),
                                      torch.as_tensor(b, dtype=torch.float64), padding=1).permute(0, 2, 3, 1).numpy()
    assert np.abs(c64 - want).max() < 1e-12
    assert np.abs(c32 - c64).max() < 1e-5
