"""CPU: the restatement of the Checkers baseline critics (tests/baseline_checkers_ref.py) against the golden vectors recorded by
executing the reference's own networks.V_checkers_local / V_checkers_global / Q_coma_checkers (tools/gen_golden_baseline_checkers.py
-> tests/golden/baseline_checkers_<case>.npz), the fixtures' weight names and shapes against the ones the device networks map, the
fixtures' rows as decodings of base columns, and how much of the GPU tests' bound float32 arithmetic alone uses on their cases."""
import os

import numpy as np
import pytest

from tests import baseline_checkers_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("tag", BR.CASES)
def test_restatement_reproduces_the_recorded_outputs(tag):
    """the tolerances of tests/test_critic_checkers_oracle.py for shim fixtures: float32 within 1e-6 relative, float64 within 1e-5"""
    w, x, out = BR.load_case(GOLDEN, tag)
    kind, n = tag.split("_n")[0], int(tag.split("_n")[1])
    assert 48 <= out.shape[0] <= 64 and out.dtype == np.float32 and out.shape[1] == (5 if kind == "coma" else 1)
    assert len(w) == (10 if (kind == "coma" or n > 1) else 7)
    for name in ("state_env", "obs_self_t"):
        if name in x:
            assert set(np.unique(x[name])) <= ({0.0, 1.0} if name == "state_env" else {-1.0, 0.0, 1.0})
    got = BR.eval_case(tag, w, x, np.float32)
    assert got.dtype == np.float32 and got.shape == out.shape
    err = np.abs(got - out) / np.maximum(1.0, np.abs(out))
    print(tag, "max relative error", float(err.max()), "max |out|", float(np.abs(out).max()))
    assert err.max() <= 1e-6
    assert np.abs(BR.eval_case(tag, w, x, np.float64) - out).max() < 1e-5


@pytest.mark.parametrize("tag", BR.CASES)
def test_fixture_weights_are_the_ones_the_device_networks_map(tag):
    from cm3_amd import baseline
    w, _, _ = BR.load_case(GOLDEN, tag)
    kind, n = tag.split("_n")[0], int(tag.split("_n")[1])
    if kind == "coma":
        names, shapes, scope = baseline.CK_COMA_NAMES, baseline.checkers_coma_weight_shapes(n), "Q_main/"
        mine = BR.init_coma_weights(np.random.default_rng(0), n, scope="Q_main")
    else:
        names, shapes, scope = baseline.CK_VALUE_NAMES[kind], baseline.checkers_value_weight_shapes(n, kind, 1 if n == 1 else 2), "V_main/"
        mine = BR.init_value_weights(np.random.default_rng(0), n, kind, scope="V_main")
    assert sorted(w) == sorted(scope + names[s] for s in shapes) == sorted(mine)
    for short, shape in shapes.items():
        assert w[scope + names[short]].shape == shape == mine[scope + names[short]].shape, short
    assert sorted(BR.canon(k) for k in w) == sorted(names[s] for s in shapes)
    assert (baseline.CK_H1_1, baseline.CK_H1_2, baseline.CK_H2, baseline.Q_UNITS) == (BR.H1_1, BR.H1_2, BR.H2, BR.UNITS)


@pytest.mark.parametrize("tag", BR.CASES)
def test_fixture_rows_are_decodings_of_base_columns(tag):
    """Tiling the base columns as the reference's train_step does and picking the fixture's rows gives the fixture's inputs back."""
    import torch
    from cm3_amd import batch as BT
    _, x, _ = BR.load_case(GOLDEN, tag)
    kind, N = tag.split("_n")[0], int(tag.split("_n")[1])
    c, pick = BR.fixture_base_columns(tag, x)
    R = x["v_goal"].shape[0]
    assert len(set(pick.tolist())) == R and pick.max() < R * N
    t = {k: torch.as_tensor(v) for k, v in c.items()}
    rows = lambda a: a.reshape(R * N, *a.shape[2:])[pick].numpy()      # noqa: E731
    goals_self, goals_others = BT.process_goals(t["goals"])
    one, others, state = BT.process_global_state(t["vec"])
    assert np.array_equal(goals_self[pick].numpy(), x["v_goal"])
    if kind == "local":
        assert np.array_equal(rows(t["obs_self_t"]), x["obs_self_t"]) and np.array_equal(rows(t["obs_self_v"]).astype(np.float32), x["obs_self_v"])
        if N > 1:
            assert np.array_equal(rows(t["obs_others"]).astype(np.float32), x["obs_others"])
    elif kind == "global":
        assert np.array_equal(BT.rep_rows(t["grid"], N)[pick].numpy(), x["state_env"])
        assert np.array_equal(one[pick].numpy().astype(np.float32), x["v_state_one_agent"])
        assert np.array_equal(others[pick].numpy().astype(np.float32), x["v_state_other_agents"])
    else:
        assert np.array_equal(BT.rep_rows(t["grid"], N)[pick].numpy(), x["state_env"])
        assert np.array_equal(state[pick].numpy().astype(np.float32), x["v_state"])
        assert np.array_equal(goals_others[pick].numpy(), x["v_goal_others"])
        assert np.array_equal(BT.process_actions(t["actions"])[1][pick].numpy(), x["action_others"])
        assert np.array_equal(rows(t["obs_self_t"]), x["obs_self_t"]) and np.array_equal(rows(t["obs_self_v"]).astype(np.float32), x["obs_self_v"])


def test_fixture_files_stay_under_the_size_limit():
    for tag in BR.CASES:
        assert os.path.getsize(os.path.join(GOLDEN, "baseline_checkers_%s.npz" % tag)) < 900 * 1024, tag


def test_float32_restatement_uses_at_most_half_the_bound_on_the_gpu_cases():
    """The GPU tests hold the kernels to 2e-5 * max(1, |ref|) against float64 on these cases; float32 arithmetic alone (NumPy's order)
    must leave at least half of that, and |ref| must reach several units so that the relative part of the bound is live."""
    from tests import baseline_checkers_feeds as BF
    worst, largest = {}, {}
    for N in BF.VALUE_AGENTS:
        for B in BF.BATCHES:
            r64, r32 = BF.refs(N, B, np.float64), BF.refs(N, B, np.float32)
            for op in r64:
                net = "coma" if op.startswith("Q") else op
                used = np.abs(r32[op].astype(np.float64) - r64[op]) / (BF.BOUND * np.maximum(1.0, np.abs(r64[op])))
                worst[net] = max(worst.get(net, 0.0), float(used.max()))
                largest[net] = max(largest.get(net, 0.0), float(np.abs(r64[op]).max()))
    for net in ("local", "global", "coma"):
        print("float32 restatement, %s: share of the bound used %.3f, max |ref| %.2f" % (net, worst[net], largest[net]))
        assert worst[net] <= 0.5 and largest[net] >= 3.0, net
