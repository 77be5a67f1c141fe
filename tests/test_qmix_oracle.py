"""CPU: the float64 restatement of the QMIX agent network (tests/qmix_ref.py) against the golden vectors recorded by executing the
reference's own networks.Qmix_single_particle (tools/gen_golden_qmix.py -> tests/golden/qmix_particle.npz), and the fixture's
weight names against the ones the device agent maps."""
import os

import numpy as np
import pytest

from tests import qmix_ref as QR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qmix_particle.npz")
CASES = [1, 4, 8, 10]


def _case(n):
    z = np.load(GOLDEN)
    tag = "n%d" % n
    w = {str(k): z[tag + "/w/" + str(k)] for k in z[tag + "/names"]}
    inputs = {k: z[tag + "/in/" + k] for k in ("obs_others", "v_obs", "v_goal")}
    return w, inputs, z[tag + "/q"], z[tag + "/argmax"]


@pytest.mark.parametrize("n", CASES)
def test_float64_restatement_reproduces_the_reference_network(n):
    w, x, q, amax = _case(n)
    got = QR.q_values(w, x["obs_others"], x["v_obs"], x["v_goal"])
    assert got.shape == q.shape == (x["v_obs"].shape[0], 5)
    assert np.abs(got - q).max() < 1e-6
    assert np.array_equal(np.argmax(got, axis=1), amax)
    assert len(set(amax.tolist())) > 1                     # the fixture exercises more than one greedy action


@pytest.mark.parametrize("n", CASES)
def test_fixture_weights_are_the_six_the_agent_maps(n):
    from cm3_amd import qmix
    w, x, _, _ = _case(n)
    assert sorted(w) == sorted("Agent_main/" + k for k in qmix.NAMES)
    assert sorted(qmix._canon(k) for k in w) == sorted(qmix.NAMES) == sorted(QR.NAMES)
    L = 4 * max(n - 1, 1)
    assert w["Agent_main/h/kernel"].shape == (L + 6, 64) and x["obs_others"].shape[1] == L
    assert w["Agent_main/out/kernel"].shape == (64, 5)
    assert qmix._canon("Agent_target/h2/bias:0") == "h2/bias"


def test_exploration_stream_is_its_own():
    """The exploration words differ from the policy sampling stream's and the action stream's for the same key."""
    from oracle import actor_oracle as AO
    from oracle import philox
    env_ids = np.arange(4096)
    we, wa = QR.explore_words(7, env_ids, 3, 5, 4)
    assert not np.array_equal(we, wa)
    u_pol = AO.policy_uniforms(7, env_ids, 3, 5, 4)
    assert not np.array_equal(philox.u01(we).astype(np.float32), u_pol)
    act = philox.expected_actions(7, env_ids, 3, 5, 4)
    assert np.mean(philox.rand5(wa) == act) < 0.3
    # uniform explore values and actions
    assert abs(float(np.mean(philox.u01(we))) - 0.5) < 0.01
    assert np.all(np.abs(np.bincount(philox.rand5(wa).ravel(), minlength=5) / wa.size - 0.2) < 0.02)


def test_epsilon_greedy_law_of_the_restatement():
    greedy = np.zeros((8192, 4), np.int64)
    ids = np.arange(8192)
    assert np.array_equal(QR.epsilon_greedy(greedy, 1, ids, 0, 0, 0.0), greedy)
    full = QR.epsilon_greedy(greedy, 1, ids, 0, 0, 1.0)
    assert np.all(np.abs(np.bincount(full.ravel(), minlength=5) / full.size - 0.2) < 0.02)
