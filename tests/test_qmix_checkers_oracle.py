"""CPU: the float64 restatement of the QMIX baseline's Checkers agent network (tests/qmix_checkers_ref.py) against the golden vectors
recorded by executing the reference's own networks.Qmix_single_checkers (tools/gen_golden_qmix_checkers.py ->
tests/golden/qmix_checkers.npz), the fixture's variable names against the ones the device agent maps, and the epsilon-greedy law
of the restatement."""
import os

import numpy as np
import pytest

from tests import qmix_checkers_ref as QC
from tests import qmix_ref as QR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qmix_checkers.npz")
CASES = [1, 2]


def _case(n):
    z = np.load(GOLDEN)
    tag = "n%d" % n
    w = {str(k): z["w/" + str(k)] for k in z["names"]}
    inputs = {k: z[tag + "/in/" + k] for k in ("a_prev", "obs_self_t", "obs_self_v", "obs_others", "goals")}
    return w, inputs, z[tag + "/q"], z[tag + "/argmax"]


def _q(w, x, dtype=np.float64):
    return QC.q_values(w, x["a_prev"], x["obs_self_t"], x["obs_self_v"], x["obs_others"], x["goals"], dtype=dtype)


@pytest.mark.parametrize("n", CASES)
def test_float64_restatement_reproduces_the_reference_network(n):
    w, x, q, amax = _case(n)
    got = _q(w, x)
    assert got.shape == q.shape == (x["obs_self_v"].shape[0], 5)
    # the shim computes in float32: 256-deep sums of products of ~1, rounded at every layer
    assert np.abs(got - q).max() < 2e-5 * max(1.0, float(np.abs(q).max()))
    assert np.array_equal(np.argmax(got, axis=1), amax)
    assert len(set(amax.tolist())) > 1                     # the fixture exercises more than one greedy action
    # the same graph in float32 is the shim's arithmetic up to summation order
    assert np.abs(_q(w, x, np.float32) - q).max() < 2e-5 * max(1.0, float(np.abs(q).max()))


@pytest.mark.parametrize("n", CASES)
def test_fixture_inputs_are_what_the_env_feeds(n):
    _, x, _, _ = _case(n)
    assert set(np.unique(x["obs_self_t"]).tolist()) <= {-1.0, 0.0, 1.0}
    assert x["obs_others"].shape[1] == 2 * max(n - 1, 1)
    assert np.array_equal(x["goals"].sum(axis=1), np.ones(x["goals"].shape[0]))
    assert x["a_prev"].min() >= 0 and x["a_prev"].max() < 5


def test_fixture_weights_are_the_thirteen_the_agent_maps():
    from cm3_amd import qmix
    w, _, _, _ = _case(1)
    assert len(w) == 13
    assert sorted(w) == sorted("Agent_main/" + k for k in qmix.CK_NAMES.values())
    assert sorted(qmix._canon(k) for k in w) == sorted(qmix.CK_NAMES.values()) == sorted(QC.NAMES)
    for name, shape in QC.shapes(2).items():
        assert w["Agent_main/" + name].shape == shape, name
    # the others branch at N = 1 reads the agent's own position: 2 inputs, as at N = 2
    assert QC.shapes(1)["branch_others/kernel"] == (2, 256) == QC.shapes(2)["branch_others/kernel"]
    assert qmix._canon("Agent_target/Qmix_single_out/kernel:0") == "Qmix_single_out/kernel"


def test_init_weights_use_the_reference_names_and_shapes():
    for n in (1, 3, 8):
        w = QC.init_weights(np.random.default_rng(n), n)
        assert sorted(QR.canon(k) for k in w) == sorted(QC.NAMES)
        for name, shape in QC.shapes(n).items():
            assert w["Agent_main/" + name].shape == shape and w["Agent_main/" + name].dtype == np.float32


def test_epsilon_greedy_law_of_the_restatement():
    """The Checkers agent draws from the particle agent's stream, keyed with the env's episode / step counters: epsilon = 0 is
    greedy, epsilon = 1 is rand5 of the action word, and in between exactly the agents whose explore word is below epsilon."""
    from oracle import philox
    rng = np.random.default_rng(5)
    E, N, seed = 8192, 2, 12341
    ids = np.arange(E) + 17
    ep = rng.integers(0, 100, E)
    st = rng.integers(0, 50, E)
    greedy = rng.integers(0, 5, (E, N))
    assert np.array_equal(QR.epsilon_greedy(greedy, seed, ids, ep, st, 0.0), greedy)
    we, wa = QR.explore_words(seed, ids, ep, st, N)
    full = QR.epsilon_greedy(greedy, seed, ids, ep, st, 1.0)
    assert np.array_equal(full, philox.rand5(wa))
    assert np.all(np.abs(np.bincount(full.ravel(), minlength=5) / full.size - 0.2) < 0.02)
    a3 = QR.epsilon_greedy(greedy, seed, ids, ep, st, 0.3)
    explored = philox.u01(we) < np.float32(0.3)
    assert abs(explored.mean() - 0.3) < 5 * np.sqrt(0.21 / explored.size)
    assert np.array_equal(a3[~explored], greedy[~explored])
    assert np.array_equal(a3[explored], philox.rand5(wa)[explored])
    # the counters are part of the key: another step gives other draws
    we2, _ = QR.explore_words(seed, ids, ep, st + 1, N)
    assert np.mean(we2 != we) > 0.99
