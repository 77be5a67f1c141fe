"""The actor oracles (oracle/actor_oracle.py, oracle/actor_checkers_oracle.py) against golden vectors produced by executing
the REFERENCE's own function bodies networks.actor_particle / networks.actor_checkers under a NumPy stand-in for the TF1
calls they make (oracle/tf_numpy_shim.py, oracle/gen_golden_actor.py -> tests/golden/actor_*.npz): layer wiring, concat
order, variable names and shapes are the reference's; the primitive-op semantics are the shim's (TensorFlow itself is not
installable here).  Re-running oracle/gen_golden_actor.py where the reference tree is at hand re-derives the committed vectors."""
import os

import numpy as np
import pytest

from oracle import actor_checkers_oracle as CO
from oracle import actor_oracle as PO
from tests.helpers import GOLDEN


def load_cases(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    tags = sorted({k.split("/")[0] for k in z.files})
    cases = {}
    for tag in tags:
        w = {k[len(tag) + 3:]: z[k] for k in z.files if k.startswith(tag + "/w/")}
        inp = {k[len(tag) + 4:]: z[k] for k in z.files if k.startswith(tag + "/in/")}
        cases[tag] = (w, inp, z[tag + "/probs"])
    return cases


@pytest.mark.parametrize("tag", ["n1_stage1", "n4_stage2", "n8_stage2"])
def test_particle_actor_oracle_matches_reference_wiring(tag):
    w, inp, probs = load_cases("actor_particle")[tag]
    got = PO.actor_probs(w, inp["obs_others"], inp["v_obs"], inp["v_goal"])
    assert got.shape == probs.shape and np.abs(got - probs).max() < 1e-6
    assert np.ptp(probs, axis=1).mean() > 0.05
    assert set(w) == set(PO.init_weights(np.random.default_rng(0), int(tag[1]), stage=int(tag[-1])))


@pytest.mark.parametrize("tag", ["n1_stage1", "n2_stage2"])
def test_checkers_actor_oracle_matches_reference_wiring(tag):
    w, inp, probs = load_cases("actor_checkers")[tag]
    got = CO.actor_probs(w, inp["a_prev"], inp["obs_self_t"], inp["obs_self_v"], inp["obs_others"], inp["goals"])
    assert got.shape == probs.shape and np.abs(got - probs).max() < 1e-6
    assert set(w) == set(CO.init_weights(np.random.default_rng(0), int(tag[1]), stage=int(tag[-1])))
    for k, v in CO.init_weights(np.random.default_rng(0), int(tag[1]), stage=int(tag[-1])).items():
        assert v.shape == w[k].shape, k
