"""CPU: tests/baseline_ref.py against the fixture recorded from the reference's own networks.V_particle_local / V_particle_global /
Q_global (tools/gen_golden_baseline.py): evaluated in float32 on the placeholders' inputs, the restatement reproduces the recorded
outputs -- the same NumPy operations in the same order, so exactly."""
import os

import numpy as np
import pytest

import baseline_ref as BR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("tag", BR.VALUE_CASES + BR.COMA_CASES)
def test_restatement_reproduces_the_recorded_outputs(tag):
    w, x, out = BR.load_case(GOLDEN, tag)
    n = int(tag.split("_n")[1])
    assert 40 <= out.shape[0] <= 96 and out.dtype == np.float32
    assert out.shape[1] == (5 if tag.startswith("coma") else 1)
    assert len(w) == (6 if tag.startswith("coma") else (4 if n == 1 else 7))
    got = BR.eval_case(tag, w, x, np.float32)
    assert got.dtype == np.float32 and got.shape == out.shape
    assert np.array_equal(got, out)
    # ... and float64 agrees to float32 accuracy: the fixture is no accident of rounding
    ref = BR.eval_case(tag, w, x, np.float64)
    assert np.all(np.abs(out - ref) <= 2e-5 * np.maximum(1.0, np.abs(ref)))


def test_the_fixture_carries_the_reference_variable_names():
    w, _, _ = BR.load_case(GOLDEN, "local_n4")
    assert sorted(w) == ["V_main/V_particle_branch_self/bias", "V_main/V_particle_branch_self/kernel", "V_main/V_particle_out/kernel",
                         "V_main/W_branch_self_out", "V_main/stage-2/V_local_others/bias", "V_main/stage-2/V_local_others/kernel",
                         "V_main/stage-2/W_others_out"]
    assert w["V_main/stage-2/V_local_others/kernel"].shape == (12, 128)
    w, _, _ = BR.load_case(GOLDEN, "global_n10")
    assert w["V_main/stage-2/V_particle_branch2/kernel"].shape == (54, 128) and "V_main/stage-2/W_branch2_h2" in w
    w, x, _ = BR.load_case(GOLDEN, "coma_n10")
    assert w["Q_main/stage-2/Q_goals/h1/kernel"].shape == (119, 256) and w["Q_main/stage-2/Q_goals/out/bias"].shape == (5,)
    assert x["action_others"].shape[1:] == (9, 5)
