"""CPU: the restatement of the particle QMIX mixer (tests/qmix_mixer_ref.py) against the golden vectors recorded by executing the
reference's own networks.Qmix_mixer (tools/gen_golden_qmix_mixer.py -> tests/golden/qmix_mixer_particle.npz), the fixture's weight
names and shapes against the ones the device mixer maps, and -- where the reference sources are readable -- the generator re-run
against the committed file.

Both distances to the fixture are measured per row as |restatement - fixture| / max(1, |fixture|), the measure of
tests/test_critic_oracle.py: |q_tot| reaches 193, where one float32 step of the fixture's own value is 1.5e-5, so an absolute 1e-5
is below what the fixture can resolve (the float64 restatement is 1.7e-5 away from it at N = 10 in absolute terms, 3.6e-6 in this
measure; the float32 restatement in the shim's order reproduces the fixture bit for bit)."""
import os

import numpy as np
import pytest

from tests import qmix_mixer_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "qmix_mixer_particle.npz")
AGENTS = [1, 2, 3, 4, 8, 10]
BOUND = 2e-5                       # the project's float32-network bound (tests/critic_feeds.py)


def load_case(n):
    z = np.load(GOLDEN)
    tag = "n%d" % n
    w = {str(k): z[tag + "/w/" + str(k)] for k in z[tag + "/names"]}
    return w, {k: z[tag + "/in/" + k] for k in ("agent_qs", "state", "goals_all")}, z[tag + "/q_tot"]


def _distance(got, q):
    return float((np.abs(got - q) / np.maximum(1.0, np.abs(q))).max())


@pytest.mark.parametrize("n", AGENTS)
def test_restatement_reproduces_the_reference_network(n):
    w, x, q = load_case(n)
    got = MR.q_tot(w, x["agent_qs"], x["state"], x["goals_all"], dtype=np.float32)
    assert got.dtype == np.float32 and q.dtype == np.float32 and got.shape == q.shape == (x["state"].shape[0], 1)
    assert 40 <= q.shape[0] <= 96
    assert x["agent_qs"].shape == (q.shape[0], n) and x["state"].shape[1] == 4 * n and x["goals_all"].shape[1] == 2 * n
    ref = MR.q_tot(w, x["agent_qs"], x["state"], x["goals_all"], dtype=np.float64)
    print("N=%d: float32 restatement %.3g, float64 restatement %.3g (absolute %.3g) from the fixture; |q_tot| %.3g .. %.3g"
          % (n, _distance(got, q), _distance(ref, q), float(np.abs(ref - q).max()), float(np.abs(q).min()), float(np.abs(q).max())))
    assert _distance(got, q) <= 1e-6
    assert _distance(ref, q) <= 1e-5


@pytest.mark.parametrize("n", AGENTS)
def test_kernel_order_is_the_same_network(n):
    """the sums in the order the device kernel evaluates them: float64 equal to the matmul form to rounding, float32 inside the
    project's bound against float64, which the kernel has to meet (the share is printed)"""
    w, x, _ = load_case(n)
    args = (w, x["agent_qs"], x["state"], x["goals_all"])
    ref = MR.q_tot(*args, dtype=np.float64)
    assert np.abs(MR.q_tot(*args, dtype=np.float64, order="kernel") - ref).max() <= 1e-12 * np.abs(ref).max()
    k32 = MR.q_tot(*args, dtype=np.float32, order="kernel")
    assert k32.dtype == np.float32
    share = float((np.abs(k32 - ref) / (BOUND * np.maximum(1.0, np.abs(ref)))).max())
    print("N=%d: float32 in kernel order uses %.3f of the bound" % (n, share))
    assert share <= 1.0


@pytest.mark.parametrize("n", AGENTS)
def test_fixture_weights_are_the_five_the_mixer_maps(n):
    from cm3_amd import qmix
    w, _, _ = load_case(n)
    want = list(qmix.MIXER_NAMES.values())
    assert sorted(want) == sorted(MR.NAMES) and len(w) == 5
    assert sorted(w) == sorted("Mixer_target/" + k for k in want)
    assert sorted(qmix._mixer_canon(k) for k in w) == sorted(want) == sorted(MR.canon(k) for k in w)
    shapes = qmix.mixer_weight_shapes(n)
    for short, shape in shapes.items():
        assert w["Mixer_target/" + qmix.MIXER_NAMES[short]].shape == shape == MR.shapes(n)[qmix.MIXER_NAMES[short]], short
        assert w["Mixer_target/" + qmix.MIXER_NAMES[short]].dtype == np.float32
    assert qmix._mixer_canon("Mixer_main/hyper_b_final_l1/kernel:0") == "hyper_b_final_l1/kernel"
    assert sorted(MR.init_weights(np.random.default_rng(0), n)) == sorted(want)
    for k, v in MR.init_weights(np.random.default_rng(0), n, scope="Mixer_target").items():
        assert v.shape == w[k].shape and v.dtype == np.float32


def test_fixture_is_no_larger_than_the_largest_critic_fixture():
    import glob
    largest = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "critic_*.npz")))
    assert os.path.getsize(GOLDEN) <= largest


def _reference_root():
    import inspect
    from oracle import tf_numpy_shim
    return inspect.signature(tf_numpy_shim.load_networks).parameters["ref_root"].default


@pytest.mark.skipif(not os.path.exists(os.path.join(_reference_root(), "alg", "networks.py")),
                    reason="the reference sources are not readable here")
def test_generator_reproduces_the_committed_fixture(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_qmix_mixer", os.path.join(ROOT, "tools", "gen_golden_qmix_mixer.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    again = np.load(gen.main(str(tmp_path)))
    have = np.load(GOLDEN)
    assert sorted(again.files) == sorted(have.files)
    for k in have.files:
        assert np.array_equal(again[k], have[k]), k
