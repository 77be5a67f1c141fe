"""CPU: the restatement of the Checkers QMIX mixer (tests/qmix_mixer_checkers_ref.py) against the golden vectors recorded by executing
the reference's own networks.Qmix_mixer_checkers (tools/gen_golden_qmix_mixer_checkers.py -> tests/golden/qmix_mixer_checkers_n*.npz),
the fixture's weight names and shapes against the ones the device mixer maps, the share of the project's bound that the float32
restatement alone uses on the GPU tests' cases, and -- where the reference sources are readable -- the generator re-run against the
committed files.

Distances to the fixture are measured per row as |restatement - fixture| / max(1, |fixture|), the measure of
tests/test_qmix_mixer_oracle.py: |q_tot| reaches 112, where one float32 step of the fixture's own value is 7.6e-6.  The float32
restatement in the shim's order reproduces the fixture bit for bit; the float64 one is at most 4.8e-7 away in this measure."""
import glob
import os

import numpy as np
import pytest

from tests import qmix_mixer_checkers_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "qmix_mixer_checkers_n%d.npz")
AGENTS = [1, 2, 3, 5]
BOUND = 2e-5                       # the project's float32-network bound (tests/critic_feeds.py)
INPUTS = ("agent_qs", "state_env", "state", "goals_all")


def load_case(n):
    z = np.load(GOLDEN % n)
    w = {str(k): z["w/" + str(k)] for k in z["names"]}
    return w, {k: z["in/" + k] for k in INPUTS}, z["q_tot"]


def _distance(got, q):
    return float((np.abs(got - q) / np.maximum(1.0, np.abs(q))).max())


def _args(w, x):
    return (w, x["agent_qs"], x["state_env"], x["state"], x["goals_all"])


@pytest.mark.parametrize("n", AGENTS)
def test_restatement_reproduces_the_reference_network(n):
    w, x, q = load_case(n)
    got = MR.q_tot(*_args(w, x), dtype=np.float32)
    assert got.dtype == np.float32 and q.dtype == np.float32 and got.shape == q.shape == (x["state"].shape[0], 1)
    assert 40 <= q.shape[0] <= 96
    assert x["agent_qs"].shape == (q.shape[0], n) and x["state"].shape[1] == 4 * n and x["goals_all"].shape[1] == 2 * n
    assert x["state_env"].shape == (q.shape[0], 3, 9, 2) and set(np.unique(x["state_env"])) <= {0.0, 1.0}
    assert np.array_equal(x["goals_all"].reshape(-1, 2).sum(axis=1), np.ones(q.shape[0] * n))          # one-hot goals
    ref = MR.q_tot(*_args(w, x), dtype=np.float64)
    print("N=%d: float32 restatement %.3g, float64 restatement %.3g (absolute %.3g) from the fixture; |q_tot| %.3g .. %.3g"
          % (n, _distance(got, q), _distance(ref, q), float(np.abs(ref - q).max()), float(np.abs(q).min()), float(np.abs(q).max())))
    assert _distance(got, q) <= 1e-6
    assert _distance(ref, q) <= 1e-5


@pytest.mark.parametrize("n", AGENTS)
def test_kernel_order_is_the_same_network(n):
    """the sums in the order the device kernel evaluates them: float64 equal to the matmul form to rounding, float32 inside the
    project's bound against float64, which the kernel has to meet (the share is printed)"""
    w, x, _ = load_case(n)
    ref = MR.q_tot(*_args(w, x), dtype=np.float64)
    assert np.abs(MR.q_tot(*_args(w, x), dtype=np.float64, order="kernel") - ref).max() <= 1e-12 * np.abs(ref).max()
    k32 = MR.q_tot(*_args(w, x), dtype=np.float32, order="kernel")
    assert k32.dtype == np.float32
    share = float((np.abs(k32 - ref) / (BOUND * np.maximum(1.0, np.abs(ref)))).max())
    print("N=%d: float32 in kernel order uses %.3f of the bound" % (n, share))
    assert share <= 1.0


def test_float32_restatement_uses_at_most_half_of_the_bound_on_the_gpu_cases():
    """The GPU tests (tests/test_gpu_qmix_mixer_checkers.py) hold the device to 2e-5 * max(1, |ref|) against the float64 restatement
    on MR.gpu_case / MR.gpu_weights.  The float32 NumPy restatement of the same rows, in the shim's matmul order and in the kernel's
    order, must use at most half of that bound, so that the bound is one the format can meet on these cases; and |q_tot| must span
    both the absolute and the relative part of the bound."""
    worst, lo, hi = {"matmul": 0.0, "kernel": 0.0}, np.inf, 0.0
    for n in MR.GPU_AGENTS:
        for b in MR.GPU_BATCHES:
            ref = MR.gpu_ref(n, b)
            lo, hi = min(lo, float(np.abs(ref).min())), max(hi, float(np.abs(ref).max()))
            for order in worst:
                got = MR.gpu_ref(n, b, dtype=np.float32, order=order)
                assert got.dtype == np.float32
                share = float((np.abs(got - ref) / (BOUND * np.maximum(1.0, np.abs(ref)))).max())
                print("N=%d B=%d %s: %.3f of the bound" % (n, b, order, share))
                worst[order] = max(worst[order], share)
    print("worst shares: matmul %.3f, kernel %.3f; |q_tot| %.3g .. %.3g" % (worst["matmul"], worst["kernel"], lo, hi))
    assert max(worst.values()) <= 0.5
    assert lo < 0.5 and hi > 20.0


@pytest.mark.parametrize("n", AGENTS)
def test_fixture_weights_are_the_seven_the_mixer_maps(n):
    from cm3_amd import qmix
    w, _, _ = load_case(n)
    want = list(qmix.CK_MIXER_NAMES.values())
    assert sorted(want) == sorted(MR.NAMES) and len(w) == 7
    assert sorted(w) == sorted("Mixer_target/" + k for k in want)
    assert sorted(qmix._mixer_canon(k) for k in w) == sorted(want) == sorted(MR.canon(k) for k in w)
    for short, shape in qmix.checkers_mixer_weight_shapes(n).items():
        name = qmix.CK_MIXER_NAMES[short]
        assert w["Mixer_target/" + name].shape == shape == MR.shapes(n)[name], short
        assert w["Mixer_target/" + name].dtype == np.float32
    assert sorted(MR.init_weights(np.random.default_rng(0), n)) == sorted(want)
    for k, v in MR.init_weights(np.random.default_rng(0), n, scope="Mixer_target").items():
        assert v.shape == w[k].shape and v.dtype == np.float32


def test_fixtures_are_no_larger_than_the_largest_other_fixture():
    mine = [GOLDEN % n for n in AGENTS]
    largest = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")) if p not in mine)
    assert all(os.path.getsize(p) <= largest for p in mine)
    assert not os.path.exists(GOLDEN % 8)                      # (N = 8: the float64 restatement only)


def _reference_root():
    import inspect
    from oracle import tf_numpy_shim
    return inspect.signature(tf_numpy_shim.load_networks).parameters["ref_root"].default


@pytest.mark.skipif(not os.path.exists(os.path.join(_reference_root(), "alg", "networks.py")),
                    reason="the reference sources are not readable here")
def test_generator_reproduces_the_committed_fixtures(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_qmix_mixer_checkers",
                                                  os.path.join(ROOT, "tools", "gen_golden_qmix_mixer_checkers.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    paths = gen.main(str(tmp_path))
    assert sorted(os.path.basename(p) for p in paths) == sorted(os.path.basename(GOLDEN % n) for n in AGENTS)
    for path in paths:
        again, have = np.load(path), np.load(os.path.join(ROOT, "tests", "golden", os.path.basename(path)))
        assert sorted(again.files) == sorted(have.files)
        for k in have.files:
            assert np.array_equal(again[k], have[k]), (path, k)
