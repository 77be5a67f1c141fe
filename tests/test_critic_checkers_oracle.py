"""CPU: the restatement of the CM3 Checkers critics (tests/critic_checkers_ref.py) in float32 against the golden vectors recorded by
executing the reference's own networks.Q_global_checkers / networks.Q_credit_checkers (tools/gen_golden_critic_checkers.py ->
tests/golden/critic_checkers_<kind>_n<N>.npz), the fixture's weight names and shapes against the ones the device critic maps, the
fixture's rows as decodings of base columns, and -- where the reference sources are readable -- the generator re-run against the
committed files."""
import os

import numpy as np
import pytest

from tests import critic_checkers_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("global", 1), ("global", 2), ("credit", 2), ("global", 8), ("credit", 8)]


def golden_path(kind, n):
    return os.path.join(ROOT, "tests", "golden", "critic_checkers_%s_n%d.npz" % (kind, n))


def load_case(kind, n):
    z = np.load(golden_path(kind, n))
    w = {str(k): z["w/" + str(k)] for k in z["names"]}
    names = ("s_grid", "s_n", "g_n", "t_obs", "v_obs") + (("a_n", "s_others", "a_others") if kind == "global"
                                                         else ("a_m", "s_m", "s_others"))
    return w, {k: z["in/" + k] for k in names}, z["q"]


def ref_q(kind, n, w, x, dtype):
    if kind == "global":
        return CR.q_global(w, x["s_grid"], x["s_n"], x["g_n"], x["a_n"], x["s_others"], x["a_others"], x["t_obs"], x["v_obs"],
                           stage=1 if n == 1 else 2, dtype=dtype)
    return CR.q_credit(w, x["s_grid"], x["s_n"], x["g_n"], x["a_m"], x["s_m"], x["s_others"], x["t_obs"], x["v_obs"], dtype=dtype)


@pytest.mark.parametrize("kind,n", CASES)
def test_float32_restatement_reproduces_the_reference_network(kind, n):
    w, x, q = load_case(kind, n)
    got = ref_q(kind, n, w, x, np.float32)
    assert got.dtype == np.float32 and got.shape == q.shape == (x["s_n"].shape[0], 1)
    assert 40 <= q.shape[0] <= 64
    assert set(np.unique(x["s_grid"])) <= {0.0, 1.0} and set(np.unique(x["t_obs"])) <= {-1.0, 0.0, 1.0}
    err = np.abs(got - q) / np.maximum(1.0, np.abs(q))
    print(kind, n, "max relative error", float(err.max()), "max |q|", float(np.abs(q).max()))
    assert err.max() <= 1e-6
    assert np.abs(ref_q(kind, n, w, x, np.float64) - q).max() < 1e-5       # and float64 stays next to it


@pytest.mark.parametrize("kind,n", CASES)
def test_fixture_weights_are_the_twelve_the_critic_maps(kind, n):
    from cm3_amd import critic
    w, x, _ = load_case(kind, n)
    scope = "Q_%s_main/" % kind
    want = [k for k in critic.CK_NAMES.values() if n > 1 or "stage-2" not in k]
    assert sorted(critic.CK_NAMES.values()) == sorted(CR.NAMES) and len(CR.NAMES) == 12
    assert sorted(w) == sorted(scope + k for k in want)
    assert sorted(critic._canon(k) for k in w) == sorted(want) == sorted(CR.canon(k) for k in w)
    shapes = critic.checkers_weight_shapes(n, kind, 1 if n == 1 else 2)
    for short, shape in shapes.items():
        assert w[scope + critic.CK_NAMES[short]].shape == shape, short
    assert len(shapes) == len(w) == (12 if n > 1 else 9)
    assert (critic.CK_H1_1, critic.CK_H1_2, critic.CK_H2) == (256, 32, 256) == (CR.H1_1, CR.H1_2, CR.H2)
    assert critic._canon("Q_credit_target/conv_o/Conv/weights:0") == "conv_o/Conv/weights"
    assert sorted(CR.init_weights(np.random.default_rng(0), n, kind)) == sorted(want)
    for k, v in CR.init_weights(np.random.default_rng(0), n, kind, scope="Q_%s_main" % kind).items():
        assert v.shape == w[k].shape and v.dtype == np.float32


@pytest.mark.parametrize("kind,n", CASES)
def test_fixture_rows_are_decodings_of_base_columns(kind, n):
    """Tiling the base columns as the reference's train_step does and picking the fixture's rows gives the fixture's inputs back."""
    _, x, _ = load_case(kind, n)
    cols, pick = CR.fixture_base_columns(kind, n, x)
    rows = x["s_n"].shape[0]
    nn, mm = CR.pair_agents(rows, n)
    i = np.arange(rows)
    assert len(set(pick.tolist())) == rows and pick.max() < rows * n * (n if kind == "credit" else 1)
    if kind == "credit":
        assert {(a, b) for a, b in zip(nn.tolist(), mm.tolist())} == {(a, b) for a in range(n) for b in range(n)}
        assert np.array_equal(pick // n % n, mm) and np.array_equal(pick % n, nn)
        assert np.array_equal(cols["vec"][i, mm].astype(np.float32), x["s_m"])
        assert np.array_equal(cols["obs_self_t"][i, mm], x["t_obs"]) and np.array_equal(cols["obs_self_v"][i, mm].astype(np.float32), x["v_obs"])
        assert np.array_equal(np.eye(5, dtype=np.float32)[cols["actions"][i, mm]], x["a_m"])
    else:
        assert np.array_equal(cols["obs_self_t"][i, nn], x["t_obs"])
        assert np.array_equal(np.eye(5, dtype=np.float32)[cols["actions"][i, nn]], x["a_n"])
    assert np.array_equal(cols["vec"][i, nn].astype(np.float32), x["s_n"]) and np.array_equal(cols["goals"][i, nn], x["g_n"])


def _reference_root():
    import inspect
    from oracle import tf_numpy_shim
    return inspect.signature(tf_numpy_shim.load_networks).parameters["ref_root"].default


@pytest.mark.skipif(not os.path.exists(os.path.join(_reference_root(), "alg", "networks.py")),
                    reason="the reference sources are not readable here")
def test_generator_reproduces_the_committed_fixtures(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_critic_checkers",
                                                  os.path.join(ROOT, "tools", "gen_golden_critic_checkers.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    paths = gen.main(str(tmp_path))
    assert sorted(paths) == sorted("%s_n%d" % c for c in CASES)
    for kind, n in CASES:
        again, have = np.load(paths["%s_n%d" % (kind, n)]), np.load(golden_path(kind, n))
        assert os.path.getsize(golden_path(kind, n)) < 900 * 1024
        assert sorted(again.files) == sorted(have.files)
        for k in have.files:
            assert np.array_equal(again[k], have[k]), k


def test_float32_restatement_uses_at_most_half_the_bound_on_the_gpu_cases():
    """The GPU tests hold the kernel to 2e-5 * max(1, |ref|) against float64 on these cases; float32 arithmetic alone (NumPy's order)
    must leave at least half of that, and |Q| must reach several units so that the relative part of the bound is live."""
    from tests import critic_checkers_feeds as CF
    worst = largest = 0.0
    for N in CF.AGENTS:
        for B in CF.BATCHES:
            r64, r32 = CF.refs(N, B, np.float64), CF.refs(N, B, np.float32)
            for op in r64:
                used = np.abs(r32[op].astype(np.float64) - r64[op]) / (CF.BOUND * np.maximum(1.0, np.abs(r64[op])))
                worst, largest = max(worst, float(used.max())), max(largest, float(np.abs(r64[op]).max()))
    print("float32 restatement: share of the bound used %.3f, max |q| %.2f" % (worst, largest))
    assert worst <= 0.5 and largest >= 3.0
