"""CPU: the two ways cm3_amd.batch.train_step_feeds gets its static feeds build the SAME dict -- names, shapes, dtypes, bits: the torch
composition (_static_feeds_composed: the reference's own gathers and repeats) and the spec tables of the tiling kernels
(particle_static_feed_specs / checkers_static_feed_specs, evaluated with tests/rows_tile_ref.py).  At N = 3 there are two other
agents, so a wrong order of the `others` mapping shows.  And: with `static` given, train_step_feeds creates no identity matrix."""
import pytest
import torch

from tests import rows_tile_ref as REF
from tests.test_particle_static_feeds import particle_cols, specs_and_static


def checkers_cols(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    f = lambda *s: torch.randint(-3, 4, s, generator=g).to(torch.float64) + torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    cols = dict(grid=f(B, 3, 9, 2), vec=f(B, N, 4), obs_others=f(B, N, 2 * (N - 1)), obs_self_t=f(B, N, 5, 5, 3), obs_self_v=f(B, N, 4),
                actions_prev=torch.randint(0, 5, (B, N), generator=g, dtype=torch.int32),
                actions=torch.randint(0, 5, (B, N), generator=g, dtype=torch.int32), reward=f(B), local_rewards=f(B, N),
                next_grid=f(B, 3, 9, 2), next_vec=f(B, N, 4), next_obs_others=f(B, N, 2 * (N - 1)), next_obs_self_t=f(B, N, 5, 5, 3),
                next_obs_self_v=f(B, N, 4), done=torch.tensor([False, True, False, False, True][:B]),
                goals=torch.nn.functional.one_hot(torch.randint(0, 2, (B, N), generator=g), 2))
    return cols


def _both(env, N):
    from cm3_amd import batch as BR
    if env == "particle":
        cols = particle_cols(5, N, seed=3)
        assert cols["v_global"].dtype == torch.float32
        _, S = specs_and_static(cols)
    else:
        cols = checkers_cols(5, N, seed=4)
        assert cols["vec"].dtype == torch.float64
        S = REF.static_feeds(cols, BR.checkers_static_feed_specs({n: tuple(v.shape) for n, v in cols.items()}, cols["goals"].dtype))
    return cols, S, BR._static_feeds_composed(cols, BR._ENVS[env], 5, True)


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("env", ["particle", "checkers"])
def test_composed_dict_equals_spec_dict(env, N):
    cols, S, C = _both(env, N)
    assert set(C) == set(S) and len(S) == (22 if env == "particle" else 33)
    for name in S:
        assert C[name].shape == S[name].shape and C[name].dtype == S[name].dtype, (name, C[name].shape, S[name].shape, C[name].dtype,
                                                                                    S[name].dtype)
        assert torch.equal(C[name], S[name]), name


@pytest.mark.parametrize("env", ["particle", "checkers"])
def test_without_credit_only_the_per_agent_rows_are_built(env):
    from cm3_amd import batch as BR
    cols, S, C = _both(env, 2)
    P = BR._static_feeds_composed(cols, BR._ENVS[env], 5, False)
    B = 5
    assert set(P) == {name for name, t in S.items() if t.shape[0] == B * 2}             # per agent row: B N rows
    assert all(torch.equal(P[name], C[name]) for name in P)


@pytest.mark.parametrize("env", ["particle", "checkers"])
def test_static_path_creates_no_identity_matrix(env, monkeypatch):
    """train_step_feeds(static=...) reads the counterfactual actions from the static dict; a torch.eye it issued anyway would be
    captured by OnPolicyPhasePlan into a graph that outlives the tensor."""
    from cm3_amd import batch as BR
    B, N = 5, 2
    cols, S, _ = _both(env, N)

    def run(ops, feed):
        rows = max([v.shape[0] for v in feed.values() if torch.is_tensor(v) and v.dim() > 0] or [1])
        answer = {"action_samples_target": torch.arange(B * N) % 5, "probs": torch.full((rows, 5), 0.2, dtype=torch.float64)}
        return [None if (op.endswith("_op") or op == "list_update_target_ops") else answer.get(op, torch.ones(rows, dtype=torch.float64))
                for op in ops]

    want = BR.train_step_feeds(cols, run, 0.99, 0.1, env=env, static=S)

    def no_eye(*args, **kwargs):
        raise AssertionError("torch.eye called on the static path")
    monkeypatch.setattr(torch, "eye", no_eye)
    calls = BR.train_step_feeds(cols, run, 0.99, 0.1, env=env, static=S)
    assert [c[0] for c in calls] == [c[0] for c in want] and len(calls) == 11
    with pytest.raises(AssertionError, match="torch.eye called"):                       # (the composition does build one)
        BR.train_step_feeds(cols, run, 0.99, 0.1, env=env)
