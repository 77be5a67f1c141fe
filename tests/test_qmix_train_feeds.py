"""CPU: cm3_amd.batch.qmix_train_step_feeds / process_batch_qmix against the arrays the REAL alg_qmix.Alg.train_step built and fed
(tests/golden/trainstep_qmix_particle_n*.npz, recorded by tools/gen_golden_qmix_trainstep.py from the reference code under a
recording session): call order, feed keys, and shape, dtype and bits of every array -- td_target included, whose row sum the
eight- and ten-agent fixtures pin to np.sum's eight-accumulator tree and its tail."""
import json
import os

import numpy as np
import pytest
import torch

TAGS = ("n1", "n4", "n8", "n10")
ORDER = [["argmax_Q_target"], ["mixer_target"], ["mixer_op"], ["list_update_target_ops"]]
FEEDS = [{"obs_others", "v_obs", "v_goal"},
         {"v_state", "v_goal_all", "actions_1hot", "obs_others", "v_obs", "v_goal"},
         {"v_state", "v_goal_all", "actions_1hot", "obs_others", "v_obs", "v_goal", "td_target"}, set()]


def _load(golden_dir, tag):
    z = np.load(os.path.join(golden_dir, "trainstep_qmix_particle_%s.npz" % tag))
    index = json.loads(str(z["index"]))
    cols = {k[3:]: torch.as_tensor(z[k]) for k in z.files if k.startswith("in_")}
    return z, index, cols


def _same(got, want, what):
    got = got.numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert np.array_equal(got, want), what


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_is_what_the_issue_describes(tag, golden_dir):
    z, index, cols = _load(golden_dir, tag)
    assert [c["ops"] for c in index["calls"]] == ORDER
    assert [set(c["feed"]) for c in index["calls"]] == FEEDS
    assert index["gamma"] == 0.99 and index["n_agents"] == int(tag[1:])
    assert cols["v_global"].shape[0] <= 12
    assert z["c1_res_mixer_target"].dtype == np.float32 and z["c1_res_mixer_target"].shape == (cols["v_global"].shape[0], 1)
    assert z["c0_res_argmax_Q_target"].shape == (cols["v_global"].shape[0] * index["n_agents"],)
    assert z["c2_feed_td_target"].dtype == np.float64


@pytest.mark.parametrize("tag", TAGS)
def test_feeds_equal_the_reference_train_step(tag, golden_dir):
    from cm3_amd.batch import qmix_train_step_feeds
    z, index, cols = _load(golden_dir, tag)
    seen = []

    def run(ops, feed):
        c = len(seen)
        seen.append(ops)
        return [torch.as_tensor(z["c%d_res_%s" % (c, op)]) if ("c%d_res_%s" % (c, op)) in z.files else None for op in ops]

    calls = qmix_train_step_feeds(cols, run, index["gamma"])
    assert seen == ORDER and [ops for ops, _ in calls] == ORDER
    for c, ((ops, feed), want) in enumerate(zip(calls, index["calls"])):
        assert sorted(feed) == want["feed"], (c, sorted(feed))
        for k, v in feed.items():
            _same(v, z["c%d_feed_%s" % (c, k)], (tag, c, k))


@pytest.mark.parametrize("tag", TAGS)
def test_process_batch_qmix_against_the_fed_arrays(tag, golden_dir):
    from cm3_amd.batch import process_batch_qmix
    z, index, cols = _load(golden_dir, tag)
    N = index["n_agents"]
    (n_steps, v_global, obs_others, v_local, a1, ao, reward, reward_local, v_global_next, obs_others_next, v_local_next, done,
     goals) = process_batch_qmix(cols)
    B = cols["v_global"].shape[0]
    assert n_steps == B
    _same(obs_others, z["c2_feed_obs_others"], "obs_others")
    _same(v_local, z["c2_feed_v_obs"], "v_local")
    _same(a1, z["c2_feed_actions_1hot"], "actions_1hot")
    _same(obs_others_next, z["c0_feed_obs_others"], "obs_others_next")
    _same(v_local_next, z["c0_feed_v_obs"], "v_local_next")
    _same(v_global.reshape(B, -1), z["c2_feed_v_state"], "state")
    _same(v_global_next.reshape(B, -1), z["c1_feed_v_state"], "state_next")
    _same(goals.reshape(B * N, -1), z["c0_feed_v_goal"], "goals_self")
    _same(goals.reshape(B, -1), z["c1_feed_v_goal_all"], "goals_all")
    # the reference's own shapes and dtypes for what train_step does not feed (alg_qmix.py:236-285)
    assert tuple(ao.shape) == (B * N, N - 1, 5) and ao.dtype == torch.float64
    _same(reward, np.repeat(z["in_reward"], N, axis=0), "reward")
    _same(reward_local, z["in_reward_local"].reshape(B * N), "reward_local")
    _same(done, z["in_done"], "done")                                        # per time step: NOT repeated (unlike alg_credit)
    _same(goals, z["in_goals"], "goals")


@pytest.mark.parametrize("N", [1, 4, 7, 8, 10, 15])
def test_row_sum_follows_numpy(N):
    from cm3_amd.batch import _row_sum_numpy_order
    rng = np.random.default_rng(N)
    x = rng.standard_normal((257, N)) * 10.0 ** rng.integers(-6, 6, (257, N))
    assert np.array_equal(_row_sum_numpy_order(torch.as_tensor(x)).numpy(), np.sum(x, axis=1))


@pytest.mark.parametrize("qdtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [1, 4, 8, 10])
def test_td_target_composition_equals_the_numpy_expression(N, qdtype):
    from cm3_amd.batch import qmix_td_target
    rng = np.random.default_rng(50 + N)
    n, gamma = 130, 0.99
    r = rng.standard_normal((n, N)) * 10.0 ** rng.integers(-3, 3, (n, N))
    q = rng.standard_normal((n, 1)).astype(qdtype)
    done = rng.random(n) < 0.3
    want = np.sum(r, axis=1) + gamma * np.squeeze(q) * (-(done - 1))
    _same(qmix_td_target(torch.as_tensor(r), torch.as_tensor(q), torch.as_tensor(done), gamma), want, "td_target")


def test_target_agent_refuses_host_columns(golden_dir):
    from cm3_amd.batch import qmix_train_step_feeds
    _, index, cols = _load(golden_dir, "n4")
    with pytest.raises(ValueError):
        qmix_train_step_feeds(cols, lambda ops, feed: [None], index["gamma"], target_agent=object())
