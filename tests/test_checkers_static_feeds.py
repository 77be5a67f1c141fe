"""CPU: the output list of cm3_amd.batch.checkers_static_feeds_device (checkers_static_feed_specs), evaluated with a NumPy
restatement of cm3_rows_tile's row formula (tests/rows_tile_ref.py), against the arrays the REAL alg_credit_checkers.train_step fed
(tests/golden/trainstep_checkers_n2.npz) and, at N = 3 (two other agents: the `others` mapping), against the torch composition."""
import json
import os

import numpy as np
import torch

from tests import rows_tile_ref as REF
from tests.helpers import GOLDEN


TD_ONLY = {"done_rep", "not_done", "nd_rep", "r_rep"}      # outputs that enter the TD targets, not a feed of their own


def _specs_and_static(cols, l_action=5):
    from cm3_amd import batch as BR
    specs = BR.checkers_static_feed_specs({n: tuple(v.shape) for n, v in cols.items()}, cols["goals"].dtype, l_action)
    return specs, REF.static_feeds(cols, specs)


def _tensor_feeds(calls):
    return sum(1 for _, feed in calls for v in feed.values() if torch.is_tensor(v))


def test_kind_numbers_are_the_library_s():
    from cm3_amd import _lib
    assert (REF.TILE_COPY, REF.TILE_F32_TO_F64, REF.TILE_ONEHOT_I64, REF.TILE_ONEHOT_F64, REF.TILE_EYE_F64, REF.TILE_NOT_I64) == (
        _lib.TILE_COPY, _lib.TILE_F32_TO_F64, _lib.TILE_ONEHOT_I64, _lib.TILE_ONEHOT_F64, _lib.TILE_EYE_F64, _lib.TILE_NOT_I64)


def test_specs_name_every_output_once_and_fit_three_launches():
    from cm3_amd import batch as BR
    shapes = dict(grid=(6, 3, 9, 2), vec=(6, 2, 4), obs_self_t=(6, 2, 5, 5, 3), obs_self_v=(6, 2, 4), goals=(6, 2, 2))
    specs = BR.checkers_static_feed_specs(shapes, torch.int64)
    names = [s.name for s in specs]
    assert len(set(names)) == len(names) == 33
    assert -(-len(specs) // 16) <= 3                                      # 16 outputs per launch of cm3_rows_tile
    by_name = {s.name: s for s in specs}
    assert by_name["state_env"].epr * 8 == 432 and by_name["cf_ot"].epr * 8 == 600      # the two wide rows
    assert by_name["cf_ot"].rows == 6 * 2 * 2 * 5 and by_name["cf_ot"].shape == (120, 5, 5, 3)
    for s in specs:
        want = s.shape if s.shape is not None else (s.rows, s.epr)
        assert int(np.prod(want)) == s.rows * s.epr, s.name


def test_specs_equal_the_real_train_step_feeds():
    """Every static feed, through train_step_feeds(static=...), equals the recorded c<k>_feed_<name> array in value, shape and dtype;
    the number compared is the number of tensor feeds of the composition's own call list (71 at this fixture, 11 calls)."""
    from cm3_amd import batch as BR
    z = np.load(os.path.join(GOLDEN, "trainstep_checkers_n2.npz"))
    meta = json.loads(str(z["index"]))
    cols = {k[3:]: torch.as_tensor(z[k]) for k in z.files if k.startswith("in_")}

    def session():
        it = iter(range(len(meta["calls"])))

        def run(ops, feed):
            c = next(it)
            entry = meta["calls"][c]
            assert ops == entry["ops"], (c, ops, entry["ops"])
            return [torch.as_tensor(z["c%d_res_%s" % (c, op)]) if op in entry["results"] else None for op in ops]
        return run

    spec_calls = BR.train_step_feeds(cols, session(), meta["gamma"], meta["epsilon"], env="checkers")
    assert len(spec_calls) == 11 and _tensor_feeds(spec_calls) == 71
    specs, S = _specs_and_static(cols)
    calls = BR.train_step_feeds(cols, session(), meta["gamma"], meta["epsilon"], env="checkers", static=S)
    assert [c[0] for c in calls] == [e["ops"] for e in meta["calls"]] and len(calls) == 11
    n_arrays, fed = 0, set()
    for c, ((ops, feed), entry) in enumerate(zip(calls, meta["calls"])):
        assert sorted(feed) == entry["feed"], (c, ops)
        for k, v in feed.items():
            want = z["c%d_feed_%s" % (c, k)]
            got = v.numpy() if torch.is_tensor(v) else np.asarray(v)
            assert got.shape == want.shape and got.dtype == want.dtype, (c, ops, k, got.shape, want.shape, got.dtype, want.dtype)
            assert np.array_equal(got, want), (c, ops, k)
            if torch.is_tensor(v):
                n_arrays += 1
                fed.update(name for name, t in S.items() if t is v)
    assert n_arrays == 71
    # every output of the list is fed as it is, but the four that only enter the TD targets (checked through those, and here)
    assert fed == set(S) - TD_ONLY
    done, r_local = z["in_done"], z["in_local_rewards"]
    assert np.array_equal(S["done_rep"].numpy(), np.repeat(done, 2)) and S["done_rep"].dtype == torch.bool
    assert np.array_equal(S["not_done"].numpy(), 1 - np.repeat(done, 2).astype(np.int64)) and S["not_done"].dtype == torch.int64
    assert np.array_equal(S["nd_rep"].numpy(), 1 - np.repeat(done, 4).astype(np.int64)) and S["nd_rep"].dtype == torch.int64
    assert np.array_equal(S["r_rep"].numpy(), np.repeat(r_local.reshape(-1, 1, 2), 2, axis=1).reshape(-1))


def test_specs_equal_the_composition_at_three_agents():
    from cm3_amd import batch as BR
    B, N = 7, 3
    g = torch.Generator().manual_seed(11)
    f = lambda *s: torch.randint(-3, 4, s, generator=g).to(torch.float64) + torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    cols = dict(grid=f(B, 3, 9, 2), vec=f(B, N, 4), obs_others=f(B, N, 2 * (N - 1)), obs_self_t=f(B, N, 5, 5, 3), obs_self_v=f(B, N, 4),
                actions_prev=torch.randint(0, 5, (B, N), generator=g, dtype=torch.int32),
                actions=torch.randint(0, 5, (B, N), generator=g, dtype=torch.int32), reward=f(B), local_rewards=f(B, N),
                next_grid=f(B, 3, 9, 2), next_vec=f(B, N, 4), next_obs_others=f(B, N, 2 * (N - 1)), next_obs_self_t=f(B, N, 5, 5, 3),
                next_obs_self_v=f(B, N, 4), done=torch.rand(B, generator=g) < 0.4,
                goals=torch.nn.functional.one_hot(torch.randint(0, 2, (B, N), generator=g), 2))
    assert cols["goals"].dtype == torch.int64 and bool(cols["done"].any()) and not bool(cols["done"].all())

    def session():
        gg = torch.Generator().manual_seed(5)

        def run(ops, feed):
            rows = max([v.shape[0] for v in feed.values() if torch.is_tensor(v) and v.dim() > 0] or [1])
            outs = []
            for op in ops:
                if op.endswith("_op") or op == "list_update_target_ops":
                    outs.append(None)
                elif op == "action_samples_target":
                    outs.append(torch.randint(0, 5, (B * N,), generator=gg))
                elif op == "probs":
                    outs.append(torch.rand(rows, 5, generator=gg, dtype=torch.float64))
                else:
                    outs.append(torch.rand(rows, generator=gg, dtype=torch.float64))
            return outs
        return run

    specs, S = _specs_and_static(cols)
    a = BR.train_step_feeds(cols, session(), 0.99, 0.1, env="checkers", static=S)
    b = BR.train_step_feeds(cols, session(), 0.99, 0.1, env="checkers")
    assert [c[0] for c in a] == [c[0] for c in b] and len(a) == 11
    n, fed = 0, set()
    for (ops, fa), (_, fb) in zip(a, b):
        assert sorted(fa) == sorted(fb), ops
        for k in fb:
            if torch.is_tensor(fb[k]):
                assert fa[k].dtype == fb[k].dtype and fa[k].shape == fb[k].shape, (ops, k, fa[k].dtype, fb[k].dtype, fa[k].shape, fb[k].shape)
                assert torch.equal(fa[k], fb[k]), (ops, k)
                n += 1
                fed.update(name for name, t in S.items() if t is fa[k])
            else:
                assert fa[k] == fb[k]
    assert n == _tensor_feeds(b) == 71 and fed == set(S) - TD_ONLY
