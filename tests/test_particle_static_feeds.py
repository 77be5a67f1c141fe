"""CPU: the output list of cm3_amd.batch.particle_static_feeds_device (particle_static_feed_specs), evaluated with a NumPy
restatement of cm3_rows_tile's row formula (tests/rows_tile_ref.py), against the arrays the REAL alg_credit.train_step fed
(tests/golden/trainstep_particle_n4.npz) and, at N = 3 (two other agents: the `others` mapping), against the torch composition."""
import json
import os

import numpy as np
import torch

from tests import rows_tile_ref as REF
from tests.helpers import GOLDEN


# outputs that are no feed of their own: reward_rep / done_rep are the `reward` / `done` of process_batch's tuple, which train_step
# never feeds; not_done, nd_rep and r_rep enter the TD targets
TD_ONLY = {"reward_rep", "done_rep", "not_done", "nd_rep", "r_rep"}
SPEC_NAMES = ("v_global", "goals", "reward", "reward_local")


def particle_cols(B, N, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    f = lambda *s: (torch.randint(-3, 4, s, generator=g).to(dtype) + torch.rand(*s, generator=g, dtype=dtype))      # noqa: E731
    cols = dict(v_global=f(B, N, 4), obs_others=f(B, N, 4 * (N - 1)), v_local=f(B, N, 4),
                actions=torch.randint(0, 5, (B, N), generator=g, dtype=torch.int32), reward=f(B), reward_local=f(B, N),
                v_global_next=f(B, N, 4), obs_others_next=f(B, N, 4 * (N - 1)), v_local_next=f(B, N, 4),
                done=torch.rand(B, generator=g) < 0.4, goals=f(B, N, 2))
    assert bool(cols["done"].any()) and not bool(cols["done"].all())
    return cols


def specs_and_static(cols, l_action=5):
    from cm3_amd import batch as BR
    specs = BR.particle_static_feed_specs({n: tuple(cols[n].shape) for n in SPEC_NAMES}, {n: cols[n].dtype for n in SPEC_NAMES}, l_action)
    return specs, REF.static_feeds(cols, specs)


def _tensor_feeds(calls):
    return sum(1 for _, feed in calls for v in feed.values() if torch.is_tensor(v))


def test_specs_name_every_output_once_and_fit_two_launches():
    from cm3_amd import batch as BR
    specs = BR.particle_static_feed_specs(dict(v_global=(6, 3, 4), goals=(6, 3, 2)), {n: torch.float32 for n in SPEC_NAMES})
    names = [s.name for s in specs]
    assert len(set(names)) == len(names) == 22
    assert -(-len(specs) // 16) <= 2                                      # 16 outputs per launch of cm3_rows_tile
    assert names[16] == "a1_rep_m" and names[:2] == ["a1", "ao"]          # the sixteen of the first launch, then the six of the second
    for s in specs:
        want = s.shape if s.shape is not None else (s.rows, s.epr)
        assert int(np.prod(want)) == s.rows * s.epr, s.name
    by_name = {s.name: s for s in specs}
    assert by_name["cf_s_others"].rows == 6 * 3 * 3 * 5 * 2 and by_name["cf_s_others"].shape == (270, 8)


def test_copies_keep_the_dtypes_of_their_columns():
    from cm3_amd import batch as BR
    dtypes = dict(v_global=torch.float32, goals=torch.int64, reward=torch.float64, reward_local=torch.float32)
    by_name = {s.name: s for s in BR.particle_static_feed_specs(dict(v_global=(2, 2, 4), goals=(2, 2, 2)), dtypes)}
    assert by_name["reward_rep"].dtype == torch.float64 and by_name["r_rep"].dtype == torch.float32
    assert by_name["goals_self_rep"].dtype == by_name["cf_goals"].dtype == torch.int64
    assert by_name["s_n_rep"].dtype == by_name["cf_s_m"].dtype == by_name["one_next_rep_n"].dtype == torch.float32
    assert by_name["others"].dtype == by_name["cf_s_others"].dtype == by_name["cf_eye"].dtype == torch.float64


def test_specs_equal_the_real_train_step_feeds():
    """Every static feed, through train_step_feeds(static=...), equals the recorded c<k>_feed_<name> array in value, shape and dtype;
    the number compared is the number of tensor feeds of the composition's own call list (48 at eleven calls: 3 + 5 + 6 + 5 + 6 + 3 +
    4 + 3 + 5 + 8, epsilon being a float)."""
    from cm3_amd import batch as BR
    z = np.load(os.path.join(GOLDEN, "trainstep_particle_n4.npz"))
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

    spec_calls = BR.train_step_feeds(cols, session(), meta["gamma"], meta["epsilon"])
    assert len(spec_calls) == 11
    n_composed = _tensor_feeds(spec_calls)
    specs, S = specs_and_static(cols)
    calls = BR.train_step_feeds(cols, session(), meta["gamma"], meta["epsilon"], static=S)
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
    assert n_arrays == n_composed == 48
    assert fed == set(S) - TD_ONLY
    # the five that are no feed of their own, directly
    done, reward, r_local = z["in_done"], z["in_reward"], z["in_reward_local"]
    assert np.array_equal(S["reward_rep"].numpy(), np.repeat(reward, 4)) and S["reward_rep"].dtype == torch.float64
    assert np.array_equal(S["done_rep"].numpy(), np.repeat(done, 4)) and S["done_rep"].dtype == torch.bool
    assert np.array_equal(S["not_done"].numpy(), 1 - np.repeat(done, 4).astype(np.int64)) and S["not_done"].dtype == torch.int64
    assert np.array_equal(S["nd_rep"].numpy(), 1 - np.repeat(done, 16).astype(np.int64)) and S["nd_rep"].dtype == torch.int64
    assert np.array_equal(S["r_rep"].numpy(), np.repeat(r_local.reshape(-1, 1, 4), 4, axis=1).reshape(-1))


def test_specs_equal_the_composition_at_three_agents():
    """Seeded float32 columns on the CPU: `b` goes through the torch composition, `a` through the spec dict."""
    from cm3_amd import batch as BR
    B, N = 7, 3
    cols = particle_cols(B, N, seed=11)

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

    specs, S = specs_and_static(cols)
    a = BR.train_step_feeds(cols, session(), 0.99, 0.1, static=S)
    b = BR.train_step_feeds(cols, session(), 0.99, 0.1)
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
    assert n == _tensor_feeds(b) == 48 and fed == set(S) - TD_ONLY
