"""GPU: the row-granular path of cm3_rows_tile (wide CM3_TILE_COPY rows: a group of lanes per row, 16- / 8-byte units) against torch
indexing, and the Checkers train-step feeds built with it -- cm3_amd.batch.checkers_static_feeds_device, train_step_feeds(env="checkers",
static=...), CheckersRollout.on_policy_phase, OnPolicyPhasePlan over a CheckersRollout -- against the arrays the REAL
alg_credit_checkers.train_step fed (tests/golden/trainstep_checkers_n2.npz) and against the torch composition (device_tiling=False),
which tests/test_batch.py pins to the same arrays."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import rows_tile_ref as REF
from tests.helpers import GOLDEN, ROOT, band_init, load_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _row_threshold():
    """kTileRowMinBytes of csrc/batch.hip: the row size from which a COPY column takes the row path"""
    src = open(os.path.join(ROOT, "cm3_amd", "csrc", "batch.hip")).read()
    return int(re.search(r"constexpr uint32_t kTileRowMinBytes = (\d+);", src).group(1))


def _offset_view(n, dtype, gen, offset_elems):
    """a contiguous [n] view `offset_elems` elements into a fresh (at least 16-byte aligned) allocation"""
    raw = torch.randint(-1000, 1000, (n + 4,), generator=gen, device=DEV).to(dtype)
    assert raw.data_ptr() % 16 == 0
    return raw[offset_elems:offset_elems + n]


def _kernel_cases(gen):
    """(label, source [S, epr], destination rows, terms, others): every row size of the table, both sides of the threshold"""
    T = _row_threshold()
    assert T % 8 == 0 and T >= 16
    sizes = sorted({16, 32, 216, 432, 600, T - 16, T - 8, T, T + 8, T + 16} - {0, 8})
    cases = []
    for rb in sizes:
        for rows in (1, 37, 301):          # 301: no multiple of the 4 .. 256 rows a workgroup serves at any of these sizes
            S = 5
            src = _offset_view(S * (rb // 8), torch.float64, gen, 0).reshape(S, rb // 8)
            # one row repeated; or two remainder terms: row r <- row ((r / 14) % 2) * 2 + (r / 7) % 2
            cases.append(("f64 %d B x %d rep" % (rb, rows), src, rows, ((3, 0, 1), (1, 0, 0)), None) if rows == 1 else
                         ("f64 %d B x %d mix" % (rb, rows), src, rows, ((14, 2, 2), (7, 2, 1)), None))
    # narrower elements on the row path: 4-byte and 1-byte sources, rows of whole 8-byte units from the threshold on
    cases.append(("i32 row", _offset_view(8 * (T + 24) // 4, torch.int32, gen, 0).reshape(8, (T + 24) // 4), 37, ((5, 0, 1), (1, 0, 0)), None))
    cases.append(("u8 row", _offset_view(8 * (T + 8), torch.uint8, gen, 0).reshape(8, T + 8), 37, ((5, 0, 1), (1, 0, 0)), None))
    cases.append(("u8 odd row", _offset_view(8 * (T + 3), torch.uint8, gen, 0).reshape(8, T + 3), 37, ((5, 0, 1), (1, 0, 0)), None))     # element path
    # the `others` mapping at N = 3 (rows (b, m, n, k) <- row b N + [the k-th agent other than n]), COPY kind, wide rows
    N, B = 3, 4
    for rb in (432, 600):
        src = _offset_view(B * N * (rb // 8), torch.float64, gen, 0).reshape(B * N, rb // 8)
        cases.append(("others %d B" % rb, src, B * N * N * (N - 1), None, (N, N * N * (N - 1), N - 1)))
    # a source view that is only 8-byte aligned: the element path, same result
    src = _offset_view(6 * 54, torch.float64, gen, 1).reshape(6, 54)
    assert src.data_ptr() % 16 == 8
    cases.append(("8-byte aligned source", src, 37, ((7, 0, 1), (1, 0, 0)), None))
    return cases


def _run_kernel_cases():
    from cm3_amd import _lib
    from cm3_amd.batch import _Tiler
    gen = torch.Generator(device=DEV).manual_seed(21)
    cases = _kernel_cases(gen)
    t = _Tiler(DEV)
    outs = []
    for i, (label, src, rows, terms, others) in enumerate(cases):
        kw = dict(others=others) if others is not None else dict(terms=terms)
        assert int(REF.source_rows(rows, terms, others).max()) < src.shape[0], label      # (the kernel does not check f(r): the caller does)
        out = None
        if label.startswith("f64 600 B x 37"):            # ... and a destination that is only 8-byte aligned
            out = _offset_view(rows * src.shape[1], src.dtype, gen, 1).reshape(rows, src.shape[1])
            assert out.data_ptr() % 16 == 8
        outs.append(t.add(src, rows, src.shape[1], src.dtype, _lib.TILE_COPY, out=out, **kw))
        if i == 2:                                        # a zero-row column in the same launch as non-empty ones
            empty = t.add(src, 0, src.shape[1], src.dtype, _lib.TILE_COPY, terms=terms)
            assert empty.numel() == 0
    assert len(t.specs) > 32                              # several launches, every one with columns of both paths
    t.run()
    torch.cuda.synchronize()
    width = _lib.rows_last_index_width()
    for (label, src, rows, terms, others), got in zip(cases, outs):
        f = torch.as_tensor(REF.source_rows(rows, terms, others), device=DEV)
        assert got.shape == (rows, src.shape[1]) and got.dtype == src.dtype, label
        assert torch.equal(got, src[f]), label
    return width


def test_row_path_equals_torch_indexing():
    assert _run_kernel_cases() == 32


def test_row_path_in_the_wide_index_build():
    from cm3_amd import _lib
    _lib.check(_lib.lib().cm3_rows_force_index_width(64))
    try:
        assert _run_kernel_cases() == 64
    finally:
        _lib.check(_lib.lib().cm3_rows_force_index_width(0))
    assert _run_kernel_cases() == 32


# ---- the feeds ------------------------------------------------------------------------------------------------------------------
def _tensor_feeds(calls):
    return sum(1 for _, feed in calls for v in feed.values() if torch.is_tensor(v))


def _assert_same_feeds(a, b, what):
    assert [c[0] for c in a] == [c[0] for c in b], what
    n = 0
    for (ops, fa), (_, fb) in zip(a, b):
        assert sorted(fa) == sorted(fb), (what, ops)
        for k in fb:
            if torch.is_tensor(fb[k]):
                assert fa[k].dtype == fb[k].dtype and fa[k].shape == fb[k].shape, (what, ops, k, fa[k].dtype, fb[k].dtype, fa[k].shape, fb[k].shape)
                assert torch.equal(fa[k], fb[k]), (what, ops, k)
                n += 1
            else:
                assert fa[k] == fb[k], (what, ops, k)
    assert n == _tensor_feeds(b)
    return n


def _make_run(n_agent_rows, seed=5):
    g = torch.Generator(device=DEV).manual_seed(seed)

    def run(ops, feed):
        rows = max([v.shape[0] for v in feed.values() if torch.is_tensor(v) and v.dim() > 0] or [1])
        outs = []
        for op in ops:
            if op.endswith("_op") or op == "list_update_target_ops":
                outs.append(None)
            elif op == "action_samples_target":
                outs.append(torch.randint(0, 5, (n_agent_rows,), generator=g, device=DEV))
            elif op == "probs":
                outs.append(torch.rand(rows, 5, generator=g, device=DEV, dtype=torch.float64))
            else:
                outs.append(torch.rand(rows, generator=g, device=DEV, dtype=torch.float64))
        return outs
    return run


def test_golden_feeds_on_the_device():
    """The recorded inputs on the device (actions int32, goals as recorded), static feeds from checkers_static_feeds_device: every feed
    of every call equals the array the REAL train_step fed; 71 tensors over 11 calls, counted on the composition's own call list."""
    from cm3_amd import batch as BR
    z = np.load(os.path.join(GOLDEN, "trainstep_checkers_n2.npz"))
    meta = json.loads(str(z["index"]))
    host = {k[3:]: torch.as_tensor(z[k]) for k in z.files if k.startswith("in_")}

    def session(device):
        it = iter(range(len(meta["calls"])))

        def run(ops, feed):
            c = next(it)
            entry = meta["calls"][c]
            assert ops == entry["ops"], (c, ops, entry["ops"])
            return [torch.as_tensor(z["c%d_res_%s" % (c, op)]).to(device) if op in entry["results"] else None for op in ops]
        return run

    want_calls = BR.train_step_feeds(host, session("cpu"), meta["gamma"], meta["epsilon"], env="checkers")      # the composition, on the CPU
    n_want = _tensor_feeds(want_calls)
    assert n_want == 71 and len(want_calls) == 11
    cols = {k: v.to(DEV) for k, v in host.items()}
    cols["actions"], cols["actions_prev"] = cols["actions"].to(torch.int32), cols["actions_prev"].to(torch.int32)
    static = BR.checkers_static_feeds_device(cols)
    calls = BR.train_step_feeds(cols, session(DEV), meta["gamma"], meta["epsilon"], env="checkers", static=static)
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == [e["ops"] for e in meta["calls"]] and len(calls) == 11
    n = 0
    for c, ((ops, feed), entry) in enumerate(zip(calls, meta["calls"])):
        assert sorted(feed) == entry["feed"], (c, ops)
        for k, v in feed.items():
            want = z["c%d_feed_%s" % (c, k)]
            got = v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
            assert got.shape == want.shape and got.dtype == want.dtype, (c, ops, k, got.shape, want.shape, got.dtype, want.dtype)
            assert np.array_equal(got, want), (c, ops, k)
            n += int(torch.is_tensor(v))
    assert n == n_want
    # the default path is this one: the same tensors' values without static=
    _assert_same_feeds(BR.train_step_feeds(cols, session(DEV), meta["gamma"], meta["epsilon"], env="checkers"), calls, "default")
    # out=: the same tensors are written again
    again = BR.checkers_static_feeds_device(cols, out=static)
    assert sorted(again) == sorted(static) and all(again[k].data_ptr() == static[k].data_ptr() for k in static)


def _stage2_rollout(E=64, T=40):
    from cm3_amd.checkers import VecCheckersEnv
    from cm3_amd.rollout import CheckersRollout
    cfg = load_cfg("checkers_stage2.json")
    env = VecCheckersEnv(cfg["init"], cfg["n_agents"], 9, E, device=DEV, seed=31, auto_reset=True)
    assert cfg["n_agents"] == 2
    return CheckersRollout(env, n_ticks=T, use_graph=False).collect(goals=np.eye(2))


def _band3_rollout(E=16, T=20):
    from cm3_amd.checkers import VecCheckersEnv
    from cm3_amd.rollout import CheckersRollout
    N = 3
    env = VecCheckersEnv(band_init(N, 300 + N), N, 9, E, device=DEV, seed=32, auto_reset=True)
    return CheckersRollout(env, n_ticks=T, use_graph=False).collect(goals=np.eye(2)[np.arange(N) % 2])


@pytest.mark.parametrize("source", ["n2_sample37", "n2_all", "n3_sample37"])
def test_device_tiling_equals_the_composition(source):
    from cm3_amd import batch as BR
    ro = _band3_rollout() if source.startswith("n3") else _stage2_rollout()
    gen = torch.Generator(device=DEV).manual_seed(2)
    cols = ro.as_reference_batch(numpy=False) if source == "n2_all" else ro.sample_batch(37, generator=gen, numpy=False)
    B, N = cols["vec"].shape[0], cols["vec"].shape[1]
    assert B == (64 * 40 if source == "n2_all" else 37) and N == (3 if source.startswith("n3") else 2)
    assert bool(cols["done"].any()) and cols["goals"].dtype == torch.int64 and cols["actions"].dtype == torch.int32
    static = BR.checkers_static_feeds_device(cols)
    a = BR.train_step_feeds(cols, _make_run(B * N), 0.99, 0.1, env="checkers", static=static)
    b = BR.train_step_feeds(cols, _make_run(B * N), 0.99, 0.1, env="checkers", device_tiling=False)
    torch.cuda.synchronize()
    assert _assert_same_feeds(a, b, source) == 71 and len(a) == 11
    fed = {name for name, t in static.items() for _, feed in a for v in feed.values() if v is t}
    assert fed == set(static) - {"done_rep", "not_done", "nd_rep", "r_rep"}         # (those four enter the TD targets only)
    ro.close()


def test_phase_feeds_equal_per_minibatch_composition():
    from cm3_amd import batch as BR
    ro = _stage2_rollout()
    pairs = ro.on_policy_phase(epochs=5, batch_size=37, generator=torch.Generator(device=DEV).manual_seed(4))
    assert len(pairs) == 5 and all(s is not None for _, s in pairs)
    checked = 0
    for cols, static in pairs:
        assert cols["vec"].shape[0] == 37
        a = BR.train_step_feeds(cols, _make_run(74, 6), 0.99, 0.1, env="checkers", static=static)
        b = BR.train_step_feeds(cols, _make_run(74, 6), 0.99, 0.1, env="checkers", device_tiling=False)
        checked += _assert_same_feeds(a, b, "phase")
    assert checked == 5 * 71
    # the five minibatches are views of one export and of one set of tiling outputs
    base = pairs[0][1]["cf_ot"]
    assert pairs[1][1]["cf_ot"].data_ptr() == base.data_ptr() + base.numel() * 8
    ro.close()


def test_phase_plan_over_a_checkers_rollout():
    """OnPolicyPhasePlan over a CheckersRollout: two phases into the same tensors and graphs, every replayed minibatch equal to the
    eager composition on clones of its columns."""
    from cm3_amd import batch as BR
    ro = _stage2_rollout()
    M, K, N = 4, 29, 2
    R = K * N
    bufs = {"acts": torch.zeros(R, dtype=torch.int64, device=DEV), "probs": torch.zeros(R, 5, dtype=torch.float64, device=DEV),
            "q": torch.zeros(R * N * 5, dtype=torch.float64, device=DEV)}

    def run(ops, feed):                      # (outputs live in fixed buffers: a captured consumer reads the same addresses every replay)
        rows = max([v.shape[0] for v in feed.values() if torch.is_tensor(v) and v.dim() > 0] or [1])
        outs = []
        for op in ops:
            if op.endswith("_op") or op == "list_update_target_ops":
                outs.append(None)
            elif op == "action_samples_target":
                outs.append(bufs["acts"])
            elif op == "probs":
                outs.append(bufs["probs"])
            else:
                outs.append(bufs["q"][:rows])
        return outs

    plan = BR.OnPolicyPhasePlan(ro, run, 0.99, 0.1, epochs=M, batch_size=K)
    g = torch.Generator(device=DEV).manual_seed(9)
    ptrs = None
    for phase in range(2):
        ro.collect()
        bufs["acts"].copy_(torch.randint(0, 5, (R,), generator=g, device=DEV))
        bufs["probs"].copy_(torch.rand(R, 5, generator=g, device=DEV, dtype=torch.float64))
        bufs["q"].copy_(torch.rand(R * N * 5, generator=g, device=DEV, dtype=torch.float64))
        plan.refresh(g)
        now = ({k: v.data_ptr() for k, v in plan.cols.items()}, {k: v.data_ptr() for k, v in plan.static.items()})
        ptrs = ptrs or now
        assert ptrs == now                                                      # columns and feeds are persistent
        checked = 0
        for k in range(M):
            calls = plan.step(k)
            torch.cuda.synchronize()
            cols, _ = plan.minibatch(k)
            want = BR.train_step_feeds({n: v.clone() for n, v in cols.items()}, run, 0.99, 0.1, env="checkers", device_tiling=False)
            checked += _assert_same_feeds(calls, want, (phase, k))
        assert checked == M * 71
    assert len(plan._graphs) == M
    plan.close()
    assert plan._graphs == {} and plan._calls == {}
    ro.close()
