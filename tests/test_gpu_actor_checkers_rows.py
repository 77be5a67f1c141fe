"""GPU: the CM3 Checkers actor over transition rows (cm3_actor_checkers_rows_f32; CheckersActor.probs_rows / sample_rows) against
the collection kernels it shares its layers with, the NumPy restatement of its draw (tests/actor_rows_ref.py), the float64
restatement of the network (oracle/actor_checkers_oracle.py) and the reference-derived network fixture; train_step_feeds(env=
"checkers") with device actors against its torch specification and the feeds the reference's own train_step built; the soft update
of the target actor."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import actor_checkers_oracle as AO
from tests import actor_rows_ref as RR
from tests.test_gpu_actor_checkers_f64 import _synthetic_rows
from tests.test_oracle_actor_golden import load_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 77
KERNEL = {"f32": "k_ck_actor_rows<", "bf16": "k_ck_actor_rows<", "f16x3": "k_ck_actor_rows_x3<"}
CONFIGS = [(1, 1), (1, 2)] + [(N, 2) for N in range(2, 9)]                  # (agents, stage): stage 1 at N = 1, 2 otherwise, and N = 1 at 2


def _stage(N):
    return 1 if N == 1 else 2


def _actor(N, stage=None, precision="f32", wseed=None, seed=SEED):
    from cm3_amd.actor import CheckersActor
    stage = _stage(N) if stage is None else stage
    w = AO.init_weights(np.random.default_rng(100 + N if wseed is None else wseed), N, stage=stage)
    return CheckersActor(w, N, stage=stage, device=DEV, seed=seed, precision=precision), w


def _dev(x):
    return torch.as_tensor(x, device=DEV)


def _random_rows(N, R, rseed):
    """wide-form rows as NumPy arrays: float64 windows in {-1, 0, 1}, float64 obs_self_v / obs_others, actions_prev, one-hot goals"""
    rng = np.random.default_rng(rseed)
    Lo = 2 * max(N - 1, 1)
    return dict(obs_self_t=rng.integers(-1, 2, (R, 5, 5, 3)).astype(np.float64), obs_self_v=rng.uniform(-0.5, 1.0, (R, 4)),
                obs_others=rng.uniform(-1, 1, (R, Lo)), actions_prev=rng.integers(0, 5, R), goals=np.eye(2)[rng.integers(0, 2, R)])


def _args(rows):
    """the five inputs in the order the rows methods take them"""
    return tuple(rows[k] if torch.is_tensor(rows[k]) else _dev(rows[k])
                 for k in ("obs_self_t", "obs_self_v", "obs_others", "actions_prev", "goals"))


_BLOCK = {}


def _collection(N, stage, E, precision):
    """(actor, narrow rows, wide rows, probs) of the collection kernel (actor.enqueue at epsilon 0.3, prev_done = None) on
    _synthetic_rows and the very same tensors viewed as transition rows -- computed once per key and left unchanged."""
    key = (N, stage, E, precision)
    if key not in _BLOCK:
        inp = _synthetic_rows(N, E, 75 * N, np.random.default_rng(900 + N))
        actor, _ = _actor(N, stage, precision)
        actions = torch.empty(E, N, dtype=torch.int32, device=DEV)
        probs = torch.empty(E, N, 5, dtype=torch.float32, device=DEV)
        actor.enqueue(E, inp["raw"], inp["stride"], inp["obs_self_v"], inp["obs_others"], inp["goals"], inp["actions_prev"],
                      inp["steps"], inp["episode"], actions, 0.3, probs=probs, prev_done=None)
        R = E * N
        narrow = dict(obs_self_t=inp["raw"].view(R, 75), obs_self_v=inp["obs_self_v"].view(R, 4),
                      obs_others=inp["obs_others"].view(R, -1), actions_prev=inp["actions_prev"].view(R), goals=inp["goals"].view(R))
        wide = dict(narrow, obs_self_t=narrow["obs_self_t"].double(),
                    goals=torch.nn.functional.one_hot(narrow["goals"].long(), 2).contiguous())
        torch.cuda.synchronize()
        _BLOCK[key] = (actor, narrow, wide, probs.view(R, 5))
    return _BLOCK[key]


# ---- 1. the bits of the collection kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16"])
@pytest.mark.parametrize("N,stage", CONFIGS)
def test_rows_kernel_gives_the_bits_of_the_collection_kernel(N, stage, precision):
    from cm3_amd import _lib
    E = 201                                                  # E * N mod 64: 9, 18, 27, 36, 45, 54, 63, 8 -- ragged at every N
    assert (E * N) % 64 != 0
    actor, narrow, wide, p_act = _collection(N, stage, E, precision)
    assert narrow["obs_self_t"].dtype == torch.int8 and narrow["goals"].dtype == torch.uint8
    assert wide["obs_self_t"].dtype == torch.float64 and wide["goals"].dtype == torch.int64
    assert len(torch.unique(p_act)) > 5
    for form, rows in (("narrow", narrow), ("wide", wide)):
        lead = lambda t: t.view(E, N, *t.shape[1:])          # noqa: E731  (any leading shape)
        out = actor.sample_rows(*(lead(t) for t in _args(rows)), 0.3, probs=True)
        torch.cuda.synchronize()
        v = _lib.last_kernel_variant()
        assert v.startswith(KERNEL[precision]) and (",N=%d," % N) in v and v.endswith(",prec=%s>" % precision), v
        assert (",g=%d," % (3 if form == "wide" else 0)) in v, v
        assert out["probs"].dtype == torch.float32 and tuple(out["probs"].shape) == (E * N, 5)
        assert out["actions"].dtype == torch.int32 and tuple(out["actions"].shape) == (E * N,)
        assert torch.equal(out["probs"].view(torch.int32), p_act.view(torch.int32)), form       # bit for bit


@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16"])
def test_one_agent_reads_obs_others_at_stage_2_only(precision):
    rows = _random_rows(1, 201, 17)
    moved = dict(rows, obs_others=rows["obs_others"] + 0.5)
    for stage in (1, 2):
        actor, _ = _actor(1, stage, precision)
        a, b = actor.probs_rows(*_args(rows), 0.3), actor.probs_rows(*_args(moved), 0.3)
        torch.cuda.synchronize()
        assert torch.equal(a, b) == (stage == 1), stage


# ---- 2. edges: ragged counts, rows past n_rows, every output alone ------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_row_counts_and_single_outputs(N, n_rows, precision):
    E = -(-256 // N)                                                        # a block of at least 256 rows: rows past n_rows exist
    actor, narrow, wide, p_act = _collection(N, _stage(N), E, precision)
    spec = {"probs": ((n_rows + 1, 5), torch.float32, -12345.0), "actions": ((n_rows + 1,), torch.int32, -7),
            "onehot": ((n_rows + 1, 5), torch.int64, -7)}
    fresh = lambda: {k: torch.full(shape, fill, dtype=dt, device=DEV) for k, (shape, dt, fill) in spec.items()}    # noqa: E731
    for form, clean in (("narrow", narrow), ("wide", wide)):
        want = fresh()                                                      # the unpoisoned run, all three outputs in one launch
        actor.enqueue_rows(n_rows, *(clean[k][:256].contiguous() for k in ("obs_self_t", "obs_self_v", "obs_others", "actions_prev",
                                                                           "goals")), 0.3, draw=5, **want)
        torch.cuda.synchronize()
        assert torch.equal(want["probs"][:n_rows].view(torch.int32), p_act[:n_rows].view(torch.int32)), form
        u = RR.rows_uniforms(SEED, n_rows, 5)
        assert np.array_equal(want["actions"][:n_rows].cpu().numpy(), AO.sample_actions(p_act[:n_rows].cpu().numpy(), u)), form
        assert torch.equal(want["onehot"][:n_rows], torch.nn.functional.one_hot(want["actions"][:n_rows].long(), 5)), form
        # rows at or past n_rows hold values that would change a live row if they were read into it
        rows = {k: v[:256].clone() for k, v in clean.items()}
        rows["obs_self_t"][n_rows:] = 5
        rows["actions_prev"][n_rows:] = 4
        rows["obs_self_v"][n_rows:] = 1000.0
        rows["obs_others"][n_rows:] = -1000.0
        rows["goals"][n_rows:] = 1 - rows["goals"][n_rows:]
        for name in spec:                                                   # three launches, each writing only its own buffer
            bufs = fresh()
            actor.enqueue_rows(n_rows, rows["obs_self_t"], rows["obs_self_v"], rows["obs_others"], rows["actions_prev"],
                               rows["goals"], 0.3, draw=5, **{name: bufs[name]})
            torch.cuda.synchronize()
            for k, (shape, dt, fill) in spec.items():
                if k == name:
                    assert torch.equal(bufs[k][:n_rows], want[k][:n_rows]), (form, name, k)
                    assert bool((bufs[k][n_rows:] == fill).all()), (form, name, k)    # the extra row is untouched
                else:
                    assert bool((bufs[k] == fill).all()), (form, name, k)


# ---- 3. sampling is exact against the restated stream -------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("N", [1, 2, 5])
def test_sampling_is_exact_against_the_restated_stream(N, eps):
    R = 1000
    actor, _ = _actor(N)
    rows = _args(_random_rows(N, R, 40 + N))
    assert actor.rows_draw == 0
    first = actor.sample_rows(*rows, eps, probs=True, onehot=True)
    second = actor.sample_rows(*rows, eps, probs=True)
    again = actor.sample_rows(*rows, eps, probs=True, draw=0)
    torch.cuda.synchronize()
    assert actor.rows_draw == 2                                              # one per call; an explicit draw leaves the counter alone
    assert first["actions"].dtype == torch.int32 and tuple(first["actions"].shape) == (R,)
    probs = first["probs"].cpu().numpy()
    for k, out in enumerate((first, second)):
        # the pick is a float32 inverse CDF over the device's own float32 probabilities: every row, nothing to tolerate
        assert torch.equal(out["probs"], first["probs"])
        assert np.array_equal(out["actions"].cpu().numpy(), AO.sample_actions(probs, RR.rows_uniforms(SEED, R, k))), k
    assert first["onehot"].dtype == torch.int64
    assert torch.equal(first["onehot"], torch.nn.functional.one_hot(first["actions"].long(), 5))
    assert not torch.equal(first["actions"], second["actions"])
    assert torch.equal(again["actions"], first["actions"])
    assert len(torch.unique(first["actions"])) > 1
    # a row id base shifts the stream: rows 100.. of base 0 are rows 0.. of base 100
    shifted = torch.empty(R - 100, dtype=torch.int32, device=DEV)
    ot, ov, oo, ap, vg = rows
    tail = (t[100:].contiguous() for t in (ot.reshape(R, 75), ov, oo, ap.int(), vg.long()))     # the forms the raw launch reads
    actor.enqueue_rows(R - 100, *tail, eps, actions=shifted, draw=0, row_id_base=100)
    torch.cuda.synchronize()
    assert np.array_equal(shifted.cpu().numpy(), AO.sample_actions(probs[100:], RR.rows_uniforms(SEED, R - 100, 0, row_id_base=100)))
    assert torch.equal(shifted, first["actions"][100:])


def test_epsilon_from_the_device_is_the_epsilon_of_the_descriptor():
    N, R = 2, 130
    actor, _ = _actor(N)
    rows = _args(_random_rows(N, R, 3))
    eps_dev = torch.tensor([0.3], dtype=torch.float32, device=DEV)
    a, b = actor.probs_rows(*rows, 0.3), actor.probs_rows(*rows, eps_dev)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, actor.probs_rows(*rows, 0.0))


# ---- 4. against the float64 restatement ---------------------------------------------------------------------------------------------
_REF = {}


def _restatement(N):
    if N not in _REF:
        x = _random_rows(N, 201 * N, 3000 + N)
        w = AO.init_weights(np.random.default_rng(100 + N), N, stage=_stage(N))           # the weights of _actor(N)
        p64 = AO.actor_probs(w, x["actions_prev"], x["obs_self_t"], x["obs_self_v"], x["obs_others"], x["goals"], dtype=np.float64)
        _REF[N] = (x, AO.mixed_probs(p64, 0.3))
    return _REF[N]


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("N", range(1, 9))
def test_probabilities_match_the_float64_restatement(N, precision):
    x, want = _restatement(N)
    actor, _ = _actor(N, precision=precision)
    got = actor.probs_rows(*_args(x), 0.3).double().cpu().numpy()
    err = float(np.abs(got - want).max())
    print("N=%d %s max|probs - float64| = %.3e" % (N, precision, err))
    assert np.ptp(want, axis=1).mean() > 0.05                               # the policy is not uniform
    assert err < 2e-5


# ---- 5. the reference-derived network fixture ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("tag,rows", [("n2_stage2", 96), ("n1_stage1", 40)])
def test_rows_of_the_reference_derived_fixture(tag, rows, precision):
    from cm3_amd.actor import CheckersActor
    w, inp, probs = load_cases("actor_checkers")[tag]
    N, stage = int(tag[1]), int(tag[-1])
    assert probs.shape == (rows, 5)
    actor = CheckersActor(w, N, stage=stage, device=DEV, precision=precision)
    got = actor.probs_rows(_dev(inp["obs_self_t"]).double(), _dev(inp["obs_self_v"]), _dev(inp["obs_others"]), _dev(inp["a_prev"]),
                           _dev(inp["goals"]), 0.0)                         # wide inputs, the rows as recorded
    torch.cuda.synchronize()
    err = float(np.abs(got.double().cpu().numpy() - probs.astype(np.float64)).max())
    print("%s %s max|probs - recorded| = %.3e" % (tag, precision, err))
    assert err < 2e-5


# ---- 6. the device feeds equal the specification and the reference's recorded feeds -------------------------------------------------
@pytest.mark.parametrize("N", [1, 2])
def test_device_feeds_equal_the_torch_composition(N, monkeypatch, golden_dir):
    from cm3_amd.batch import train_step_feeds
    z = np.load(os.path.join(golden_dir, "trainstep_checkers_n%d.npz" % N))
    meta = json.loads(str(z["index"]))
    gamma, eps = meta["gamma"], meta["epsilon"]
    cols = {k[3:]: _dev(z[k]) for k in z.files if k.startswith("in_")}
    B = cols["vec"].shape[0]
    assert cols["vec"].shape == (B, N, 4) and cols["vec"].is_cuda
    main, _ = _actor(N, wseed=3)
    target, _ = _actor(N, wseed=4)
    made = {}
    sample_rows, probs_rows = target.sample_rows, main.probs_rows
    monkeypatch.setattr(target, "sample_rows", lambda *a, **kw: made.setdefault("acts", sample_rows(*a, draw=9, **kw)))
    monkeypatch.setattr(main, "probs_rows", lambda *a, **kw: made.setdefault("probs", probs_rows(*a, **kw)))
    answers = {"Q_global_target": (B * N, 1), "Q_credit_target": (B * N * N, 1), "V_target": (B * N, 1), "V": (B * N, 1),
               "Q_credit": (B * N * N * 5, 1)}

    def session(seen, device):
        def run(ops, feed):
            seen.append(ops)
            if ops == ["action_samples_target"]:
                assert not device
                return [made["acts"]["actions"]]
            if ops == ["probs"]:
                assert not device
                return [made["probs"]]
            out = []
            for op in ops:
                if op == "Q_global":
                    rows = feed["v_state_one_agent"].shape[0]
                    out.append(torch.linspace(-1, 1, rows, dtype=torch.float64, device=DEV).reshape(rows, 1))
                elif op in answers:
                    shape = answers[op]
                    out.append(torch.linspace(-2, 2, shape[0], dtype=torch.float64, device=DEV).reshape(shape))
                else:
                    out.append(None)
            return out
        return run

    seen_dev, seen_spec = [], []
    calls_dev = train_step_feeds(cols, session(seen_dev, True), gamma, eps, env="checkers", target_actor=target, actor=main)
    assert sorted(made) == ["acts", "probs"]
    calls_spec = train_step_feeds(cols, session(seen_spec, False), gamma, eps, env="checkers")
    torch.cuda.synchronize()
    names = [ops for ops, _ in calls_spec]
    assert names == [e["ops"] for e in meta["calls"]]                        # the reference's own op order
    assert names[0] == ["action_samples_target"] and ["probs"] in names and names[-1] == ["list_update_target_ops"]
    assert [ops for ops, _ in calls_dev] == names == seen_spec
    assert seen_dev == [ops for ops in names if ops not in (["action_samples_target"], ["probs"])]   # never run on the device path
    for (ops, got), (_, want) in zip(calls_dev, calls_spec):
        assert sorted(got) == sorted(want), ops
        for k in want:
            if not isinstance(want[k], torch.Tensor):
                assert got[k] == want[k], (ops, k)
                continue
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (ops, k)
            assert torch.equal(got[k], want[k]), (ops, k)
    # what the device actors were asked to evaluate is what the reference fed its own actor ops
    n_arrays = 0
    assert names.index(["probs"]) == (3 if N == 1 else 7)
    for c in (0, names.index(["probs"])):
        ops, feed = calls_dev[c]
        assert sorted(feed) == meta["calls"][c]["feed"], ops
        for k, v in feed.items():
            want = z["c%d_feed_%s" % (c, k)]
            got = v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
            assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (ops, k)
            n_arrays += 1
    assert n_arrays == 12
    # ... and the samples went on through the one-hot paths
    assert made["acts"]["actions"].dtype == torch.int32 and tuple(made["acts"]["actions"].shape) == (B * N,)
    assert torch.equal(calls_dev[1][1]["action_one"], torch.nn.functional.one_hot(made["acts"]["actions"].long(), 5))
    policy = [fd for ops, fd in calls_dev if ops == ["policy_op"]][0]
    assert policy["probs_evaluated"].dtype == torch.float32 and policy["probs_evaluated"].shape == (B * N * N if N > 1 else B, 5)


# ---- 7. the soft update -------------------------------------------------------------------------------------------------------------
def test_soft_update_of_the_target_actor():
    from cm3_amd import Cm3Error
    from cm3_amd.actor import _CK_NAMES, CheckersActor, ParticleActor
    from oracle import actor_oracle as PO
    N, tau = 2, 0.01
    main, w_main = _actor(N, wseed=21)
    target, w_target = _actor(N, wseed=22)
    target.soft_update_from(main, tau)
    t32, u32 = np.float32(tau), np.float32(1.0 - tau)
    want = {}
    assert len(_CK_NAMES) == 13 and sorted(target.w) == sorted(_CK_NAMES)
    for short, name in _CK_NAMES.items():
        m, t = w_main[name], w_target[name]
        want[name] = (t32 * m + u32 * t).astype(np.float32)
        got = target.w[short].cpu().numpy()
        assert np.array_equal(got.view(np.int32), want[name].view(np.int32)), name
        assert not np.array_equal(got, t)
    fresh = CheckersActor(want, N, stage=2, device=DEV, seed=SEED)
    rows = _args(_random_rows(N, 200, 5))
    a, b = target.probs_rows(*rows, 0.1), fresh.probs_rows(*rows, 0.1)      # the forward pass reads the repacked weights
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    other_n, _ = _actor(3)
    stage1 = CheckersActor(AO.init_weights(np.random.default_rng(1), N, stage=1), N, stage=1, device=DEV)
    particle = ParticleActor(PO.init_weights(np.random.default_rng(1), N, stage=2), N, stage=2, device=DEV)
    for bad in (other_n, stage1, particle):
        with pytest.raises(Cm3Error):
            target.soft_update_from(bad, tau)


# ---- 8. what the Python methods refuse ----------------------------------------------------------------------------------------------
def test_rows_methods_refuse_mismatched_shapes_and_zero_rows():
    from cm3_amd import Cm3Error
    N = 3
    actor, _ = _actor(N)
    ot, ov, oo, ap, vg = _args(_random_rows(N, 8, 3))
    for bad in ((ot[:, :4], ov, oo, ap, vg), (ot, ov[:4], oo, ap, vg), (ot, ov, oo[:, :2], ap, vg), (ot, ov, oo, ap[:4], vg),
                (ot, ov, oo, ap, vg[:, :1]), (ot[:0], ov[:0], oo[:0], ap[:0], vg[:0])):
        with pytest.raises(Cm3Error):
            actor.probs_rows(*bad, 0.1)
        with pytest.raises(Cm3Error):
            actor.sample_rows(*bad, 0.1)
    with pytest.raises(Cm3Error):                                           # the raw launch reads two window and two goal dtypes
        actor.enqueue_rows(8, ot.float(), ov, oo, ap.int(), vg.long(), 0.1, probs=torch.empty(8, 5, device=DEV))
    # any leading shape; flat windows; index goals; other dtypes are converted
    want = actor.probs_rows(ot, ov, oo, ap, vg, 0.1)
    got = actor.probs_rows(ot.reshape(2, 4, 75).float(), ov.reshape(2, 4, 4), oo.reshape(2, 4, -1), ap.reshape(2, 4).int(),
                           vg.argmax(-1).reshape(2, 4), 0.1)
    torch.cuda.synchronize()
    assert tuple(want.shape) == (8, 5) and not torch.equal(want[0], want[1])
    assert torch.equal(got, want)
