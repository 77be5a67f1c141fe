"""GPU: the data side of the Checkers QMIX train_step on the device -- the agent network over transition rows
(cm3_qmix_checkers_rows_f32, CheckersQmixAgent.greedy_rows) against the collection kernels it shares its layers with, the float64
restatement and the reference-recorded network fixture; the soft update of the target agent; and
qmix_train_step_feeds(env="checkers") with a target agent against its torch specification."""
import os

import numpy as np
import pytest
import torch

from tests import qmix_checkers_ref as QC
from tests.helpers import load_cfg
from tests.test_gpu_actor_checkers_f64 import _synthetic_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = ("f32", "f16x3")
KERNEL = {"f32": "k_ck_qmix_rows<", "f16x3": "k_ck_qmix_rows_x3<"}


def _agent(N, precision="f32", wseed=None):
    from cm3_amd.qmix import CheckersQmixAgent
    w = QC.init_weights(np.random.default_rng(200 + N if wseed is None else wseed), N)
    return CheckersQmixAgent(w, N, device=DEV, precision=precision), w


_BLOCK = {}


def _collection(N, E, precision):
    """(agent, narrow rows, wide rows, q, actions) of the collection kernel (agent.enqueue at epsilon 0) on _synthetic_rows and the
    very same tensors viewed as transition rows -- computed once per (N, E, precision) and left unchanged."""
    key = (N, E, precision)
    if key not in _BLOCK:
        inp = _synthetic_rows(N, E, 75 * N, np.random.default_rng(900 + N))
        agent, _ = _agent(N, precision)
        actions = torch.empty(E, N, dtype=torch.int32, device=DEV)
        q = torch.empty(E, N, 5, dtype=torch.float32, device=DEV)
        agent.enqueue(E, inp["raw"], inp["stride"], inp["obs_self_v"], inp["obs_others"], inp["goals"], inp["actions_prev"],
                      inp["steps"], inp["episode"], actions, 0.0, probs=q, prev_done=None)
        R = E * N
        narrow = dict(obs_self_t=inp["raw"].view(R, 75), obs_self_v=inp["obs_self_v"].view(R, 4),
                      obs_others=inp["obs_others"].view(R, -1), actions_prev=inp["actions_prev"].view(R), goals=inp["goals"].view(R))
        wide = dict(narrow, obs_self_t=narrow["obs_self_t"].double(),
                    goals=torch.nn.functional.one_hot(narrow["goals"].long(), 2).contiguous())
        torch.cuda.synchronize()
        _BLOCK[key] = (agent, narrow, wide, q.view(R, 5), actions.view(R))
    return _BLOCK[key]


# ---- 1. the bits of the collection kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("N", range(1, 9))
def test_rows_kernel_gives_the_bits_of_the_collection_kernel(N, precision):
    from cm3_amd import _lib
    E = 201                                                  # E * N mod 64: 9, 18, 27, 36, 45, 54, 63, 8 -- ragged at every N
    assert (E * N) % 64 != 0
    agent, narrow, wide, q_act, a_act = _collection(N, E, precision)
    assert narrow["obs_self_t"].dtype == torch.int8 and narrow["goals"].dtype == torch.uint8
    assert wide["obs_self_t"].dtype == torch.float64 and wide["goals"].dtype == torch.int64
    for form, rows in (("narrow", narrow), ("wide", wide)):
        lead = lambda t: t.view(E, N, *t.shape[1:])          # noqa: E731  (any leading shape)
        out = agent.greedy_rows(lead(rows["obs_self_t"]), lead(rows["obs_self_v"]), lead(rows["obs_others"]),
                                lead(rows["actions_prev"]), lead(rows["goals"]), q=True, onehot=True, q_max=True)
        torch.cuda.synchronize()
        v = _lib.last_kernel_variant()
        assert v.startswith(KERNEL[precision]) and (",N=%d," % N) in v, v
        assert (",g=%d," % (3 if form == "wide" else 0)) in v, v
        assert out["q"].dtype == torch.float32 and out["argmax"].dtype == torch.int32
        assert out["onehot"].dtype == torch.int64 and out["q_max"].dtype == torch.float32
        assert torch.equal(out["q"].view(torch.int32), q_act.view(torch.int32)), form          # bit for bit
        assert torch.equal(out["argmax"], a_act), form
        assert torch.equal(out["onehot"], torch.nn.functional.one_hot(out["argmax"].long(), 5))
        assert torch.equal(out["q_max"], out["q"].max(-1).values)
        assert len(torch.unique(out["argmax"])) > 1


# ---- 2. edges: ragged counts, rows past n_rows, every output alone ------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_row_counts_and_single_outputs(N, n_rows, precision):
    E = -(-256 // N)                                                        # a block of at least 256 rows: rows past n_rows exist
    agent, narrow, wide, q_act, a_act = _collection(N, E, precision)
    want = {"q": q_act[:n_rows], "argmax": a_act[:n_rows], "onehot": torch.nn.functional.one_hot(a_act[:n_rows].long(), 5),
            "q_max": q_act[:n_rows].max(-1).values}
    spec = {"q": ((n_rows + 1, 5), torch.float32, -12345.0), "argmax": ((n_rows + 1,), torch.int32, -7),
            "onehot": ((n_rows + 1, 5), torch.int64, -7), "q_max": ((n_rows + 1,), torch.float32, -12345.0)}
    for form, clean in (("narrow", narrow), ("wide", wide)):
        # rows at or past n_rows hold values that would change a live row if they were read into it
        rows = {k: v[:256].clone() for k, v in clean.items()}
        rows["obs_self_t"][n_rows:] = 5
        rows["actions_prev"][n_rows:] = 4
        rows["obs_self_v"][n_rows:] = 1000.0
        rows["obs_others"][n_rows:] = -1000.0
        rows["goals"][n_rows:] = 1 - rows["goals"][n_rows:]
        for name in spec:                                                   # four launches, each writing only its own buffer
            bufs = {k: torch.full(shape, fill, dtype=dt, device=DEV) for k, (shape, dt, fill) in spec.items()}
            agent.enqueue_rows(n_rows, rows["obs_self_t"], rows["obs_self_v"], rows["obs_others"], rows["actions_prev"],
                               rows["goals"], **{name: bufs[name]})
            torch.cuda.synchronize()
            for k, (shape, dt, fill) in spec.items():
                if k == name:
                    assert torch.equal(bufs[k][:n_rows], want[k]), (form, name, k)
                    assert bool((bufs[k][n_rows:] == fill).all()), (form, name, k)    # the extra row is untouched
                else:
                    assert bool((bufs[k] == fill).all()), (form, name, k)


# ---- 3. against the float64 restatement ---------------------------------------------------------------------------------------------
_REF = {}


def _restatement(N):
    if N not in _REF:
        rng = np.random.default_rng(3000 + N)
        R, Lo = 201 * N, 2 * max(N - 1, 1)
        x = dict(obs_self_t=rng.integers(-1, 2, (R, 5, 5, 3)).astype(np.float64), obs_self_v=rng.uniform(-0.5, 1.0, (R, 4)),
                 obs_others=rng.uniform(-1, 1, (R, Lo)), actions_prev=rng.integers(0, 5, R), goals=np.eye(2)[rng.integers(0, 2, R)])
        w = QC.init_weights(np.random.default_rng(200 + N), N)
        ref = QC.q_values(w, x["actions_prev"], x["obs_self_t"], x["obs_self_v"], x["obs_others"], x["goals"])
        _REF[N] = (x, ref)
    return _REF[N]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("N", range(1, 9))
def test_q_values_match_the_float64_restatement(N, precision):
    x, ref = _restatement(N)
    agent, _ = _agent(N, precision)                           # QC.init_weights(default_rng(200 + N), N)
    dev = lambda a: torch.as_tensor(a, device=DEV)            # noqa: E731
    out = agent.greedy_rows(dev(x["obs_self_t"]), dev(x["obs_self_v"]), dev(x["obs_others"]), dev(x["actions_prev"]), dev(x["goals"]),
                            q=True, onehot=False)
    torch.cuda.synchronize()
    q = out["q"].double().cpu().numpy()
    a = out["argmax"].cpu().numpy()
    bound = 2e-5 * np.maximum(1.0, np.abs(ref).max(axis=1))
    err = np.abs(q - ref).max(axis=1)
    print("N=%d %s: max err / bound %.3f" % (N, precision, float((err / bound).max())))
    assert (err <= bound).all(), float((err / bound).max())
    top2 = np.sort(ref, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-4
    assert 1.0 - clear.mean() <= 0.01, float(1.0 - clear.mean())
    assert np.array_equal(a[clear], np.argmax(ref, axis=1)[clear])
    assert len(np.unique(a)) >= 3


# ---- 4. the reference-recorded network fixture --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("N", [1, 2])
def test_rows_of_the_reference_recorded_fixture(N, precision, golden_dir):
    from cm3_amd.qmix import CheckersQmixAgent
    z = np.load(os.path.join(golden_dir, "qmix_checkers.npz"))
    tag = "n%d" % N
    w = {str(k): z["w/" + str(k)] for k in z["names"]}
    x = {k: z[tag + "/in/" + k] for k in ("a_prev", "obs_self_t", "obs_self_v", "obs_others", "goals")}
    agent = CheckersQmixAgent(w, N, device=DEV, precision=precision)
    dev = lambda a: torch.as_tensor(a, device=DEV)            # noqa: E731
    out = agent.greedy_rows(dev(x["obs_self_t"]).double(), dev(x["obs_self_v"]), dev(x["obs_others"]), dev(x["a_prev"]),
                            dev(x["goals"]), q=True)          # wide inputs, the rows as recorded
    torch.cuda.synchronize()
    ref = z[tag + "/q"].astype(np.float64)
    q = out["q"].double().cpu().numpy()
    assert (np.abs(q - ref).max(axis=1) <= 2e-5 * np.maximum(1.0, np.abs(ref).max(axis=1))).all()
    assert np.array_equal(out["argmax"].cpu().numpy(), z[tag + "/argmax"])


# ---- 5. the soft update -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_soft_update_of_the_target_agent(precision):
    from cm3_amd import Cm3Error
    from cm3_amd.qmix import CK_NAMES, CheckersQmixAgent, ParticleQmixAgent
    from tests import qmix_ref as QR
    N, tau = 2, 0.01
    main, w_main = _agent(N, precision, wseed=21)
    target, w_target = _agent(N, precision, wseed=22)
    target.soft_update_from(main, tau)
    t32, u32 = np.float32(tau), np.float32(1.0 - tau)
    want = {}
    assert len(CK_NAMES) == 13
    for short, name in CK_NAMES.items():
        m, t = w_main["Agent_main/" + name], w_target["Agent_main/" + name]
        want[name] = (t32 * m + u32 * t).astype(np.float32)
        got = target.w[short].cpu().numpy()
        assert np.array_equal(got.view(np.int32), want[name].view(np.int32)), name
        assert not np.array_equal(got, t)
    fresh = CheckersQmixAgent(want, N, device=DEV, precision=precision)
    x, _ = _restatement(N)
    dev = lambda a: torch.as_tensor(a, device=DEV)            # noqa: E731
    rows = (dev(x["obs_self_t"]), dev(x["obs_self_v"]), dev(x["obs_others"]), dev(x["actions_prev"]), dev(x["goals"]))
    a, b = target.greedy_rows(*rows, q=True), fresh.greedy_rows(*rows, q=True)
    torch.cuda.synchronize()
    for k in ("q", "argmax", "onehot"):
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(Cm3Error):                             # another agent count
        target.soft_update_from(_agent(3, precision)[0], tau)
    with pytest.raises(Cm3Error):                             # another precision
        target.soft_update_from(_agent(N, "f16x3" if precision == "f32" else "f32")[0], tau)
    with pytest.raises(Cm3Error):                             # another class
        target.soft_update_from(ParticleQmixAgent(QR.init_weights(np.random.default_rng(0), N), N, device=DEV), tau)


# ---- 6. the device feeds equal the specification ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", ["wide", "compact"])
def test_device_feeds_equal_the_torch_composition(ring):
    from cm3_amd.batch import qmix_train_step_feeds
    from cm3_amd.checkers import VecCheckersEnv
    from cm3_amd.replay import CompactCheckersReplayBuffer, DeviceReplayBuffer
    from cm3_amd.rollout import CheckersRollout
    E, N, T, B, gamma = 24, 2, 7, 128, 0.99
    main, _ = _agent(N, "f16x3", wseed=3)
    target, _ = _agent(N, "f16x3", wseed=4)
    cfg = load_cfg("checkers_stage2.json")
    env = VecCheckersEnv(cfg["init"], N, 33, E, device=DEV, seed=12341, auto_reset=True)
    ro = CheckersRollout(env, n_ticks=T)
    ro.collect(np.eye(2), policy=main, epsilon=0.3)
    buf = (CompactCheckersReplayBuffer if ring == "compact" else DeviceReplayBuffer)(size=E * T, device=DEV)
    buf.add_rollout(ro)
    cols = buf.sample_batch(B, generator=torch.Generator(device=DEV).manual_seed(0))
    assert cols["vec"].shape == (B, N, 4) and cols["vec"].is_cuda
    assert cols["next_obs_self_t"].dtype == torch.float64 and cols["goals"].dtype == torch.int64
    q_tot = torch.as_tensor(np.random.default_rng(N).standard_normal((B, 1)).astype(np.float32), device=DEV)

    def session(seen, answer_argmax):
        def run(ops, feed):
            seen.append(ops)
            if ops == ["argmax_Q_target"]:
                assert answer_argmax
                return [target.greedy_rows(feed["obs_self_t"], feed["obs_self_v"], feed["obs_others"], feed["actions_prev"].argmax(1),
                                           feed["v_goal"], onehot=False)["argmax"]]
            return [q_tot] if ops == ["mixer_target"] else [None]
        return run

    seen_dev, seen_spec = [], []
    calls_dev = qmix_train_step_feeds(cols, session(seen_dev, False), gamma, target_agent=target, env="checkers")
    calls_spec = qmix_train_step_feeds(cols, session(seen_spec, True), gamma, env="checkers")
    torch.cuda.synchronize()
    order = [["argmax_Q_target"], ["mixer_target"], ["mixer_op"], ["list_update_target_ops"]]
    assert seen_spec == order and seen_dev == order[1:]                # the device path's run never sees argmax_Q_target
    assert [ops for ops, _ in calls_dev] == order == [ops for ops, _ in calls_spec]
    for (ops, got), (_, want) in zip(calls_dev, calls_spec):
        assert sorted(got) == sorted(want), ops
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (ops, k)
            assert torch.equal(got[k], want[k]), (ops, k)
    td = calls_dev[2][1]["td_target"]
    assert td.dtype == torch.float64 and td.shape == (B,)
    assert calls_dev[1][1]["actions_1hot"].dtype == torch.int64 and int(calls_dev[1][1]["actions_1hot"].sum()) == B * N
    assert torch.equal(calls_dev[0][1]["actions_prev"], calls_dev[2][1]["actions_1hot"])     # the action just taken
    assert len(torch.unique(calls_dev[2][1]["actions_1hot"].argmax(1))) > 1                 # (the actions taken: epsilon 0.3)
    ro.close()
