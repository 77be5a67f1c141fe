"""GPU: the CM3 particle actor over transition rows (cm3_actor_particle_rows_f32; ParticleActor.probs_rows / sample_rows) against
the collection kernel it shares its forward pass with, the NumPy restatement of its draw (tests/actor_rows_ref.py), the float64
restatement of the network (oracle/actor_oracle.py); train_step_feeds with device actors against its torch specification; the soft
update of the target actor."""
import numpy as np
import pytest
import torch

from oracle import actor_oracle as AO
from tests import actor_rows_ref as RR
from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 77


def _cfg(N):
    return {1: "particle_stage1.json", 2: "particle_stage2_merge.json", 9: "particle_ring10.json",
            10: "particle_ring10.json"}.get(N, "particle_merge8.json")


def _stage(N):
    return 1 if N == 1 else 2


def _env(E, N, seed=11, **kw):
    from cm3_amd.particle import VecParticleEnv
    return VecParticleEnv(load_cfg(_cfg(N)), N, 0.2, 33, E, device=DEV, seed=seed, **kw)


def _actor(N, precision="f32", wseed=None, seed=SEED):
    from cm3_amd.actor import ParticleActor
    w = AO.init_weights(np.random.default_rng(100 + N if wseed is None else wseed), N, stage=_stage(N))
    return ParticleActor(w, N, stage=_stage(N), device=DEV, seed=seed, precision=precision), w


def _random_rows(N, R, rseed):
    rng = np.random.default_rng(rseed)
    L = 4 * max(N - 1, 1)
    return (rng.standard_normal((R, L)).astype(np.float32), rng.standard_normal((R, 4)).astype(np.float32),
            rng.uniform(-1, 1, (R, 2)).astype(np.float32))


def _dev(x):
    return torch.as_tensor(x, device=DEV)


_ACT = {}


def _collection(N, E, precision="f32"):
    """(actor, rows, probs) of actor.act(env, 0.3, return_probs=True) on an env stepped 3 times, and the same observation as
    contiguous rows -- computed once per (N, E, precision) and left unchanged."""
    key = (N, E, precision)
    if key not in _ACT:
        env = _env(E, N, env_id_base=5)
        env.reset()
        for _ in range(3):
            env.step()
        actor, _ = _actor(N, precision)
        _, probs = actor.act(env, 0.3, return_probs=True)
        gs, oo = env.get_obs()
        rows = (oo.reshape(E * N, -1).contiguous().clone(), gs.reshape(E * N, 4).contiguous().clone(),
                env.goals.reshape(E * N, 2).contiguous().clone())
        torch.cuda.synchronize()
        _ACT[key] = (actor, rows, probs.reshape(E * N, 5).clone())
    return _ACT[key]


# ---- 1. the same bits as the collection kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16"])
@pytest.mark.parametrize("N", list(range(1, 11)))
def test_rows_kernel_gives_the_bits_of_the_collection_kernel(N, precision):
    from cm3_amd import _lib
    E = 37                                                   # 37 N rows: the last workgroup is ragged for every N
    assert (E * N) % 64 != 0
    actor, (oo, vo, vg), p_act = _collection(N, E, precision)
    assert tuple(oo.shape) == (E * N, 4 * max(N - 1, 1)) and tuple(vo.shape) == (E * N, 4) and tuple(vg.shape) == (E * N, 2)
    got = actor.probs_rows(oo.reshape(E, N, -1), vo.reshape(E, N, 4), vg.reshape(E, N, 2), 0.3)
    torch.cuda.synchronize()
    v = _lib.last_kernel_variant()
    assert v.startswith("k_actor_particle_rows<f32,N=%d," % N), v
    assert got.dtype == torch.float32 and tuple(got.shape) == (E * N, 5)
    assert torch.equal(got.view(torch.int32), p_act.view(torch.int32))                          # bit for bit
    assert len(torch.unique(got)) > 5


# ---- 2. edges: ragged counts, rows past n_rows, every output alone ----------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("N", [1, 4])
def test_row_counts_and_single_outputs(N, n_rows):
    E = 256 // N
    actor, (oo, vo, vg), p_act = _collection(N, E)                         # a 256-row block: rows past n_rows exist
    spec = {"probs": ((n_rows + 1, 5), torch.float32, -12345.0), "actions": ((n_rows + 1,), torch.int32, -7),
            "onehot": ((n_rows + 1, 5), torch.int64, -7)}
    fresh = lambda: {k: torch.full(shape, fill, dtype=dt, device=DEV) for k, (shape, dt, fill) in spec.items()}    # noqa: E731
    every = fresh()
    actor.enqueue_rows(n_rows, oo, vo, vg, 0.3, draw=5, **every)            # all three together: the reference of this test
    torch.cuda.synchronize()
    assert torch.equal(every["probs"][:n_rows].view(torch.int32), p_act[:n_rows].view(torch.int32))
    u = RR.rows_uniforms(SEED, n_rows, 5)
    assert np.array_equal(every["actions"][:n_rows].cpu().numpy(), AO.sample_actions(p_act[:n_rows].cpu().numpy(), u))
    assert torch.equal(every["onehot"][:n_rows], torch.nn.functional.one_hot(every["actions"][:n_rows].long(), 5))
    for k, (shape, dt, fill) in spec.items():
        assert bool((every[k][n_rows:] == fill).all()), k                  # the guard row is untouched
    for name in spec:                                                       # three launches, each writing only its own buffer
        bufs = fresh()
        actor.enqueue_rows(n_rows, oo, vo, vg, 0.3, draw=5, **{name: bufs[name]})
        torch.cuda.synchronize()
        for k, (shape, dt, fill) in spec.items():
            if k == name:
                assert torch.equal(bufs[k], every[k]), (name, k)            # the same values, the same untouched guard row
            else:
                assert bool((bufs[k] == fill).all()), (name, k)


# ---- 3. sampling is exact against the restated stream -----------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("N", [1, 4, 9])
def test_sampling_is_exact_against_the_restated_stream(N, eps):
    R = 1000
    actor, _ = _actor(N)
    oo, vo, vg = (_dev(x) for x in _random_rows(N, R, 40 + N))
    assert actor.rows_draw == 0
    first = actor.sample_rows(oo, vo, vg, eps, probs=True, onehot=True)
    second = actor.sample_rows(oo, vo, vg, eps, probs=True)
    again = actor.sample_rows(oo, vo, vg, eps, probs=True, draw=0)
    torch.cuda.synchronize()
    assert actor.rows_draw == 2                                              # (an explicit draw leaves the counter alone)
    assert first["actions"].dtype == torch.int32 and tuple(first["actions"].shape) == (R,)
    probs = first["probs"].cpu().numpy()
    for k, out in enumerate((first, second)):
        # the pick is a float32 inverse CDF over the device's own float32 probabilities: every row, nothing to tolerate
        assert torch.equal(out["probs"], first["probs"])
        assert np.array_equal(out["actions"].cpu().numpy(), AO.sample_actions(probs, RR.rows_uniforms(SEED, R, k))), k
    assert torch.equal(first["onehot"], torch.nn.functional.one_hot(first["actions"].long(), 5))
    assert not torch.equal(first["actions"], second["actions"])
    assert torch.equal(again["actions"], first["actions"])
    freq = np.bincount(first["actions"].cpu().numpy(), minlength=5) / R
    assert np.abs(freq - probs.mean(0)).max() < 0.05
    # a row id base shifts the stream: rows 100.. of base 0 are rows 0.. of base 100
    shifted = torch.empty(R - 100, dtype=torch.int32, device=DEV)
    actor.enqueue_rows(R - 100, oo[100:].contiguous(), vo[100:].contiguous(), vg[100:].contiguous(), eps, actions=shifted, draw=0,
                       row_id_base=100)
    torch.cuda.synchronize()
    assert torch.equal(shifted, first["actions"][100:])


def test_epsilon_from_the_device_is_the_epsilon_of_the_descriptor():
    N, R = 4, 130
    actor, _ = _actor(N)
    oo, vo, vg = (_dev(x) for x in _random_rows(N, R, 3))
    eps_dev = torch.tensor([0.3], dtype=torch.float32, device=DEV)
    a, b = actor.probs_rows(oo, vo, vg, 0.3), actor.probs_rows(oo, vo, vg, eps_dev)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, actor.probs_rows(oo, vo, vg, 0.0))


def test_rows_methods_refuse_mismatched_shapes_and_zero_rows():
    from cm3_amd import Cm3Error
    N = 4
    actor, _ = _actor(N)
    oo, vo, vg = (_dev(x) for x in _random_rows(N, 8, 3))
    for bad in ((oo[:, :8], vo, vg), (oo, vo[:4], vg), (oo, vo, vg[:, :1]), (oo[:0], vo[:0], vg[:0])):
        with pytest.raises(Cm3Error):
            actor.probs_rows(*bad, 0.1)
        with pytest.raises(Cm3Error):
            actor.sample_rows(*bad, 0.1)
    got = actor.probs_rows(oo.double().reshape(2, 4, -1), vo.double().reshape(2, 4, 4), vg.double().reshape(2, 4, 2), 0.1)
    assert torch.equal(got, actor.probs_rows(oo, vo, vg, 0.1))              # a float64 column is rounded; the leading shape is [...]


# ---- 4. against the float64 restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("N", [1, 2, 4, 8, 10])
def test_probabilities_match_the_float64_restatement(N, precision):
    R, eps = 333, 0.3
    oo, vo, vg = _random_rows(N, R, 7 + N)
    actor, w = _actor(N, precision)
    got = actor.probs_rows(_dev(oo), _dev(vo), _dev(vg), eps).double().cpu().numpy()
    want = AO.mixed_probs(AO.actor_probs(w, oo, vo, vg, dtype=np.float64), eps)
    err = float(np.abs(got - want).max())
    print("N=%d %s max|probs - float64| = %.3e" % (N, precision, err))
    assert err < 2e-5


# ---- 5. the device feeds equal the specification ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 4])
def test_device_feeds_equal_the_torch_composition(N, monkeypatch):
    from cm3_amd.batch import train_step_feeds
    B, gamma, eps = 33, 0.99, 0.3
    rng = np.random.default_rng(50 + N)
    L = 4 * max(N - 1, 1)
    f = lambda *s: _dev(rng.standard_normal(s).astype(np.float32))          # noqa: E731
    cols = {"v_global": f(B, N, 4), "obs_others": f(B, N, L), "v_local": f(B, N, 4), "actions": _dev(rng.integers(0, 5, (B, N))),
            "reward": f(B), "reward_local": f(B, N), "v_global_next": f(B, N, 4), "obs_others_next": f(B, N, L),
            "v_local_next": f(B, N, 4), "done": _dev(rng.random(B) < 0.3), "goals": f(B, N, 2)}
    main, _ = _actor(N, wseed=3)
    target, _ = _actor(N, wseed=4)
    made = {}
    sample_rows, probs_rows = target.sample_rows, main.probs_rows
    monkeypatch.setattr(target, "sample_rows", lambda *a, **kw: made.setdefault("acts", sample_rows(*a, draw=9, **kw)))
    monkeypatch.setattr(main, "probs_rows", lambda *a, **kw: made.setdefault("probs", probs_rows(*a, **kw)))
    answers = {"Q_global_target": (B * N, 1), "Q_global": None, "Q_credit_target": (B * N * N, 1), "V_target": (B * N, 1),
               "V": (B * N, 1), "Q_credit": (B * N * N * 5, 1)}

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
    calls_dev = train_step_feeds(cols, session(seen_dev, True), gamma, eps, target_actor=target, actor=main)
    assert sorted(made) == ["acts", "probs"]
    calls_spec = train_step_feeds(cols, session(seen_spec, False), gamma, eps)
    torch.cuda.synchronize()
    names = [ops for ops, _ in calls_spec]
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
    policy = [fd for ops, fd in calls_dev if ops == ["policy_op"]][0]
    assert policy["probs_evaluated"].dtype == torch.float32 and policy["probs_evaluated"].shape == (B * N * N if N > 1 else B, 5)


# ---- 6. the soft update -----------------------------------------------------------------------------------------------------------
def test_soft_update_of_the_target_actor():
    from cm3_amd import Cm3Error
    from cm3_amd.actor import _NAMES, ParticleActor
    from cm3_amd.qmix import ParticleQmixAgent
    from tests import qmix_ref as QR
    N, tau = 4, 0.01
    main, w_main = _actor(N, wseed=21)
    target, w_target = _actor(N, wseed=22)
    target.soft_update_from(main, tau)
    t32, u32 = np.float32(tau), np.float32(1.0 - tau)
    want = {}
    for short, name in _NAMES.items():
        m, t = w_main[name], w_target[name]
        want[name] = (t32 * m + u32 * t).astype(np.float32)
        got = target.w[short].cpu().numpy()
        assert np.array_equal(got.view(np.int32), want[name].view(np.int32)), name
        assert not np.array_equal(got, t)
    fresh = ParticleActor(want, N, stage=2, device=DEV, seed=SEED)
    rows = tuple(_dev(x) for x in _random_rows(N, 200, 5))
    a, b = target.probs_rows(*rows, 0.1), fresh.probs_rows(*rows, 0.1)      # the forward pass reads the repacked weights
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    other_n, _ = _actor(2)
    stage1 = ParticleActor(AO.init_weights(np.random.default_rng(1), N, stage=1), N, stage=1, device=DEV)
    qmix = ParticleQmixAgent(QR.init_weights(np.random.default_rng(1), N), N, device=DEV)
    for bad in (other_n, stage1, qmix):
        with pytest.raises(Cm3Error):
            target.soft_update_from(bad, tau)
