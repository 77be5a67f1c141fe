"""GPU: the COUNTED actor rows launches (cm3_actor_particle_rows_counted_f32 / cm3_actor_checkers_rows_counted_f32;
sample_rows(..., draw=RowsDrawCounter)) -- a launch that reads its draw counter from device memory and advances it itself, so that a
captured launch draws afresh on every replay -- and OnPolicyPhasePlan with device actors on top of it.

References: tests/actor_rows_ref.py (the restated rows stream) for the actions, the uncounted launch (probs_rows) for the
probabilities, the use_graph=False plan (train_step_feeds called eagerly with the same counter) for the graph plan."""
import numpy as np
import pytest
import torch

from oracle import actor_checkers_oracle as CO
from oracle import actor_oracle as AO
from tests import actor_rows_ref as RR
from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 77
EPS = 0.3
WRAP = 2 ** 32
DRAWS = [0, 1, WRAP - 1]
# 1 .. 65: around one workgroup of 64 rows; 513: 9 workgroups, more than the chip has XCDs; 64 * 300 + 7: more workgroups than CUs
ROWS = [1, 63, 64, 65, 513, 64 * 300 + 7]


class _Particle(object):
    name = "particle"
    kernel = {"f32": "k_actor_particle_rows<", "bf16": "k_actor_particle_rows<", "f16x3": "k_actor_particle_rows<"}
    sample = staticmethod(AO.sample_actions)

    @staticmethod
    def actor(N, precision, wseed=None):
        from cm3_amd.actor import ParticleActor
        stage = 1 if N == 1 else 2
        w = AO.init_weights(np.random.default_rng(100 + N if wseed is None else wseed), N, stage=stage)
        return ParticleActor(w, N, stage=stage, device=DEV, seed=SEED, precision=precision)

    @staticmethod
    def rows(N, R, form):
        rng = np.random.default_rng(1000 + N)
        L = 4 * max(N - 1, 1)
        return tuple(torch.as_tensor(x, device=DEV) for x in (
            rng.standard_normal((R, L)).astype(np.float32), rng.standard_normal((R, 4)).astype(np.float32),
            rng.uniform(-1, 1, (R, 2)).astype(np.float32)))


class _Checkers(object):
    name = "checkers"
    kernel = {"f32": "k_ck_actor_rows<", "f16x3": "k_ck_actor_rows_x3<"}
    sample = staticmethod(CO.sample_actions)

    @staticmethod
    def actor(N, precision, wseed=None):
        from cm3_amd.actor import CheckersActor
        stage = 1 if N == 1 else 2
        w = CO.init_weights(np.random.default_rng(100 + N if wseed is None else wseed), N, stage=stage)
        return CheckersActor(w, N, stage=stage, device=DEV, seed=SEED, precision=precision)

    @staticmethod
    def rows(N, R, form):
        """form "int8": int8 windows and uint8 index goals (what the trajectory keeps); "f64": float64 windows and int64 one-hot goals
        (what sample_batch returns) -- the same values either way"""
        rng = np.random.default_rng(2000 + N)
        Lo = 2 * max(N - 1, 1)
        win, goal = rng.integers(-1, 2, (R, 75)), rng.integers(0, 2, R)
        ot = torch.as_tensor(win.astype(np.int8) if form == "int8" else win.astype(np.float64), device=DEV)
        vg = torch.as_tensor(goal.astype(np.uint8) if form == "int8" else np.eye(2, dtype=np.int64)[goal], device=DEV)
        return (ot, torch.as_tensor(rng.uniform(-0.5, 1.0, (R, 4)), device=DEV), torch.as_tensor(rng.uniform(-1, 1, (R, Lo)), device=DEV),
                torch.as_tensor(rng.integers(0, 5, R).astype(np.int32), device=DEV), vg)


_CASE = {}


def _case(env, N, precision, R, form=None):
    """(actor, input rows, probs of the UNCOUNTED launch as float32 NumPy and as a device tensor): once per key, left unchanged"""
    key = (env.name, N, precision, R, form)
    if key not in _CASE:
        akey = (env.name, N, precision)
        if akey not in _CASE:
            _CASE[akey] = env.actor(N, precision)
        actor = _CASE[akey]
        rows = env.rows(N, R, form)
        probs = actor.probs_rows(*rows, EPS)
        torch.cuda.synchronize()
        _CASE[key] = (actor, rows, probs.cpu().numpy(), probs)
    return _CASE[key]


def _want(env, actor, probs_np, draw):
    return env.sample(probs_np, RR.rows_uniforms(SEED, probs_np.shape[0], draw % WRAP))


def _counter(start):
    from cm3_amd.actor import RowsDrawCounter
    return RowsDrawCounter(DEV, start)


def _check_counted_equals_stream(env, N, precision, R, form=None):
    from cm3_amd import _lib
    actor, rows, probs_np, probs = _case(env, N, precision, R, form)
    host_draw = actor.rows_draw
    for c in DRAWS:
        counter = _counter(c)
        assert counter.value() == c and counter.arrivals() == 0
        out = actor.sample_rows(*rows, EPS, probs=True, onehot=True, draw=counter)
        torch.cuda.synchronize()
        v = _lib.last_kernel_variant()
        assert v.startswith(env.kernel[precision]) and v.endswith(",counted>"), v
        assert np.array_equal(out["actions"].cpu().numpy(), _want(env, actor, probs_np, c)), c
        assert torch.equal(out["onehot"], torch.nn.functional.one_hot(out["actions"].long(), 5)), c
        assert torch.equal(out["probs"].view(torch.int32), probs.view(torch.int32)), c              # bit for bit
        assert counter.value() == (c + 1) % WRAP and counter.arrivals() == 0, c
    assert actor.rows_draw == host_draw                                          # the host counter is not involved
    plain = actor.sample_rows(*rows, EPS, draw=1)                                # ... and an integer draw is the launch of before
    torch.cuda.synchronize()
    assert not _lib.last_kernel_variant().endswith(",counted>")
    assert np.array_equal(plain["actions"].cpu().numpy(), _want(env, actor, probs_np, 1))


# ---- 1. a counted launch at counter value c is the uncounted launch at draw = c, and leaves c + 1 -------------------------------------
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16"])
@pytest.mark.parametrize("N", [1, 3, 4])
def test_counted_equals_stream_particle(N, precision, R):
    _check_counted_equals_stream(_Particle, N, precision, R)


@pytest.mark.parametrize("form", ["int8", "f64"])
@pytest.mark.parametrize("precision,R", [("f16x3", r) for r in ROWS] + [("f32", r) for r in (1, 65, 513, 64 * 300 + 7)])
def test_counted_equals_stream_checkers(precision, R, form):
    _check_counted_equals_stream(_Checkers, 2, precision, R, form)


# ---- 2. a launch that draws nothing leaves the counter alone --------------------------------------------------------------------------
@pytest.mark.parametrize("env,N,precision,form", [(_Particle, 4, "f16x3", None), (_Particle, 1, "f32", None), (_Checkers, 2, "f16x3", "int8"),
                                                  (_Checkers, 2, "f32", "f64")], ids=["particle-x3", "particle-f32", "checkers-x3", "checkers-f32"])
def test_probs_only_counted_call_leaves_both_words(env, N, precision, form):
    R = 513
    actor, rows, _, probs = _case(env, N, precision, R, form)
    counter = _counter(41)
    counter.state[1] = 7                                                          # (a sentinel: a launch that took tickets would move it)
    got = torch.empty(R, 5, dtype=torch.float32, device=DEV)
    staged = [t.reshape(R, -1) if t.dim() > 1 else t for t in rows]
    actor.enqueue_rows(R, *staged, EPS, probs=got, draw=counter)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), probs.view(torch.int32))
    assert counter.value() == 41 and counter.arrivals() == 7


# ---- 3. launches that share a counter on one stream draw c, c + 1, ... ----------------------------------------------------------------
@pytest.mark.parametrize("env,N,form", [(_Particle, 4, None), (_Checkers, 2, "int8")], ids=["particle", "checkers"])
@pytest.mark.parametrize("c", [5, WRAP - 2])
def test_back_to_back_launches_take_successive_draws(env, N, form, c):
    R = 513
    actor, rows, probs_np, _ = _case(env, N, "f16x3", R, form)
    counter = _counter(c)
    outs = [actor.sample_rows(*rows, EPS, draw=counter)["actions"] for _ in range(5)]       # no synchronisation in between
    torch.cuda.synchronize()
    for i, out in enumerate(outs):
        assert np.array_equal(out.cpu().numpy(), _want(env, actor, probs_np, c + i)), i
    assert counter.value() == (c + 5) % WRAP and counter.arrivals() == 0
    assert len({o.data_ptr() for o in outs}) == 5


# ---- 4. a CAPTURED counted launch draws afresh on every replay ------------------------------------------------------------------------
@pytest.mark.parametrize("env,N,form", [(_Particle, 4, None), (_Checkers, 2, "int8")], ids=["particle", "checkers"])
def test_captured_launch_advances_its_counter_on_every_replay(env, N, form):
    from cm3_amd import _lib
    R, c = 513, WRAP - 2
    actor, rows, probs_np, _ = _case(env, N, "f16x3", R, form)
    counter = _counter(c)
    box, keep = {}, []

    def enqueue(stream):
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=DEV)):
            box["out"] = actor.sample_rows(*rows, EPS, draw=counter, keep=keep)
    graph = _lib.capture_graph(DEV, enqueue)
    try:
        assert any(t is box["out"]["actions"] for t in keep)                     # the output is held by the caller's list
        torch.cuda.synchronize()
        assert counter.value() == c                                              # a capture launches nothing
        stream = torch.cuda.current_stream(DEV)
        copies = [torch.empty(R, dtype=torch.int32, device=DEV) for _ in range(3)]
        for copy in copies:
            _lib.check(_lib.lib().cm3_graph_launch(graph, stream.cuda_stream))
            copy.copy_(box["out"]["actions"])                                    # device to device, on the same stream
        torch.cuda.synchronize()
        for i, copy in enumerate(copies):
            assert np.array_equal(copy.cpu().numpy(), _want(env, actor, probs_np, c + i)), i
        assert not torch.equal(copies[0], copies[1]) and not torch.equal(copies[1], copies[2])
        assert counter.value() == (c + 3) % WRAP and counter.arrivals() == 0
    finally:
        torch.cuda.synchronize()
        _lib.lib().cm3_graph_destroy(graph)


# ---- 5 / 6. the phase plan with device actors: graph replays against eager calls -----------------------------------------------------
def _stub_session(R, N):
    """`run` for everything the device actors do not answer: fixed buffers, so a captured consumer reads the same addresses"""
    bufs = {"q": torch.zeros(R * N * 5, dtype=torch.float64, device=DEV)}

    def run(ops, feed):
        assert ops not in (["action_samples_target"], ["probs"]), ops            # the device actors answer these
        rows = max([v.shape[0] for v in feed.values() if torch.is_tensor(v) and v.dim() > 0] or [1])
        return [None if (op.endswith("_op") or op == "list_update_target_ops") else bufs["q"][:rows] for op in ops]
    return run, bufs


def _same_feeds(a, b, where):
    assert [ops for ops, _ in a] == [ops for ops, _ in b], where
    n = 0
    for (ops, fa), (_, fb) in zip(a, b):
        assert sorted(fa) == sorted(fb), (where, ops)
        for name in fb:
            if torch.is_tensor(fb[name]):
                assert fa[name].dtype == fb[name].dtype and fa[name].shape == fb[name].shape, (where, ops, name)
                assert torch.equal(fa[name], fb[name]), (where, ops, name)
                n += 1
            else:
                assert fa[name] == fb[name], (where, ops, name)
    return n


def _plan_against_eager(env, ro, N, sample_inputs):
    """Two plans over one rollout and one pair of actors, from equal counters: every feed of every step equal, the counters equal;
    the target actor is soft-updated after step 1 of the first phase (a replay reads the persistent packed weights); the sampled
    target actions of every step are the restated stream's at the draw the step must have used."""
    from cm3_amd import batch as BR
    from cm3_amd.actor import RowsDrawCounter
    M, K, eps, c0 = 3, 16, 0.5, WRAP - 4                                         # (the counter wraps inside the second phase)
    R = K * N
    main, target = env.actor(N, "f16x3", wseed=3), env.actor(N, "f16x3", wseed=4)
    run, bufs = _stub_session(R, N)
    kw = dict(epochs=M, batch_size=K, target_actor=target, actor=main)
    plan_g = BR.OnPolicyPhasePlan(ro, run, 0.99, eps, use_graph=True, draw_counter=RowsDrawCounter(DEV, c0), **kw)
    plan_e = BR.OnPolicyPhasePlan(ro, run, 0.99, eps, use_graph=False, draw_counter=RowsDrawCounter(DEV, c0), **kw)
    assert plan_g.draw_counter is not plan_e.draw_counter
    g = torch.Generator(device=DEV).manual_seed(5)
    first, ptrs, checked = {}, None, 0
    for phase in range(2):
        bufs["q"].copy_(torch.rand(R * N * 5, generator=g, device=DEV, dtype=torch.float64))
        # the SAME minibatches in both phases and both plans: what differs between the phases is the draw (and, after the update,
        # the target weights)
        plan_g.refresh(torch.Generator(device=DEV).manual_seed(9))
        plan_e.refresh(torch.Generator(device=DEV).manual_seed(9))
        now = {k: v.data_ptr() for k, v in plan_g.cols.items()}
        ptrs = ptrs or now
        assert ptrs == now                                                       # persistent addresses
        for k in range(M):
            cg, ce = plan_g.step(k), plan_e.step(k)
            torch.cuda.synchronize()
            checked += _same_feeds(cg, ce, (phase, k))
            assert plan_g.draw_counter.value() == plan_e.draw_counter.value() == (c0 + phase * M + k + 1) % WRAP, (phase, k)
            assert plan_g.draw_counter.arrivals() == 0 and plan_e.draw_counter.arrivals() == 0
            assert cg[1][0] == ["Q_global_target"]
            onehot = cg[1][1]["action_one"]                                      # action_samples_target through the one-hot path
            assert onehot.dtype == torch.int64 and tuple(onehot.shape) == (R, 5) and bool((onehot.sum(1) == 1).all())
            acts = onehot.argmax(1).cpu().numpy()
            cols, _ = plan_g.minibatch(k)
            probs = target.probs_rows(*sample_inputs(cols), eps).cpu().numpy()   # (the weights the step saw: before any update below)
            u = RR.rows_uniforms(SEED, R, (c0 + phase * M + k) % WRAP)
            assert np.array_equal(acts, env.sample(probs, u)), (phase, k)
            if k == 0:
                first[phase] = (acts.copy(), {n: v.clone() for n, v in cols.items()}, probs, u)
            if phase == 0 and k == 1:
                target.soft_update_from(main, 0.5)
    assert checked >= 2 * M * 40
    assert len(plan_g._graphs) == M and sorted(plan_g._keep) == list(range(M)) and all(plan_g._keep[k] for k in range(M))
    # step 0 of the two phases: the same columns, other samples -- the draws are not frozen into the graph
    (a0, cols0, _, u0), (a1, cols1, probs1, _) = first[0], first[1]
    assert all(torch.equal(cols0[n], cols1[n]) for n in cols0)
    assert not np.array_equal(a0, a1)
    assert not np.array_equal(a1, env.sample(probs1, u0))                        # (phase 2 at phase 1's draw would have been this)
    assert main.rows_draw == 0 and target.rows_draw == 0                         # the host counters were never used
    plan_g.close()
    plan_e.close()
    assert plan_g._graphs == {} and plan_g._calls == {} and plan_g._keep == {}


def test_plan_with_device_actors_particle():
    from cm3_amd.particle import VecParticleEnv
    from cm3_amd.rollout import ParticleRollout
    N = 4
    env = VecParticleEnv(load_cfg("particle_stage2_cross.json"), N, 0.2, 33, 8, device=DEV, dtype=torch.float32, auto_reset=True, seed=8)
    env.reset()
    ro = ParticleRollout(env, n_ticks=33, use_graph=False)
    ro.collect()

    def sample_inputs(cols):
        B = cols["v_global"].shape[0]
        return (cols["obs_others_next"].reshape(B * N, -1), cols["v_local_next"].reshape(B * N, -1), cols["goals"].reshape(B * N, -1))
    _plan_against_eager(_Particle, ro, N, sample_inputs)
    ro.close()


def test_plan_with_device_actors_checkers():
    from cm3_amd.checkers import VecCheckersEnv
    from cm3_amd.rollout import CheckersRollout
    cfg = load_cfg("checkers_stage2.json")
    N = cfg["n_agents"]
    assert N == 2
    env = VecCheckersEnv(cfg["init"], N, 9, 8, device=DEV, seed=31, auto_reset=True)
    ro = CheckersRollout(env, n_ticks=40, use_graph=False).collect(goals=np.eye(2))

    def sample_inputs(cols):
        B = cols["vec"].shape[0]
        rows = lambda x: x.reshape(B * N, *x.shape[2:])                          # noqa: E731
        return (rows(cols["next_obs_self_t"]), rows(cols["next_obs_self_v"]), rows(cols["next_obs_others"]), cols["actions"].reshape(-1),
                rows(cols["goals"]))
    _plan_against_eager(_Checkers, ro, N, sample_inputs)
    ro.close()


# ---- 7. without actors the plan is the plan of before ---------------------------------------------------------------------------------
def test_plan_without_actors_is_unchanged():
    from cm3_amd import batch as BR
    from cm3_amd.particle import VecParticleEnv
    from cm3_amd.rollout import ParticleRollout
    N, M, K = 4, 3, 16
    R = K * N
    env = VecParticleEnv(load_cfg("particle_stage2_cross.json"), N, 0.2, 33, 8, device=DEV, dtype=torch.float32, auto_reset=True, seed=8)
    env.reset()
    ro = ParticleRollout(env, n_ticks=33, use_graph=False)
    bufs = {"acts": torch.zeros(R, dtype=torch.int64, device=DEV), "probs": torch.zeros(R, 5, dtype=torch.float64, device=DEV),
            "q": torch.zeros(R * N * 5, dtype=torch.float64, device=DEV)}

    def run(ops, feed):
        rows = max([v.shape[0] for v in feed.values() if torch.is_tensor(v) and v.dim() > 0] or [1])
        answer = {"action_samples_target": bufs["acts"], "probs": bufs["probs"]}
        return [None if (op.endswith("_op") or op == "list_update_target_ops") else answer.get(op, bufs["q"][:rows]) for op in ops]

    plan = BR.OnPolicyPhasePlan(ro, run, 0.99, 0.1, epochs=M, batch_size=K)
    assert plan.draw_counter is None and plan.target_actor is None and plan.actor is None
    g = torch.Generator(device=DEV).manual_seed(9)
    checked = 0
    for phase in range(2):
        ro.collect()
        bufs["acts"].copy_(torch.randint(0, 5, (R,), generator=g, device=DEV))
        bufs["probs"].copy_(torch.rand(R, 5, generator=g, device=DEV, dtype=torch.float64))
        bufs["q"].copy_(torch.rand(R * N * 5, generator=g, device=DEV, dtype=torch.float64))
        plan.refresh(g)
        for k in range(M):
            calls = plan.step(k)
            torch.cuda.synchronize()
            cols, _ = plan.minibatch(k)
            want = BR.train_step_feeds({n: v.clone() for n, v in cols.items()}, run, 0.99, 0.1, device_tiling=False)
            checked += _same_feeds(calls, want, (phase, k))
    assert checked >= 2 * M * 40
    # no actor launch was captured: nothing is held but the int32 form of `run`'s int64 actions, which the one-hot launch reads
    assert all(t.dtype == torch.int32 and t.numel() == R for k in range(M) for t in plan._keep[k])
    plan.close()
    ro.close()
