"""GPU: the Checkers QMIX learner (cm3_qmix_learner_checkers_grad_f32 + cm3_adam_step_f32; cm3_amd.qmix.CheckersQmixLearner) -- loss and
the twenty gradients against tests/qmix_learner_checkers_ref.py in float64, the kink at exactly zero, step = gradients + Adam bit for
bit, five steps on a fixed batch, the sums across tiles and chunks, a hipGraph of step, train_step and
qmix_train_step_feeds(env="checkers", learner=).

Bound: the project's 2e-5 (tests/critic_feeds.py:BOUND), per tensor: |got - ref| <= 2e-5 * max(1, max |ref tensor|).  The parity
cases (qmix_learner_checkers_ref.CASES) keep every float64 pre-activation of a relu or abs at least 3e-5 from zero; the helper asserts
it.  Float32 autograd uses at most 0.053 of the bound on the gradients and the loss (tests/test_qmix_learner_checkers_oracle.py); the
device sums in another order, so its share is its own: each test prints it."""
import numpy as np
import pytest
import torch

from tests import critic_feeds as CF
from tests import qmix_learner_checkers_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA, TAU = 0.99, 0.01
_CACHE = {}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _case(N, B, seed):
    """(named weights, device columns, td float64 on the device, the float64 reference): once per case, left unchanged"""
    key = (N, B, seed)
    if key not in _CACHE:
        wa, wm, cols, td, w, ref = (LR.cached_case(N, B, seed) if key in LR.CASES
                                    else LR.case(N, B, seed) + (None, None))
        _CACHE[key] = (w, {k: v.to(DEV) for k, v in cols.items()}, torch.as_tensor(td).to(DEV), ref)
        _CACHE[("host",) + key] = (wa, wm, cols, td)
    return _CACHE[key]


def _nets(N, seed, weights=None, precision="f32", **kw):
    """a fresh (agent, mixer, learner) on the weights of case (N, ., seed)"""
    from cm3_amd.qmix import CheckersQmixAgent, CheckersQmixLearner, CheckersQmixMixer
    wa, wm = weights if weights is not None else LR.case(N, 1, seed)[:2]
    agent, mixer = CheckersQmixAgent(wa, N, device=DEV, precision=precision), CheckersQmixMixer(wm, N, device=DEV)
    return agent, mixer, CheckersQmixLearner(agent, mixer, **kw)


def _fresh_from(agent, mixer):
    """new objects built from the TF-shaped tensors the two hold now"""
    from cm3_amd.qmix import CK_MIXER_NAMES, CK_NAMES, CheckersQmixAgent, CheckersQmixMixer
    a = CheckersQmixAgent({CK_NAMES[k]: v.cpu().numpy() for k, v in agent.w.items()}, agent.n, device=DEV)
    m = CheckersQmixMixer({CK_MIXER_NAMES[k]: v.cpu().numpy() for k, v in mixer.w.items()}, mixer.n, device=DEV)
    return a, m


def _within(got, ref, what, shares=None):
    """per tensor: prints the share of 2e-5 * max(1, max |ref|) used, then asserts it"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    used = float(np.abs(got - ref).max()) / (CF.BOUND * max(1.0, float(np.abs(ref).max())))
    print("%s: max |ref| %.4g, share of the bound used %.3f" % (what, float(np.abs(ref).max()), used))
    if shares is not None:
        shares.append((used, what))
    assert used <= 1.0, (what, used)


def _state(learner):
    """every tensor a step changes, cloned"""
    out = {"w/" + k: v.clone() for k, v in learner.w.items()}
    out.update({"m/" + k: v.clone() for k, v in learner.m.items()})
    out.update({"v/" + k: v.clone() for k, v in learner.v.items()})
    out["powers"] = learner.powers.clone()
    return out


def _assert_same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert _same(a[k], b[k]), k


def _agent_args(cols, B, N):
    rows = lambda x: x.reshape(B * N, *x.shape[2:])      # noqa: E731
    return (rows(cols["obs_self_t"]), rows(cols["obs_self_v"]), rows(cols["obs_others"]), cols["actions_prev"].reshape(B * N),
            rows(cols["goals"]))


def _q_sel(agent, cols, B, N):
    q = agent.greedy_rows(*_agent_args(cols, B, N), q=True, onehot=False)["q"]
    return q.gather(1, cols["actions"].reshape(-1, 1).long()).reshape(B, N)


def _check_grads(out, learner, ref, tag):
    shares = []
    _within(out["loss"].cpu().numpy().reshape(()), ref["loss"], "loss " + tag, shares)
    for k in LR.NAMES:
        g = out["grads"][k]
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(learner.w[k].shape), k
        _within(g.cpu().numpy(), ref["grads"][k], "grad %s %s" % (k, tag), shares)
    print("largest share %s: %.3f (%s)" % ((tag,) + max(shares)))


# ---- 1. gradients and loss against float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,seed", LR.CASES)
def test_gradients_and_loss_match_float64(N, B, seed):
    """Measured on an MI355X: the largest share of the bound over a case's loss and twenty gradients is 0.029, 0.049, 0.038, 0.027,
    0.040, 0.029, 0.026 in the order of CASES (profiles/r32_qmix_learner_checkers.txt)."""
    from cm3_amd import _lib
    w, cols, td, ref = _case(N, B, seed)
    agent, mixer, learner = _nets(N, seed)
    assert sorted(learner.w) == sorted(LR.NAMES) and all(learner.w["agent/" + k] is agent.w[k] for k in agent.w)
    before = _state(learner)
    out = learner.gradients(cols, td)
    torch.cuda.synchronize()
    variant = _lib.last_kernel_variant()
    assert variant.startswith("k_qmix_learner_checkers_reduce<f32,N=%d," % N), variant
    assert variant.endswith(",after=stage+6gemm+mixer+4gemm+xtd>"), variant      # (the thirteen launches before it)
    assert sorted(out) == ["grads", "loss", "q_tot"] and sorted(out["grads"]) == sorted(LR.NAMES)
    assert out["loss"].dtype == torch.float32 and tuple(out["loss"].shape) == (1,)
    assert out["q_tot"].dtype == torch.float32 and tuple(out["q_tot"].shape) == (B, 1)
    _check_grads(out, learner, ref, "N=%d B=%d" % (N, B))
    # it changes nothing
    _assert_same_state(before, _state(learner))
    # q_tot is the mixer's launch on the agent's own Q values at the taken actions, bit for bit
    q_sel = _q_sel(agent, cols, B, N)
    _within(q_sel.cpu().numpy(), ref["q_sel"], "q_sel N=%d B=%d" % (N, B))
    assert _same(mixer.q_tot(cols["grid"], cols["vec"], cols["goals"], q_sel)["q_tot"], out["q_tot"])
    # the compact forms -- int8 windows and grids, uint8 index goals -- go in unwidened and give the same bits
    keep = {k: v.clone() for k, v in out["grads"].items()}
    narrow = dict(cols)
    narrow["obs_self_t"], narrow["grid"] = cols["obs_self_t"].to(torch.int8), cols["grid"].to(torch.int8)
    narrow["goals"] = cols["goals"][..., 1].to(torch.uint8)
    again = learner.gradients(narrow, td.float())
    assert _same(again["q_tot"], out["q_tot"]) and _same(again["loss"], out["loss"])
    for k in LR.NAMES:
        assert _same(again["grads"][k], keep[k]), k


def test_the_forward_pass_is_float32_whatever_the_agents_precision():
    """the learner's forward pass is exact float32 on agent.w: an agent at split float16 trains on the same gradients"""
    N, B, seed = 3, 13, 0
    w, cols, td, _ = _case(N, B, seed)
    _, _, a = _nets(N, seed)
    _, _, b = _nets(N, seed, precision="f16x3")
    ga, gb = a.gradients(cols, td), b.gradients(cols, td)
    assert _same(ga["q_tot"], gb["q_tot"]) and _same(ga["loss"], gb["loss"])
    for k in LR.NAMES:
        assert _same(ga["grads"][k], gb["grads"][k]), k


# ---- 2. the kink at exactly zero -----------------------------------------------------------------------------------------------------
def test_relu_grad_passes_nothing_at_exactly_zero():
    """both conv biases 0.0, an all-zero window and an all-zero grid: 150 + 108 conv pre-activations are exactly 0 in any precision.
    "> 0" matches the float64 reference; ">= 0" would move conv_b's gradients by thousands of bounds
    (tests/test_qmix_learner_checkers_oracle.py).  Measured on an MI355X: the largest share of the bound 0.064 (agent/lin_b)."""
    wa, wm, cols, td = LR.kink_case()
    N, B = LR.KINK[0], LR.KINK[1]
    w = LR.short_weights(wa, wm)
    ref = LR.loss_and_grads(w, cols, td)
    assert int((ref["pre"]["conv"][0] == 0).sum()) == 150 and int((ref["pre"]["mixer_conv"][0] == 0).sum()) == 108
    _, _, learner = _nets(N, None, weights=(wa, wm))
    out = learner.gradients({k: v.to(DEV) for k, v in cols.items()}, torch.as_tensor(td).to(DEV))
    _check_grads(out, learner, ref, "kink N=%d B=%d" % (N, B))


# ---- 3. step is gradients followed by Adam -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,seed", [(3, 13, 0), (2, 40, 265)])
def test_step_is_gradients_then_adam_bit_for_bit(N, B, seed):
    from cm3_amd.qmix import _GUARD
    w, cols, td, _ = _case(N, B, seed)
    agent_a, mixer_a, a = _nets(N, seed, max_batch=64)
    agent_b, mixer_b, b = _nets(N, seed, max_batch=64)
    agent_c, mixer_c, c = _nets(N, seed, max_batch=64)
    untouched = _state(c)
    canary = -7.5
    a._grad_store.fill_(canary)
    a._workspace.fill_(canary)
    loss = a.step(cols, td)
    out = b.gradients(cols, td)
    assert _same(loss, out["loss"])
    for k in LR.NAMES:
        assert _same(a.grads[k], b.grads[k]), k
    b.enqueue_adam()
    _assert_same_state(_state(a), _state(b))
    for k in LR.NAMES:
        assert not _same(a.w[k], c.w[k]), k
    _assert_same_state(untouched, _state(c))
    # the launches follow the new weights: both networks were repacked
    args = _agent_args(cols, B, N)
    fresh_agent, fresh_mixer = _fresh_from(agent_a, mixer_a)
    q = agent_a.greedy_rows(*args, q=True, onehot=False)["q"]
    assert _same(q, fresh_agent.greedy_rows(*args, q=True, onehot=False)["q"])
    assert not _same(q, agent_c.greedy_rows(*args, q=True, onehot=False)["q"])
    aq = q[:, 0].reshape(B, N)
    qt = mixer_a.q_tot(cols["grid"], cols["vec"], cols["goals"], aq)["q_tot"]
    assert _same(qt, fresh_mixer.q_tot(cols["grid"], cols["vec"], cols["goals"], aq)["q_tot"])
    assert not _same(qt, mixer_c.q_tot(cols["grid"], cols["vec"], cols["goals"], aq)["q_tot"])
    # canaries: past the workspace's used part and past every gradient tensor
    used = a.workspace_floats(a.max_batch)
    assert a._workspace.numel() == used + _GUARD and bool((a._workspace[used:] == canary).all())
    assert a.workspace_floats(B) <= used and not bool((a._workspace[:a.workspace_floats(B)] == canary).all())
    mask = torch.ones_like(a._grad_store, dtype=torch.bool)
    for k, g in a.grads.items():
        at = (g.data_ptr() - a._grad_store.data_ptr()) // 4
        mask[at:at + g.numel()] = False
        assert not bool((g == canary).any()), k
    assert int(mask.sum()) >= 20 * _GUARD and bool((a._grad_store[mask] == canary).all())


# ---- 4. five steps on a fixed batch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,seed", LR.CASES)
def test_five_steps_follow_the_float64_trajectory(N, B, seed):
    """Five losses within 2e-5 * max(1, |loss|) of the float64 trajectory (the loss is continuous across the kinks: no margin
    condition).  Measured on an MI355X: the largest share of the bound per case 0.347, 0.441, 0.355, 0.052, 0.091, 0.029, 0.099 in the
    order of CASES (the float32 NumPy restatement: 0.373, 0.390, 0.342, 0.049, 0.095, 0.029, 0.104)."""
    w, cols, td, _ = _case(N, B, seed)
    host = _CACHE[("host", N, B, seed)]
    want = LR.trajectory(w, host[2], host[3], 5)
    _, _, learner = _nets(N, seed, max_batch=64)
    got = [learner.step(cols, td) for _ in range(5)]
    got = [float(x.cpu()[0]) for x in got]
    used = [abs(g - r) / (CF.BOUND * max(1.0, abs(r))) for g, r in zip(got, want)]
    print("five losses N=%d B=%d: %s; float64 %s; shares of the bound used %s"
          % (N, B, ["%.6g" % x for x in got], ["%.6g" % x for x in want], ["%.3f" % x for x in used]))
    assert max(used) <= 1.0, used


# ---- 5. reduction across tiles and chunks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,seed", [(2, 128, 5), (8, 40, 5)])
def test_the_whole_batch_is_the_combination_of_its_halves(N, B, seed):
    """N = 2, B = 128: the workload's shape, 6400 patch rows in 25 chunks.  N = 8, B = 40: 320 agent rows, more than one 256-row chunk
    of every agent job.  Device against device: no margin condition."""
    w, cols, td, _ = _case(N, B, seed)
    half = B // 2
    _, _, learner = _nets(N, seed)
    first = learner.gradients(cols, td)
    whole = {k: v.clone() for k, v in first["grads"].items()}
    loss = first["loss"].clone()
    second = learner.gradients(cols, td)
    assert _same(second["loss"], loss) and _same(second["q_tot"], first["q_tot"])
    for k in LR.NAMES:
        assert _same(second["grads"][k], whole[k]), k
    halves = []
    for lo in (0, half):
        part = learner.gradients({k: v[lo:lo + half] for k, v in cols.items()}, td[lo:lo + half])
        assert _same(part["q_tot"], first["q_tot"][lo:lo + half])
        halves.append(({k: v.cpu().numpy().astype(np.float64) for k, v in part["grads"].items()}, float(part["loss"].cpu()[0])))
    _within(loss.cpu().numpy().reshape(()), (halves[0][1] + halves[1][1]) / 2, "loss of the halves")
    for k in LR.NAMES:
        _within(whole[k].cpu().numpy(), (halves[0][0][k] + halves[1][0][k]) / 2, "grad %s of the halves" % k)


# ---- 6. a hipGraph of step -------------------------------------------------------------------------------------------------------------
def test_a_captured_step_replays_as_three_eager_steps():
    from cm3_amd import _lib
    N, B, seed = 3, 13, 0
    w, cols, td, _ = _case(N, B, seed)
    _, _, eager = _nets(N, seed, max_batch=16)
    agent, mixer, learner = _nets(N, seed, max_batch=16)
    for _ in range(3):
        eager.step(cols, td)
    start = _state(learner)
    box, keep = {}, []

    def enqueue(stream):
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=DEV)):
            box["loss"] = learner.step(cols, td, keep=keep)
    graph = _lib.capture_graph(DEV, enqueue)
    try:
        assert any(t is box["loss"] for t in keep)                     # the outputs are held by the caller's list
        torch.cuda.synchronize()
        _assert_same_state(start, _state(learner))                     # a capture launches nothing
        stream = torch.cuda.current_stream(DEV)
        losses = []
        for _ in range(3):
            _lib.check(_lib.lib().cm3_graph_launch(graph, stream.cuda_stream))
            losses.append(box["loss"].clone())
        torch.cuda.synchronize()
    finally:
        _lib.check(_lib.lib().cm3_graph_destroy(graph))
    _assert_same_state(_state(eager), _state(learner))
    assert float(losses[0].cpu()[0]) != float(losses[2].cpu()[0])
    assert np.allclose(learner.powers.cpu().numpy(), [0.9 ** 4, 0.999 ** 4], rtol=1e-6)      # the powers advanced on the device
    # the packed copies followed too
    args = _agent_args(cols, B, N)
    assert _same(agent.greedy_rows(*args, q=True, onehot=False)["q"], eager.agent.greedy_rows(*args, q=True, onehot=False)["q"])
    # a batch larger than the workspace was sized for cannot grow it inside a capture
    _, _, small = _nets(N, seed, max_batch=8)

    def too_large(stream):
        with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=DEV)):
            with pytest.raises(Exception, match="a capture cannot allocate"):
                small.step(cols, td)
            small.agent.repack()                                                                # (a capture of something)
    _lib.check(_lib.lib().cm3_graph_destroy(_lib.capture_graph(DEV, too_large)))
    small.step(cols, td)                                                                       # outside of one it grows
    assert small.max_batch == B


# ---- 7. train_step and qmix_train_step_feeds(env="checkers", learner=) -------------------------------------------------------------------
def _targets(N):
    from cm3_amd.qmix import CheckersQmixAgent, CheckersQmixMixer
    from tests import qmix_checkers_ref as QC
    from tests import qmix_mixer_checkers_ref as MC
    rng = np.random.default_rng(4242 + N)
    return (CheckersQmixAgent(QC.init_weights(rng, N), N, device=DEV),
            CheckersQmixMixer(MC.init_weights(rng, N, scale=0.5, scope="Mixer_target"), N, device=DEV))


@pytest.mark.parametrize("N,B,seed", [(2, 3, 0), (3, 13, 0)])
def test_train_step_and_the_feeds_with_a_learner(N, B, seed):
    from cm3_amd.batch import qmix_train_step_feeds
    w, cols, td, _ = _case(N, B, seed)
    seen = []

    def run(ops, feed):
        seen.append(ops)
        assert ops != ["mixer_op"] or allow_mixer_op, "run was called for mixer_op"
        return [None for _ in ops]
    # without a learner: the recorded list, and the TD target the device computes on the MAIN agent's Q at the target's argmax
    allow_mixer_op = True
    t_agent, t_mixer = _targets(N)
    agent, mixer, learner = _nets(N, seed, max_batch=16)
    plain = qmix_train_step_feeds(cols, run, GAMMA, env="checkers", target_agent=t_agent, target_mixer=t_mixer, mixer_q_agent=agent)
    assert seen == [["mixer_op"], ["list_update_target_ops"]]
    td_dev = plain[2][1]["td_target"]
    # with one
    allow_mixer_op = False
    del seen[:]
    calls = qmix_train_step_feeds(cols, run, GAMMA, env="checkers", target_agent=t_agent, target_mixer=t_mixer, mixer_q_agent=agent,
                                  learner=learner)
    assert seen == [["list_update_target_ops"]]
    assert [ops for ops, _ in calls] == [ops for ops, _ in plain] == [["argmax_Q_target"], ["mixer_target"], ["mixer_op"],
                                                                      ["list_update_target_ops"]]
    for (_, fa), (_, fb) in zip(calls, plain):
        assert list(fa) == list(fb)
        for k in fa:
            assert fa[k].dtype == fb[k].dtype and torch.equal(fa[k], fb[k]), k
    # the weights after the call are learner.step's on the same TD target
    _, _, other = _nets(N, seed, max_batch=16)
    other.step(cols, td_dev)
    _assert_same_state(_state(other), _state(learner))
    # train_step: the same step, then both soft updates
    t_agent2, t_mixer2 = _targets(N)
    _, _, whole = _nets(N, seed, max_batch=16)
    loss = whole.train_step(cols, GAMMA, t_agent2, t_mixer2, TAU)
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (1,)
    _assert_same_state(_state(other), _state(whole))
    t_agent.soft_update_from(agent, TAU)
    t_mixer.soft_update_from(mixer, TAU)
    for k in t_agent.w:
        assert _same(t_agent.w[k], t_agent2.w[k]), k
    for k in t_mixer.w:
        assert _same(t_mixer.w[k], t_mixer2.w[k]), k
    # the refusals, with their messages
    from cm3_amd.qmix import ParticleQmixAgent, ParticleQmixLearner, ParticleQmixMixer
    from tests import qmix_learner_ref as PLR
    pa, pm, _, _ = PLR.case(N, 1, 1)
    particle = ParticleQmixLearner(ParticleQmixAgent(pa, N, device=DEV), ParticleQmixMixer(pm, N, device=DEV), max_batch=1)
    with pytest.raises(ValueError, match="takes a CheckersQmixLearner as learner, got ParticleQmixLearner: the Checkers learner is not built"):
        qmix_train_step_feeds(cols, run, GAMMA, env="checkers", target_agent=t_agent, target_mixer=t_mixer, learner=particle)
    with pytest.raises(ValueError, match="pass target_agent and target_mixer"):
        qmix_train_step_feeds(cols, run, GAMMA, env="checkers", target_agent=t_agent, learner=learner)
    _, _, wrong = _nets(N + 1, seed, max_batch=1)
    with pytest.raises(ValueError, match="learner is built for %d agents, the batch has %d" % (N + 1, N)):
        qmix_train_step_feeds(cols, run, GAMMA, env="checkers", target_agent=t_agent, target_mixer=t_mixer, learner=wrong)
