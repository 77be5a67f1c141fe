"""GPU: the particle QMIX learner (cm3_qmix_learner_particle_grad_f32, cm3_adam_step_f32; cm3_amd.qmix.ParticleQmixLearner) -- loss and
the eleven gradients against tests/qmix_learner_ref.py in float64, Adam on its own, step = gradients + Adam bit for bit, five steps on
a fixed batch, the sums across workgroups and chunks at the workload's shape, a hipGraph of step, train_step and
qmix_train_step_feeds(learner=).

Bound: the project's 2e-5 (tests/critic_feeds.py:BOUND), per tensor: |got - ref| <= 2e-5 * max(1, max |ref tensor|).  The parity
cases (qmix_learner_ref.CASES) keep every float64 pre-activation of a relu or abs at least 1e-4 from zero; the helper asserts it.  A
float32 NumPy restatement uses at most 0.03 of the bound on the gradients and the loss (tests/test_qmix_learner_oracle.py); the
device sums in another order, so its share is its own: each test prints it."""
import ctypes

import numpy as np
import pytest
import torch

from tests import critic_feeds as CF
from tests import qmix_learner_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA, TAU = 0.99, 0.01
_CACHE = {}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _case(N, B, seed):
    """(short-named weights, device columns, td float64 on the device, the float64 reference): once per case, left unchanged"""
    key = (N, B, seed)
    if key not in _CACHE:
        wa, wm, cols, td = LR.case(N, B, seed)
        w = LR.short_weights(wa, wm)
        ref = LR.loss_and_grads(w, cols, td, check_margin=key in LR.CASES)
        _CACHE[key] = (w, {k: v.to(DEV) for k, v in cols.items()}, torch.as_tensor(td).to(DEV), ref)
        _CACHE[("host",) + key] = (cols, td)
    return _CACHE[key]


def _nets(N, seed, **kw):
    """a fresh (agent, mixer, learner) on the weights of case (N, ., seed)"""
    from cm3_amd.qmix import ParticleQmixAgent, ParticleQmixLearner, ParticleQmixMixer
    wa, wm, _, _ = LR.case(N, 1, seed)
    agent, mixer = ParticleQmixAgent(wa, N, device=DEV), ParticleQmixMixer(wm, N, device=DEV)
    return agent, mixer, ParticleQmixLearner(agent, mixer, **kw)


def _fresh_from(agent, mixer):
    """new objects built from the TF-shaped tensors the two hold now"""
    from cm3_amd.qmix import MIXER_NAMES, ParticleQmixAgent, ParticleQmixMixer
    a = ParticleQmixAgent({k: v.cpu().numpy() for k, v in agent.w.items()}, agent.n, device=DEV)
    m = ParticleQmixMixer({MIXER_NAMES[k]: v.cpu().numpy() for k, v in mixer.w.items()}, mixer.n, device=DEV)
    return a, m


def _within(got, ref, what):
    """per tensor: prints the share of 2e-5 * max(1, max |ref|) used, then asserts it"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    used = float(np.abs(got - ref).max()) / (CF.BOUND * max(1.0, float(np.abs(ref).max())))
    print("%s: max |ref| %.4g, share of the bound used %.3f" % (what, float(np.abs(ref).max()), used))
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


# ---- 1. gradients and loss against float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,seed", LR.CASES)
def test_gradients_and_loss_match_float64(N, B, seed):
    from cm3_amd import _lib
    w, cols, td, ref = _case(N, B, seed)
    agent, mixer, learner = _nets(N, seed)
    before = _state(learner)
    out = learner.gradients(cols, td)
    torch.cuda.synchronize()
    variant = _lib.last_kernel_variant()
    assert variant.startswith("k_qmix_learner_reduce<f32,N=%d," % N), variant
    assert variant.endswith(",after=fwd+mixer+bwd+xtd>"), variant      # (k_learner_agent_fwd, _mixer, _agent_bwd, _xtd ran before it)
    assert sorted(out) == ["grads", "loss", "q_tot"] and sorted(out["grads"]) == sorted(LR.NAMES)
    assert out["loss"].dtype == torch.float32 and tuple(out["loss"].shape) == (1,)
    assert out["q_tot"].dtype == torch.float32 and tuple(out["q_tot"].shape) == (B, 1)
    _within(out["loss"].cpu().numpy().reshape(()), ref["loss"], "loss N=%d B=%d" % (N, B))
    for k in LR.NAMES:
        g = out["grads"][k]
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(learner.w[k].shape), k
        _within(g.cpu().numpy(), ref["grads"][k], "grad %s N=%d B=%d" % (k, N, B))
    # it changes nothing
    _assert_same_state(before, _state(learner))
    # q_tot is the mixer's launch on the agent's own Q values at the taken actions, bit for bit
    rows = lambda x: x.reshape(B * N, -1)      # noqa: E731
    q = agent.greedy_rows(rows(cols["obs_others"]), rows(cols["v_local"]), rows(cols["goals"]), q=True, onehot=False)["q"]
    q_sel = q.gather(1, cols["actions"].reshape(-1, 1).long()).reshape(B, N)
    _within(q_sel.cpu().numpy(), ref["q_sel"], "q_sel N=%d B=%d" % (N, B))
    assert _same(mixer.q_tot(cols["v_global"], cols["goals"], q_sel)["q_tot"], out["q_tot"])
    # float64 columns are rounded to float32 as everywhere else: the same launches
    wide = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in cols.items()}
    keep = {k: v.clone() for k, v in out["grads"].items()}
    again = learner.gradients(wide, td.float().double())
    assert _same(again["q_tot"], out["q_tot"])
    for k in LR.NAMES:
        assert _same(again["grads"][k], keep[k]), k


# ---- 2. Adam on its own -------------------------------------------------------------------------------------------------------------
def test_adam_alone_over_three_steps():
    """cm3_adam_step_f32 on the device's own gradients read back, scaled per tensor by 1, 1e-3, 1e3, 1e-6, ... with every seventh
    element an exact zero, over three consecutive steps, against the float64 restatement on those same float32 gradients.  The bound is
    measured per quantity (var, m, v, the two powers): 4 x the largest deviation of the FLOAT32 NumPy restatement of the same formulas
    from the float64 one on these inputs (the factor for the device's sqrt and division rounding).  Measured on the host with the
    float64 gradients of this case, rounded to float32, standing in for the device's: var 4.0e-8 on weights up to 0.55 (less than
    float32's spacing there), m 2.0e-3 on moments up to 8.1e3, v 37 on up to 2.9e6, the powers 8.7e-8; the test measures them again
    on the gradients it applies and prints both sides."""
    N, B, seed = 4, 37, 111
    w, cols, td, _ = _case(N, B, seed)
    agent, mixer, learner = _nets(N, seed)
    base = {k: v.clone() for k, v in learner.gradients(cols, td)["grads"].items()}
    scales = [1.0, 1e-3, 1e3, 1e-6, 30.0, 1e-2, 1.0, 1e2, 1e-4, 1e3, 1.0]
    W64 = {k: v.cpu().numpy().astype(np.float64) for k, v in learner.w.items()}
    m64, v64, p64 = LR.adam_state(W64)
    W32 = {k: v.cpu().numpy() for k, v in learner.w.items()}
    m32, v32, p32 = LR.adam_state(W32, dtype=np.float32)
    dev32 = {"var": 0.0, "m": 0.0, "v": 0.0, "powers": 0.0}
    worst = dict(dev32)
    for step in range(3):
        grads = {}
        for (k, g), s in zip(base.items(), scales):
            g = (g * (s * (1.0 + step))).clone()
            g.reshape(-1)[step::7] = 0.0
            grads[k] = g
            learner.grads[k].copy_(g)
        learner.enqueue_adam()
        torch.cuda.synchronize()
        from cm3_amd import _lib
        assert _lib.last_kernel_variant().startswith("k_adam_step<f32,"), _lib.last_kernel_variant()
        host = {k: g.cpu().numpy() for k, g in grads.items()}
        W64, m64, v64, p64 = LR.adam_step(W64, host, m64, v64, p64)
        W32, m32, v32, p32 = LR.adam_step(W32, host, m32, v32, p32, dtype=np.float32)
        got = {"var": learner.w, "m": learner.m, "v": learner.v}
        for q, r64, r32 in (("var", W64, W32), ("m", m64, m32), ("v", v64, v32)):
            dev32[q] = max(dev32[q], max(float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) for k in r64))
            worst[q] = max(worst[q], max(float(np.abs(got[q][k].cpu().numpy().astype(np.float64) - r64[k]).max()) for k in r64))
        dev32["powers"] = max(dev32["powers"], float(np.abs(p32.astype(np.float64) - p64).max()))
        worst["powers"] = max(worst["powers"], float(np.abs(learner.powers.cpu().numpy().astype(np.float64) - p64).max()))
    for q in dev32:
        print("adam %s: float32 restatement deviates %.3g, the device %.3g (bound 4 x the former)" % (q, dev32[q], worst[q]))
    for q in dev32:
        assert worst[q] <= 4.0 * dev32[q], (q, worst[q], dev32[q])
    # the powers after three steps, and an exact zero gradient from the start leaves its weight where it was
    assert np.allclose(learner.powers.cpu().numpy(), [0.9 ** 4, 0.999 ** 4], rtol=1e-6)
    # the arrival counter is back at zero
    assert learner._state[2:].view(torch.int32).tolist() == [0, 0]


# ---- 3. step is gradients followed by Adam -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,seed", [(3, 13, 0), (4, 37, 111)])
def test_step_is_gradients_then_adam_bit_for_bit(N, B, seed):
    from cm3_amd.qmix import _GUARD
    w, cols, td, _ = _case(N, B, seed)
    agent_a, mixer_a, a = _nets(N, seed)
    agent_b, mixer_b, b = _nets(N, seed)
    agent_c, mixer_c, c = _nets(N, seed)
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
    assert not _same(a.w["h/kernel"], c.w["h/kernel"]) and not _same(a.w["w1"], c.w["w1"])
    _assert_same_state(untouched, _state(c))
    # the launches follow the new weights: both networks were repacked
    rows = lambda x: x.reshape(B * N, -1)      # noqa: E731
    args = (rows(cols["obs_others"]), rows(cols["v_local"]), rows(cols["goals"]))
    fresh_agent, fresh_mixer = _fresh_from(agent_a, mixer_a)
    q = agent_a.greedy_rows(*args, q=True, onehot=False)["q"]
    assert _same(q, fresh_agent.greedy_rows(*args, q=True, onehot=False)["q"])
    assert not _same(q, agent_c.greedy_rows(*args, q=True, onehot=False)["q"])
    aq = q[:, 0].reshape(B, N)
    qt = mixer_a.q_tot(cols["v_global"], cols["goals"], aq)["q_tot"]
    assert _same(qt, fresh_mixer.q_tot(cols["v_global"], cols["goals"], aq)["q_tot"])
    assert not _same(qt, mixer_c.q_tot(cols["v_global"], cols["goals"], aq)["q_tot"])
    # canaries: past the workspace's used part and past every gradient tensor
    used = a.workspace_floats(a.max_batch)
    assert a._workspace.numel() == used + _GUARD and bool((a._workspace[used:] == canary).all())
    assert a.workspace_floats(B) <= used and not bool((a._workspace[:a.workspace_floats(B)] == canary).all())
    mask = torch.ones_like(a._grad_store, dtype=torch.bool)
    for k, g in a.grads.items():
        at = (g.data_ptr() - a._grad_store.data_ptr()) // 4
        mask[at:at + g.numel()] = False
        assert not bool((g == canary).any()), k
    assert int(mask.sum()) >= 11 * _GUARD and bool((a._grad_store[mask] == canary).all())


# ---- 4. five steps on a fixed batch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B,seed", LR.CASES)
def test_five_steps_follow_the_float64_trajectory(N, B, seed):
    """Five losses within 2e-5 * max(1, |loss|) of the float64 trajectory (the loss is continuous across the kinks: no margin
    condition).  Measured on an MI355X: the largest share of the bound per case 0.853 (N = 1, B = 1, the fourth loss; the float32
    NumPy restatement uses 0.83 there), 0.044, 0.248, 0.149, 0.330, 0.335, 0.064 in the order of CASES."""
    w, cols, td, _ = _case(N, B, seed)
    want = LR.trajectory(w, *_CACHE[("host", N, B, seed)], 5)
    _, _, learner = _nets(N, seed)
    got = [learner.step(cols, td) for _ in range(5)]
    got = [float(x.cpu()[0]) for x in got]
    used = [abs(g - r) / (CF.BOUND * max(1.0, abs(r))) for g, r in zip(got, want)]
    print("five losses N=%d B=%d: %s; float64 %s; shares of the bound used %s"
          % (N, B, ["%.6g" % x for x in got], ["%.6g" % x for x in want], ["%.3f" % x for x in used]))
    assert max(used) <= 1.0, used


# ---- 5. reduction across workgroups at the workload's shape -----------------------------------------------------------------------------
def test_the_whole_batch_is_the_combination_of_its_halves():
    N, B, seed = 4, 128, 5
    w, cols, td, ref = _case(N, B, seed)
    _, _, learner = _nets(N, seed)
    first = learner.gradients(cols, td)
    whole = {k: v.clone() for k, v in first["grads"].items()}
    loss = first["loss"].clone()
    second = learner.gradients(cols, td)
    assert _same(second["loss"], loss) and _same(second["q_tot"], first["q_tot"])
    for k in LR.NAMES:
        assert _same(second["grads"][k], whole[k]), k
    halves = []
    for lo in (0, 64):
        part = learner.gradients({k: v[lo:lo + 64] for k, v in cols.items()}, td[lo:lo + 64])
        assert _same(part["q_tot"], first["q_tot"][lo:lo + 64])
        halves.append(({k: v.cpu().numpy().astype(np.float64) for k, v in part["grads"].items()}, float(part["loss"].cpu()[0])))
    _within(loss.cpu().numpy().reshape(()), (64 * halves[0][1] + 64 * halves[1][1]) / 128, "loss of the halves")
    for k in LR.NAMES:
        _within(whole[k].cpu().numpy(), (64 * halves[0][0][k] + 64 * halves[1][0][k]) / 128, "grad %s of the halves" % k)


# ---- 6. a hipGraph of step -------------------------------------------------------------------------------------------------------------
def test_a_captured_step_replays_as_three_eager_steps():
    from cm3_amd import _lib
    N, B, seed = 4, 37, 111
    w, cols, td, _ = _case(N, B, seed)
    _, _, eager = _nets(N, seed)
    agent, mixer, learner = _nets(N, seed)
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
    rows = lambda x: x.reshape(B * N, -1)      # noqa: E731
    args = (rows(cols["obs_others"]), rows(cols["v_local"]), rows(cols["goals"]))
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


# ---- 7. train_step and qmix_train_step_feeds(learner=) -----------------------------------------------------------------------------------
def _targets(N):
    from cm3_amd.qmix import ParticleQmixAgent, ParticleQmixMixer
    from tests import qmix_mixer_ref as MR
    from tests import qmix_ref as QR
    rng = np.random.default_rng(4242 + N)
    return (ParticleQmixAgent(QR.init_weights(rng, N), N, device=DEV),
            ParticleQmixMixer(MR.init_weights(rng, N, scale=0.5, scope="Mixer_target"), N, device=DEV))


@pytest.mark.parametrize("N,B,seed", [(2, 3, 1), (4, 37, 111)])
def test_train_step_and_the_feeds_with_a_learner(N, B, seed):
    from cm3_amd.batch import qmix_train_step_feeds
    w, cols, td, _ = _case(N, B, seed)
    seen = []

    def run(ops, feed):
        seen.append(ops)
        assert ops != ["mixer_op"] or allow_mixer_op, "run was called for mixer_op"
        return [None for _ in ops]
    # without a learner: the recorded list, and the TD target the device computes
    allow_mixer_op = True
    t_agent, t_mixer = _targets(N)
    plain = qmix_train_step_feeds(cols, run, GAMMA, target_agent=t_agent, target_mixer=t_mixer)
    assert seen == [["mixer_op"], ["list_update_target_ops"]]
    td_dev = plain[2][1]["td_target"]
    # with one
    allow_mixer_op = False
    del seen[:]
    agent, mixer, learner = _nets(N, seed)
    calls = qmix_train_step_feeds(cols, run, GAMMA, target_agent=t_agent, target_mixer=t_mixer, learner=learner)
    assert seen == [["list_update_target_ops"]]
    assert [ops for ops, _ in calls] == [ops for ops, _ in plain] == [["argmax_Q_target"], ["mixer_target"], ["mixer_op"],
                                                                      ["list_update_target_ops"]]
    for (_, fa), (_, fb) in zip(calls, plain):
        assert list(fa) == list(fb)
        for k in fa:
            assert fa[k].dtype == fb[k].dtype and torch.equal(fa[k], fb[k]), k
    # the weights after the call are learner.step's on the same TD target
    _, _, other = _nets(N, seed)
    other.step(cols, td_dev)
    _assert_same_state(_state(other), _state(learner))
    # train_step: the same step, then both soft updates
    t_agent2, t_mixer2 = _targets(N)
    _, _, whole = _nets(N, seed)
    loss = whole.train_step(cols, GAMMA, t_agent2, t_mixer2, TAU)
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (1,)
    _assert_same_state(_state(other), _state(whole))
    t_agent.soft_update_from(agent, TAU)
    t_mixer.soft_update_from(mixer, TAU)
    for k in t_agent.w:
        assert _same(t_agent.w[k], t_agent2.w[k]), k
    for k in t_mixer.w:
        assert _same(t_mixer.w[k], t_mixer2.w[k]), k
    # both refusals, with their messages
    with pytest.raises(ValueError, match="the Checkers learner is not built"):
        qmix_train_step_feeds(cols, run, GAMMA, env="checkers", learner=learner)
    with pytest.raises(ValueError, match="pass target_agent and target_mixer"):
        qmix_train_step_feeds(cols, run, GAMMA, target_agent=t_agent, learner=learner)
    _, _, wrong = _nets(N + 1, seed)
    with pytest.raises(ValueError, match="learner is built for %d agents, the batch has %d" % (N + 1, N)):
        qmix_train_step_feeds(cols, run, GAMMA, target_agent=t_agent, target_mixer=t_mixer, learner=wrong)
