"""GPU: qmix_train_step_feeds with a device target mixer (target_mixer=ParticleQmixMixer).

1. A train step with target_agent and target_mixer against the same call without target_mixer, where `run` answers mixer_target with
   the torch network (tests/qmix_mixer_ref.py:torch_mixer, float32 as a tf.float32 session) on the arrays it is fed -- agent_qs
   from the target agent's Q values times the fed actions_1hot, as the graph selects them: the same ops in the same order with the
   same feed keys, `run` called for neither target op, every feed equal bit for bit except mixer_op's td_target, which is within
   2e-5 * max(1, |q_tot|) pushed through the TD arithmetic (gamma * that).
2. The refusals of a target_mixer the function cannot use.
3. A full step in the caller's order: feeds, soft_update_from on agent and mixer, and the next call evaluates the updated weights."""
import numpy as np
import pytest
import torch

from tests import critic_feeds as CF
from tests import qmix_mixer_ref as MR
from tests import qmix_ref as QR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.99
B = 13
ORDER = [["argmax_Q_target"], ["mixer_target"], ["mixer_op"], ["list_update_target_ops"]]


def _agent(N, seed):
    from cm3_amd.qmix import ParticleQmixAgent
    return ParticleQmixAgent(QR.init_weights(np.random.default_rng(seed), N, scale=1.0), N, device=DEV)


def _mixer(N, seed):
    from cm3_amd.qmix import ParticleQmixMixer
    return ParticleQmixMixer(MR.init_weights(np.random.default_rng(seed), N, scale=0.5, scope="Mixer_target"), N, device=DEV)


def _session(seen, agent=None, mixer=None, q_seen=None):
    """`run`: answers mixer_target with the torch network when given the target agent and mixer, refuses the op otherwise"""
    def run(ops, feed):
        seen.append(ops)
        assert ops != ["argmax_Q_target"], "run was called for argmax_Q_target"
        if ops == ["mixer_target"]:
            assert mixer is not None, "run was called for mixer_target"
            q = agent.greedy_rows(feed["obs_others"], feed["v_obs"], feed["v_goal"], q=True)["q"]
            n = feed["v_goal_all"].shape[1] // 2
            agent_qs = (q * feed["actions_1hot"].to(torch.float32)).sum(dim=1).reshape(-1, n)        # q_target_selected (alg_qmix.py:106-107)
            q_tot = MR.torch_mixer(mixer.w, agent_qs, feed["v_state"], feed["v_goal_all"])
            assert q_tot.dtype == torch.float32 and tuple(q_tot.shape) == (feed["v_state"].shape[0], 1)
            if q_seen is not None:
                q_seen.append(q_tot)
            return [q_tot]
        return [None]
    return run


@pytest.mark.parametrize("N", [2, 4])
def test_train_step_with_a_device_target_mixer(N):
    from cm3_amd.batch import qmix_train_step_feeds
    cols = CF.make_cols(B, N, 300 + N, device=DEV)
    assert 0 < int(cols["done"].sum()) < B
    agent, mixer = _agent(N, 10 + N), _mixer(N, 20 + N)
    seen_dev, seen_ref, q_ref = [], [], []
    got = qmix_train_step_feeds(cols, _session(seen_dev), GAMMA, target_agent=agent, target_mixer=mixer)
    want = qmix_train_step_feeds(cols, _session(seen_ref, agent, mixer, q_ref), GAMMA, target_agent=agent)
    torch.cuda.synchronize()
    assert seen_dev == ORDER[2:] and seen_ref == ORDER[1:]             # run was called for neither target op
    assert [ops for ops, _ in got] == ORDER == [ops for ops, _ in want]
    checked = 0
    for (ops, fa), (_, fb) in zip(got, want):
        assert sorted(fa) == sorted(fb), ops
        for name in fb:
            assert fa[name].dtype == fb[name].dtype and fa[name].shape == fb[name].shape, (ops, name)
            if name == "td_target":
                q = q_ref[0].double().cpu().numpy().reshape(-1)
                diff = np.abs(fa[name].cpu().numpy() - fb[name].cpu().numpy())
                allowed = GAMMA * CF.BOUND * np.maximum(1.0, np.abs(q))
                print("td_target, N=%d: max |q_tot| %.3f, share of the bound used %.3f" % (N, float(np.abs(q).max()), float((diff / allowed).max())))
                assert fa[name].dtype == torch.float64 and tuple(fa[name].shape) == (B,)
                assert (diff <= allowed).all(), float((diff / allowed).max())
                checked += 1
            else:
                assert torch.equal(fa[name], fb[name]), (ops, name)
    assert checked == 1
    # the feed is the mixer's own launch on the batch's columns at the target agent's Q values
    g = agent.greedy_rows(cols["obs_others_next"].reshape(B * N, -1), cols["v_local_next"].reshape(B * N, -1), cols["goals"].reshape(B * N, -1),
                          q_max=True)
    td = mixer.q_tot(cols["v_global_next"], cols["goals"], g["q_max"].reshape(B, N), cols["reward_local"], cols["done"], GAMMA)["td"]
    assert torch.equal(got[2][1]["td_target"], td)
    # without target_mixer nothing changes: the same call twice, and with target_mixer=None spelled out
    again = qmix_train_step_feeds(cols, _session([], agent, mixer), GAMMA, target_agent=agent, target_mixer=None)
    for (ops, fa), (_, fb) in zip(again, want):
        assert sorted(fa) == sorted(fb) and all(torch.equal(fa[k], fb[k]) for k in fb), ops


def test_refusals():
    from cm3_amd.batch import qmix_train_step_feeds
    N = 2
    cols = CF.make_cols(B, N, 7, device=DEV)
    host = CF.make_cols(B, N, 7)
    agent, mixer = _agent(N, 1), _mixer(N, 2)

    def never(ops, feed):
        raise AssertionError("run was called: the refusal must come first")
    with pytest.raises(ValueError, match="pass target_agent"):
        qmix_train_step_feeds(cols, never, GAMMA, target_mixer=mixer)
    with pytest.raises(ValueError, match="target_mixer evaluates device columns; call without it"):
        qmix_train_step_feeds(host, never, GAMMA, target_agent=agent, target_mixer=mixer)
    with pytest.raises(ValueError, match="for 2 agents .the batch's count., got one for 4"):
        qmix_train_step_feeds(cols, never, GAMMA, target_agent=agent, target_mixer=_mixer(4, 3))
    with pytest.raises(ValueError, match="takes a ParticleQmixMixer for 2 agents"):
        qmix_train_step_feeds(cols, never, GAMMA, target_agent=agent, target_mixer=agent)
    with pytest.raises(ValueError, match="the Checkers mixer is not built"):
        qmix_train_step_feeds({}, never, GAMMA, env="checkers", target_mixer=mixer)


def test_a_full_step_in_the_callers_order():
    from cm3_amd.batch import qmix_train_step_feeds
    from cm3_amd.qmix import MIXER_NAMES, NAMES, ParticleQmixAgent, ParticleQmixMixer
    N, tau = 4, 0.25
    cols = CF.make_cols(B, N, 55, device=DEV)
    target_agent, main_agent = _agent(N, 1), _agent(N, 2)
    target_mixer, main_mixer = _mixer(N, 3), _mixer(N, 4)
    trained = MR.init_weights(np.random.default_rng(5), N, scale=0.5)          # what the optimiser step leaves in Mixer_main

    def run(ops, feed):
        assert ops in ORDER[2:], ops
        if ops == ["mixer_op"]:                                                # the session trains the main mixer: variables written in place
            for short, t in main_mixer.w.items():
                t.copy_(torch.as_tensor(trained[MIXER_NAMES[short]]))
        return [None]

    first = qmix_train_step_feeds(cols, run, GAMMA, target_agent=target_agent, target_mixer=target_mixer)
    # what list_update_target_ops computes, in float32, from the variables as they stand after the optimiser step
    want_agent = {k: (tau * main_agent.w[k] + (1.0 - tau) * target_agent.w[k]).cpu().numpy() for k in NAMES}
    want_mixer = {MIXER_NAMES[s]: (tau * torch.as_tensor(trained[MIXER_NAMES[s]]).to(DEV) + (1.0 - tau) * target_mixer.w[s]).cpu().numpy()
                  for s in MIXER_NAMES}
    target_agent.soft_update_from(main_agent, tau)
    target_mixer.soft_update_from(main_mixer, tau)
    second = qmix_train_step_feeds(cols, run, GAMMA, target_agent=target_agent, target_mixer=target_mixer)
    fresh = qmix_train_step_feeds(cols, run, GAMMA, target_agent=ParticleQmixAgent(want_agent, N, device=DEV),
                                  target_mixer=ParticleQmixMixer(want_mixer, N, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(second[2][1]["td_target"], fresh[2][1]["td_target"])
    assert not torch.equal(second[2][1]["td_target"], first[2][1]["td_target"])
    assert torch.equal(second[1][1]["actions_1hot"], fresh[1][1]["actions_1hot"])
