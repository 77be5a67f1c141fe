"""GPU: qmix_train_step_feeds(env="checkers") with a device target mixer (target_mixer=CheckersQmixMixer).

1. A train step with target_agent and target_mixer against the same call without target_mixer, where `run` answers mixer_target with
   the torch network (tests/qmix_mixer_checkers_ref.py:torch_mixer, float32 as a tf.float32 session) on the arrays it is fed -- agent_qs
   from the target agent's Q values times the fed actions_1hot: the same ops in the same order with the same feed keys, `run` called
   for neither target op, every feed equal bit for bit except mixer_op's td_target, which is within 2e-5 * max(1, |q_tot|) pushed
   through the TD arithmetic (gamma * that) and equals, bit for bit, qmix_td_target on the mixer's own q_tot.
2. The float64 / int64 one-hot columns and the compact int8 / uint8 ones give the same td_target bits.
3. The refusals of a target_mixer the function cannot use, on device columns.
4. A full step in the caller's order: feeds, soft_update_from on agent and mixer, and the next call evaluates the updated weights.
5. mixer_q_agent: the reference Checkers graph's own wiring of mixer_target (the MAIN agent's Q values at the target's argmax)."""
import numpy as np
import pytest
import torch

from tests import critic_checkers_feeds as CCF
from tests import critic_feeds as CF
from tests import qmix_checkers_ref as QC
from tests import qmix_mixer_checkers_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.99
B = 13
ORDER = [["argmax_Q_target"], ["mixer_target"], ["mixer_op"], ["list_update_target_ops"]]


def _agent(N, seed):
    from cm3_amd.qmix import CheckersQmixAgent
    return CheckersQmixAgent(QC.init_weights(np.random.default_rng(seed), N), N, device=DEV)


def _mixer(N, seed):
    from cm3_amd.qmix import CheckersQmixMixer
    return CheckersQmixMixer(MR.init_weights(np.random.default_rng(seed), N, scale=0.5, scope="Mixer_target"), N, device=DEV)


def _cols(N, seed):
    cols = CCF.make_cols(B, N, seed, device=DEV)
    assert 0 < int(cols["done"].sum()) < B
    return cols


def _session(seen, agent=None, mixer=None, q_seen=None):
    """`run`: answers mixer_target with the torch network when given the target agent and mixer, refuses the op otherwise"""
    def run(ops, feed):
        seen.append(ops)
        assert ops != ["argmax_Q_target"], "run was called for argmax_Q_target"
        if ops == ["mixer_target"]:
            assert mixer is not None, "run was called for mixer_target"
            q = agent.greedy_rows(feed["obs_self_t"], feed["obs_self_v"], feed["obs_others"], feed["actions_prev"].argmax(1), feed["v_goal"],
                                  q=True)["q"]
            n = feed["v_goal_all"].shape[1] // 2
            agent_qs = (q * feed["actions_1hot"].to(torch.float32)).sum(dim=1).reshape(-1, n)
            q_tot = MR.torch_mixer(mixer.w, agent_qs, feed["state_env"], feed["v_state"], feed["v_goal_all"])
            assert q_tot.dtype == torch.float32 and tuple(q_tot.shape) == (feed["v_state"].shape[0], 1)
            if q_seen is not None:
                q_seen.append(q_tot)
            return [q_tot]
        return [None]
    return run


@pytest.mark.parametrize("N", [2, 3])
def test_train_step_with_a_device_target_mixer(N):
    from cm3_amd.batch import qmix_td_target, qmix_train_step_feeds
    cols = _cols(N, 300 + N)
    agent, mixer = _agent(N, 10 + N), _mixer(N, 20 + N)
    seen_dev, seen_ref, q_ref = [], [], []
    got = qmix_train_step_feeds(cols, _session(seen_dev), GAMMA, target_agent=agent, target_mixer=mixer, env="checkers")
    want = qmix_train_step_feeds(cols, _session(seen_ref, agent, mixer, q_ref), GAMMA, target_agent=agent, env="checkers")
    torch.cuda.synchronize()
    assert seen_dev == ORDER[2:] and seen_ref == ORDER[1:]             # run was called for neither target op
    assert [(ops, sorted(f)) for ops, f in got] == [(ops, sorted(f)) for ops, f in want]
    assert [ops for ops, _ in got] == ORDER
    checked = 0
    for (ops, fa), (_, fb) in zip(got, want):
        for name in fb:
            assert fa[name].dtype == fb[name].dtype and fa[name].shape == fb[name].shape, (ops, name)
            if name == "td_target":
                q = q_ref[0].double().cpu().numpy().reshape(-1)
                diff = np.abs(fa[name].cpu().numpy() - fb[name].cpu().numpy())
                allowed = GAMMA * CF.BOUND * np.maximum(1.0, np.abs(q))
                print("td_target, N=%d: |q_tot| %.3f .. %.3f, share of the bound used %.3f"
                      % (N, float(np.abs(q).min()), float(np.abs(q).max()), float((diff / allowed).max())))
                assert fa[name].dtype == torch.float64 and tuple(fa[name].shape) == (B,)
                assert (diff <= allowed).all(), float((diff / allowed).max())
                checked += 1
            else:
                assert torch.equal(fa[name], fb[name]), (ops, name)
    assert checked == 1
    # the feed is the mixer's own launch on the batch's columns at the target agent's Q values, and qmix_td_target on its q_tot
    rows = lambda x: x.reshape(B * N, *x.shape[2:])                      # noqa: E731
    g = agent.greedy_rows(rows(cols["next_obs_self_t"]), rows(cols["next_obs_self_v"]), rows(cols["next_obs_others"]),
                          cols["actions"].reshape(B * N), rows(cols["goals"]), q_max=True)
    own = mixer.q_tot(cols["next_grid"], cols["next_vec"], cols["goals"], g["q_max"].reshape(B, N), cols["local_rewards"], cols["done"], GAMMA)
    assert torch.equal(got[2][1]["td_target"], own["td"])
    assert torch.equal(got[2][1]["td_target"], qmix_td_target(cols["local_rewards"].reshape(B, N), own["q_tot"], cols["done"], GAMMA))
    # without target_mixer nothing changes: the same call twice, and with target_mixer=None spelled out
    again = qmix_train_step_feeds(cols, _session([], agent, mixer), GAMMA, target_agent=agent, target_mixer=None, env="checkers")
    for (ops, fa), (_, fb) in zip(again, want):
        assert sorted(fa) == sorted(fb) and all(torch.equal(fa[k], fb[k]) for k in fb), ops


@pytest.mark.parametrize("N", [2, 3])
def test_compact_columns_give_the_same_td_target(N):
    from cm3_amd.batch import qmix_train_step_feeds
    cols = _cols(N, 400 + N)
    compact = dict(cols)
    for k in ("grid", "next_grid", "obs_self_t", "next_obs_self_t"):
        compact[k] = cols[k].to(torch.int8)
    compact["goals"] = cols["goals"].argmax(dim=2).to(torch.uint8)
    agent, mixer = _agent(N, 30 + N), _mixer(N, 40 + N)
    wide = qmix_train_step_feeds(cols, _session([]), GAMMA, target_agent=agent, target_mixer=mixer, env="checkers")
    narrow = qmix_train_step_feeds(compact, _session([]), GAMMA, target_agent=agent, target_mixer=mixer, env="checkers")
    torch.cuda.synchronize()
    assert narrow[1][1]["state_env"].dtype == torch.int8 and narrow[1][1]["v_goal_all"].dtype == torch.uint8
    assert torch.equal(wide[2][1]["td_target"].view(torch.int64), narrow[2][1]["td_target"].view(torch.int64))


@pytest.mark.parametrize("N", [2, 3])
def test_mixer_q_agent_evaluates_the_reference_graphs_wiring(N):
    """alg_qmix_checkers.py:106 builds mixer_target on mixer_q_input: Agent_main's Q values on the fed next observations, selected by
    the fed one-hot actions (the target agents' argmax).  With mixer_q_agent=main the device path evaluates that: against a `run` that
    plays that session with the torch mixer, and bit for bit against the mixer's own launch on the main agent's gathered Q values."""
    from cm3_amd.batch import qmix_train_step_feeds
    cols = _cols(N, 500 + N)
    target, main, mixer = _agent(N, 50 + N), _agent(N, 60 + N), _mixer(N, 70 + N)
    q_ref = []
    got = qmix_train_step_feeds(cols, _session([]), GAMMA, target_agent=target, target_mixer=mixer, mixer_q_agent=main, env="checkers")
    want = qmix_train_step_feeds(cols, _session([], main, mixer, q_ref), GAMMA, target_agent=target, env="checkers")
    plain = qmix_train_step_feeds(cols, _session([]), GAMMA, target_agent=target, target_mixer=mixer, env="checkers")
    torch.cuda.synchronize()
    assert [(ops, sorted(f)) for ops, f in got] == [(ops, sorted(f)) for ops, f in want]
    for (ops, fa), (_, fb) in zip(got, want):
        for name in fb:
            if name != "td_target":
                assert torch.equal(fa[name], fb[name]), (ops, name)
    q = q_ref[0].double().cpu().numpy().reshape(-1)
    diff = np.abs(got[2][1]["td_target"].cpu().numpy() - want[2][1]["td_target"].cpu().numpy())
    allowed = GAMMA * CF.BOUND * np.maximum(1.0, np.abs(q))
    print("td_target with mixer_q_agent, N=%d: share of the bound used %.3f" % (N, float((diff / allowed).max())))
    assert (diff <= allowed).all(), float((diff / allowed).max())
    rows = lambda x: x.reshape(B * N, *x.shape[2:])                      # noqa: E731
    args = (rows(cols["next_obs_self_t"]), rows(cols["next_obs_self_v"]), rows(cols["next_obs_others"]), cols["actions"].reshape(B * N),
            rows(cols["goals"]))
    a = target.greedy_rows(*args)["argmax"].long()
    q_main = main.greedy_rows(*args, q=True)["q"]
    agent_qs = (q_main * torch.nn.functional.one_hot(a, 5).to(torch.float32)).sum(dim=1)            # reduce_sum(agent_qs * actions_1hot)
    own = mixer.q_tot(cols["next_grid"], cols["next_vec"], cols["goals"], agent_qs.reshape(B, N), cols["local_rewards"], cols["done"], GAMMA)
    assert torch.equal(got[2][1]["td_target"], own["td"])
    assert not torch.equal(got[2][1]["td_target"], plain[2][1]["td_target"])                       # (the default: the target agents' Q)

    def never(ops, feed):
        raise AssertionError("run was called: the refusal must come first")
    with pytest.raises(ValueError, match="mixer_q_agent names the agent .* pass target_mixer as well"):
        qmix_train_step_feeds(cols, never, GAMMA, target_agent=target, mixer_q_agent=main, env="checkers")
    with pytest.raises(ValueError, match="mixer_q_agent must be a CheckersQmixAgent for %d agents" % N):
        qmix_train_step_feeds(cols, never, GAMMA, target_agent=target, target_mixer=mixer, mixer_q_agent=mixer, env="checkers")
    with pytest.raises(ValueError, match="mixer_q_agent must be a CheckersQmixAgent for %d agents" % N):
        qmix_train_step_feeds(cols, never, GAMMA, target_agent=target, target_mixer=mixer, mixer_q_agent=_agent(N + 1, 1), env="checkers")


def test_refusals():
    from cm3_amd.batch import qmix_train_step_feeds
    from cm3_amd.qmix import ParticleQmixMixer
    from tests import qmix_mixer_ref as PMR
    N = 2
    cols = _cols(N, 7)
    host = CCF.make_cols(B, N, 7)
    agent, mixer = _agent(N, 1), _mixer(N, 2)
    particle = ParticleQmixMixer(PMR.init_weights(np.random.default_rng(3), N), N, device=DEV)

    def never(ops, feed):
        raise AssertionError("run was called: the refusal must come first")
    with pytest.raises(ValueError, match="pass target_agent"):
        qmix_train_step_feeds(cols, never, GAMMA, target_mixer=mixer, env="checkers")
    with pytest.raises(ValueError, match="target_mixer evaluates device columns; call without it"):
        qmix_train_step_feeds(host, never, GAMMA, target_agent=agent, target_mixer=mixer, env="checkers")
    with pytest.raises(ValueError, match="for 2 agents .the batch's count., got one for 3"):
        qmix_train_step_feeds(cols, never, GAMMA, target_agent=agent, target_mixer=_mixer(3, 3), env="checkers")
    with pytest.raises(ValueError, match="takes a CheckersQmixMixer as target_mixer, got ParticleQmixMixer: the Checkers mixer is not built"):
        qmix_train_step_feeds(cols, never, GAMMA, target_agent=agent, target_mixer=particle, env="checkers")
    with pytest.raises(ValueError, match="takes a CheckersQmixMixer as target_mixer, got CheckersQmixAgent"):
        qmix_train_step_feeds(cols, never, GAMMA, target_agent=agent, target_mixer=agent, env="checkers")
    pcols = CF.make_cols(B, N, 7, device=DEV)
    with pytest.raises(ValueError, match="takes a ParticleQmixMixer for 2 agents .the batch's count., got CheckersQmixMixer"):
        qmix_train_step_feeds(pcols, never, GAMMA, target_agent=agent, target_mixer=mixer)


def test_a_full_step_in_the_callers_order():
    from cm3_amd.batch import qmix_train_step_feeds
    from cm3_amd.qmix import CK_MIXER_NAMES, CK_NAMES, CheckersQmixAgent, CheckersQmixMixer
    N, tau = 3, 0.25
    cols = _cols(N, 55)
    target_agent, main_agent = _agent(N, 1), _agent(N, 2)
    target_mixer, main_mixer = _mixer(N, 3), _mixer(N, 4)
    trained = MR.init_weights(np.random.default_rng(5), N, scale=0.5)          # what the optimiser step leaves in Mixer_main

    def run(ops, feed):
        assert ops in ORDER[2:], ops
        if ops == ["mixer_op"]:                                                # the session trains the main mixer: variables written in place
            for short, t in main_mixer.w.items():
                t.copy_(torch.as_tensor(trained[CK_MIXER_NAMES[short]]))
        return [None]

    first = qmix_train_step_feeds(cols, run, GAMMA, target_agent=target_agent, target_mixer=target_mixer, env="checkers")
    # what list_update_target_ops computes, in float32, from the variables as they stand after the optimiser step
    want_agent = {CK_NAMES[k]: (tau * main_agent.w[k] + (1.0 - tau) * target_agent.w[k]).cpu().numpy() for k in CK_NAMES}
    want_mixer = {CK_MIXER_NAMES[s]: (tau * torch.as_tensor(trained[CK_MIXER_NAMES[s]]).to(DEV) + (1.0 - tau) * target_mixer.w[s]).cpu().numpy()
                  for s in CK_MIXER_NAMES}
    target_agent.soft_update_from(main_agent, tau)
    target_mixer.soft_update_from(main_mixer, tau)
    second = qmix_train_step_feeds(cols, run, GAMMA, target_agent=target_agent, target_mixer=target_mixer, env="checkers")
    fresh = qmix_train_step_feeds(cols, run, GAMMA, target_agent=CheckersQmixAgent(want_agent, N, device=DEV),
                                  target_mixer=CheckersQmixMixer(want_mixer, N, device=DEV), env="checkers")
    torch.cuda.synchronize()
    assert torch.equal(second[2][1]["td_target"], fresh[2][1]["td_target"])
    assert not torch.equal(second[2][1]["td_target"], first[2][1]["td_target"])
    assert torch.equal(second[1][1]["actions_1hot"], fresh[1][1]["actions_1hot"])
