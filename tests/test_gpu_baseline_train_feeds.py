"""GPU: cm3_amd.batch.baseline_train_step_feeds on device columns.

1. With all six device networks: `run` is never called for the replaced ops (their entries still appear, in the reference's order);
   the TD feeds carry the bits of the networks' own launches on the base columns; `run` overwrites v_main.w / q_main.w in place at the
   optimiser steps and the later launches follow the new weights (repack() after V_op and after Q_op); every feed no network output
   enters equals the call without networks bit for bit.
2. With every network None the device-column call equals the host-column call bit for bit."""
import numpy as np
import pytest
import torch

from tests import baseline_feeds as BF
from tests import baseline_ref as BR
from tests.test_gpu_actor_rows_counted import _Particle, _same_feeds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA, EPS = 0.99, 0.1
REPLACED = (["V_target", "V"], ["action_samples_target"], ["Q_target"], ["Q", "probs"])


def _write_in_place(net, w, names):
    for short, t in net.w.items():
        t.copy_(torch.as_tensor(w[names[short]]))


@pytest.mark.parametrize("N,IAC", [(2, False), (4, False), (4, True), (3, True)])
def test_train_step_with_device_networks(N, IAC):
    from cm3_amd.baseline import COMA_NAMES, VALUE_NAMES, ParticleComaCritic, ParticleValue
    from cm3_amd.batch import baseline_train_step_feeds, rep_rows, td_target
    B, draw = 5, 17
    kind = "local" if IAC else "global"
    rng = np.random.default_rng(50 + N)
    wv = [BR.init_value_weights(rng, N, kind, scale=1.5) for _ in range(3)]       # target, main, what V_op trains main to
    wq = [BR.init_coma_weights(rng, N, scale=1.5) for _ in range(3)]
    cols = BF.make_cols(B, N, 900 + N, device=DEV)
    cols["done"] = (torch.arange(B) % 3 == 1).to(DEV)
    v_target, v_main = (ParticleValue(w, N, kind=kind, device=DEV) for w in wv[:2])
    q_target, q_main = (ParticleComaCritic(w, N, device=DEV) for w in wq[:2])
    target_actor, actor = _Particle.actor(N, "f32", wseed=3), _Particle.actor(N, "f32", wseed=4)
    use_Q = 0 if IAC else 1
    g = torch.Generator().manual_seed(N)
    v_res = torch.randn(B * N, 1, generator=g).to(DEV)
    seen = []

    def run(ops, feed):
        assert ops not in REPLACED, "run was called for %s" % ops
        seen.append(ops)
        if ops == ["V_op", "V"]:                              # the optimiser steps: new variables, written in place
            _write_in_place(v_main, wv[2], VALUE_NAMES[kind])
            return [None, v_res]
        if ops == ["Q_op"]:
            _write_in_place(q_main, wq[2], COMA_NAMES)
        return [None for _ in ops]

    nets = dict(v_target=v_target, v_main=v_main, target_actor=target_actor, actor=actor, q_target=q_target, q_main=q_main)
    if IAC:                                                   # (IAC trains no COMA critic: the reference never runs those ops)
        nets.update(q_target=None, q_main=None, actor=None)
    # what the launches must give, from the networks' own methods on the base columns BEFORE the step changes any weight
    v_args = (cols["obs_others_next"], cols["v_local_next"], cols["goals"]) if IAC else (cols["v_global_next"], cols["goals"])
    want_v_td = v_target.v_rows(*v_args, cols["reward_local"], cols["done"], GAMMA)["td"].clone()
    v_next = v_main.v_rows(*v_args)["v64"].clone()
    got = baseline_train_step_feeds(cols, run, GAMMA, EPS, IAC=IAC, use_Q=use_Q, use_V=1, draw=draw, **nets)
    torch.cuda.synchronize()
    ops_all = [["V_target", "V"], ["V_op", "V"]]
    if not IAC:
        ops_all += [["action_samples_target"], ["Q_target"], ["Q_op"], ["Q", "probs"]]
    ops_all += [["policy_op"], ["list_update_target_ops"]]
    assert [ops for ops, _ in got] == ops_all
    assert seen == [ops for ops in ops_all if ops not in REPLACED]
    feeds = {tuple(ops): f for ops, f in got}
    not_done = -(rep_rows(cols["done"], N).to(torch.int64) - 1)
    assert torch.equal(feeds[("V_op", "V")]["V_td_target"], want_v_td)
    assert torch.equal(feeds[("policy_op",)]["V_td_target"], td_target(cols["reward_local"].reshape(-1), v_next, not_done, GAMMA))
    assert torch.equal(feeds[("policy_op",)]["V_evaluated"], v_res.reshape(-1))
    # v_main was repacked after V_op: its next launch follows the weights `run` wrote, not the ones it was built with
    fresh = ParticleValue(wv[2], N, kind=kind, device=DEV)
    assert torch.equal(v_main.v_rows(*v_args)["v"], fresh.v_rows(*v_args)["v"]) and not torch.equal(fresh.v_rows(*v_args)["v64"], v_next)
    if not IAC:
        acts = target_actor.sample_rows(cols["obs_others_next"].reshape(B * N, -1), cols["v_local_next"].reshape(B * N, -1),
                                        cols["goals"].reshape(B * N, -1), EPS, draw=draw)["actions"]
        a_others = feeds[("Q_target",)]["action_others"]
        from cm3_amd.batch import process_actions
        assert torch.equal(a_others, process_actions(acts.reshape(B, N))[1])
        td = q_target.q_rows(cols["v_global_next"], cols["goals"], acts, cols["v_local_next"], cols["reward"], cols["done"], GAMMA)["td"]
        assert torch.equal(feeds[("Q_op",)]["Q_td_target"], td)
        # Q is read AFTER the optimiser step on Q_main: the launch followed the weights `run` wrote at Q_op
        new = ParticleComaCritic(wq[2], N, device=DEV).q_rows(cols["v_global"], cols["goals"], cols["actions"], cols["v_local"])["q"]
        old = ParticleComaCritic(wq[1], N, device=DEV).q_rows(cols["v_global"], cols["goals"], cols["actions"], cols["v_local"])["q"]
        assert torch.equal(feeds[("policy_op",)]["Q_evaluated"], new) and not torch.equal(new, old)
        probs = actor.probs_rows(cols["obs_others"].reshape(B * N, -1), cols["v_local"].reshape(B * N, -1), cols["goals"].reshape(B * N, -1), EPS)
        assert torch.equal(feeds[("policy_op",)]["probs_evaluated"], probs)
        BF.within(new.cpu().numpy(), BF.coma_ref_on_feed(wq[2], feeds[("Q", "probs")], np.float64), what="Q after Q_op, N=%d" % N)
    # every feed that no network output enters equals the call without networks
    blank = baseline_train_step_feeds(cols, BF.blank_run(torch.zeros(B * N, dtype=torch.long), dev=DEV), GAMMA, EPS, IAC=IAC, use_Q=use_Q)
    from_networks = {"V_td_target", "V_evaluated", "Q_td_target", "Q_evaluated", "probs_evaluated", "action_others"}
    n = 0
    for (ops, fa), (_, fb) in zip(got, blank):
        assert sorted(fa) == sorted(fb), ops
        for name in fb:
            if name in from_networks and not (name == "action_others" and ops != ["Q_target"]):
                continue
            if torch.is_tensor(fb[name]):
                assert fa[name].dtype == fb[name].dtype and torch.equal(fa[name], fb[name]), (ops, name)
                n += 1
            else:
                assert fa[name] == fb[name], (ops, name)
    assert n >= (10 if IAC else 30)


@pytest.mark.parametrize("N,IAC,use_Q,use_V", [(4, True, 0, 1), (4, False, 1, 0), (3, False, 1, 1), (1, True, 0, 1), (1, False, 1, 1)])
def test_without_networks_device_columns_equal_host_columns(N, IAC, use_Q, use_V):
    from cm3_amd.batch import baseline_train_step_feeds
    B = 6
    host = BF.make_cols(B, N, 70 + N)
    host["done"] = torch.arange(B) % 3 == 1
    acts = torch.as_tensor(np.random.default_rng(N).integers(0, 5, B * N))
    g = torch.Generator().manual_seed(3)
    fixed = {"V_target": torch.randn(B * N, 1, generator=g), "V": torch.randn(B * N, 1, generator=g),
             "Q_target": torch.randn(B * N, 5, generator=g), "Q": torch.randn(B * N, 5, generator=g),
             "probs": torch.rand(B * N, 5, generator=g), "action_samples_target": acts}

    def run_on(dev):
        return lambda ops, feed: [None if (op.endswith("_op") or op == "list_update_target_ops") else fixed[op].to(dev) for op in ops]
    a = baseline_train_step_feeds(host, run_on("cpu"), GAMMA, EPS, IAC=IAC, use_Q=use_Q, use_V=use_V)
    b = baseline_train_step_feeds({k: v.to(DEV) for k, v in host.items()}, run_on(DEV), GAMMA, EPS, IAC=IAC, use_Q=use_Q, use_V=use_V,
                                  target_actor=None, actor=None, v_target=None, v_main=None, q_target=None, q_main=None)
    torch.cuda.synchronize()
    moved = [(ops, {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in f.items()}) for ops, f in b]
    assert _same_feeds(moved, a, "host against device") >= 8
