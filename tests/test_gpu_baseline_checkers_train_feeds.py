"""GPU: cm3_amd.batch.baseline_train_step_feeds(env="checkers") on device columns, in the three configurations IAC, COMA and both
critics.

1. With all device networks `run` is never called for the replaced ops (their entries still appear, in the reference's order); `run`
   overwrites v_main.w / q_main.w in place at the optimiser steps and the later launches follow the new weights (repack() after V_op
   and after Q_op).  Every feed still handed to `run` equals the feed of the path WITHOUT device networks bit for bit -- there torch
   networks of the same weights (float64, tests/baseline_checkers_feeds.torch_net) answer inside `run`, with the same sampled target
   actions and the same actor probabilities -- except the feeds a device network's values enter (V_td_target, Q_td_target,
   Q_evaluated): those stay within the project's bound 2e-5 * max(1, |ref|) of that path's.
2. With every network None the device-column call equals the host-column call bit for bit."""
import numpy as np
import pytest
import torch

from tests import baseline_checkers_feeds as BF
from tests import baseline_checkers_ref as BR
from tests.test_gpu_actor_rows_counted import _Checkers, _same_feeds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA, EPS = 0.99, 0.1
REPLACED = (["V_target", "V"], ["action_samples_target"], ["Q_target"], ["Q", "probs"])
CONFIGS = {"iac": dict(IAC=True, use_V=1, use_Q=0), "coma": dict(IAC=False, use_V=0, use_Q=1), "both": dict(IAC=False, use_V=1, use_Q=1)}
FROM_NETWORKS = ("V_td_target", "Q_td_target", "Q_evaluated")


def _write_in_place(net, w, names):
    for short, t in net.w.items():
        t.copy_(torch.as_tensor(w[names[short]]))


@pytest.mark.parametrize("N,config", [(2, "iac"), (2, "coma"), (2, "both"), (3, "both"), (5, "iac")])
def test_train_step_with_device_networks(N, config):
    from cm3_amd.baseline import CK_COMA_NAMES, CK_VALUE_NAMES, CheckersComaCritic, CheckersValue
    from cm3_amd.batch import baseline_train_step_feeds
    cfg = CONFIGS[config]
    B, draw = 5, 17
    kind = "local" if cfg["IAC"] else "global"
    rng = np.random.default_rng(50 + N)
    wv = [BR.init_value_weights(rng, N, kind) for _ in range(3)]                  # target, main, what V_op trains main to
    wq = [BR.init_coma_weights(rng, N) for _ in range(3)]
    cols = BF.make_cols(B, N, 900 + N, device=DEV)
    cols["done"] = (torch.arange(B) % 3 == 1).to(DEV)
    nets = {}
    if cfg["use_V"]:
        nets["v_target"], nets["v_main"] = (CheckersValue(w, N, kind=kind, device=DEV) for w in wv[:2])
    if cfg["use_Q"]:
        nets["q_target"], nets["q_main"] = (CheckersComaCritic(w, N, device=DEV) for w in wq[:2])
        nets["target_actor"], nets["actor"] = _Checkers.actor(N, "f32", wseed=3), _Checkers.actor(N, "f32", wseed=4)
    rows = lambda x: x.reshape(B * N, *x.shape[2:])      # noqa: E731
    goals_self = rows(cols["goals"])
    acts = probs = None
    if cfg["use_Q"]:      # what the two actors give on the base columns: the no-network path's `run` answers with the same values
        acts = nets["target_actor"].sample_rows(rows(cols["next_obs_self_t"]), rows(cols["next_obs_self_v"]), rows(cols["next_obs_others"]),
                                                cols["actions"].reshape(-1), goals_self, EPS, draw=draw)["actions"].clone()
        probs = nets["actor"].probs_rows(rows(cols["obs_self_t"]), rows(cols["obs_self_v"]), rows(cols["obs_others"]),
                                         cols["actions_prev"].reshape(-1), goals_self, EPS).clone()
    seen = []

    def run_device(ops, feed):
        assert ops not in REPLACED, "run was called for %s" % ops
        seen.append(ops)
        if ops == ["V_op", "V"]:                              # the optimiser steps: new variables, written in place
            _write_in_place(nets["v_main"], wv[2], CK_VALUE_NAMES[kind])
            return [None, BF.torch_net(wv[1], feed, kind, N)]
        if ops == ["Q_op"]:
            _write_in_place(nets["q_main"], wq[2], CK_COMA_NAMES)
        return [None for _ in ops]

    def run_torch(ops, feed):
        if ops == ["V_target", "V"]:
            return [BF.torch_net(wv[0], feed, kind, N), BF.torch_net(wv[1], feed, kind, N)]
        if ops == ["V_op", "V"]:
            return [None, BF.torch_net(wv[1], feed, kind, N)]
        if ops == ["action_samples_target"]:
            return [acts]
        if ops == ["Q_target"]:
            return [BF.torch_net(wq[0], feed, "coma", N)]
        if ops == ["Q", "probs"]:                             # read AFTER the optimiser step on Q_main
            return [BF.torch_net(wq[2], feed, "coma", N), probs]
        return [None for _ in ops]

    got = baseline_train_step_feeds(cols, run_device, GAMMA, EPS, draw=draw, env="checkers", **cfg, **nets)
    torch.cuda.synchronize()
    ops_all = ([["V_target", "V"], ["V_op", "V"]] if cfg["use_V"] else []) + \
        ([["action_samples_target"], ["Q_target"], ["Q_op"], ["Q", "probs"]] if cfg["use_Q"] else []) + [["policy_op"], ["list_update_target_ops"]]
    assert [ops for ops, _ in got] == ops_all
    assert seen == [ops for ops in ops_all if ops not in REPLACED]
    want = baseline_train_step_feeds(cols, run_torch, GAMMA, EPS, env="checkers", **cfg)
    assert [ops for ops, _ in want] == ops_all
    n_equal = n_close = 0
    for (ops, fa), (_, fb) in zip(got, want):
        assert sorted(fa) == sorted(fb), ops
        for name in fb:
            if name in FROM_NETWORKS:
                if ops in REPLACED:       # (never handed to run)
                    continue
                assert fa[name].shape == fb[name].shape, (ops, name)
                BF.within(fa[name].cpu().numpy(), fb[name].cpu().numpy(), what="%s %s N=%d %s" % (ops, name, N, config))
                n_close += 1
            elif torch.is_tensor(fb[name]):
                assert fa[name].dtype == fb[name].dtype and torch.equal(fa[name], fb[name]), (ops, name)
                n_equal += 1
            else:
                assert fa[name] == fb[name], (ops, name)
    assert n_close == 2 * cfg["use_V"] + 2 * cfg["use_Q"] and n_equal >= (10 if config == "iac" else 18)
    # the launches followed the weights `run` wrote: a fresh network of those weights gives the same bits
    feeds = {tuple(ops): f for ops, f in got}
    if cfg["use_V"]:
        args = (cols["next_obs_self_t"], cols["next_obs_self_v"], cols["next_obs_others"], cols["goals"]) if cfg["IAC"] else \
            (cols["next_grid"], cols["next_vec"], cols["goals"])
        fresh, stale = (CheckersValue(w, N, kind=kind, device=DEV).v_rows(*args)["v"] for w in (wv[2], wv[1]))
        assert torch.equal(nets["v_main"].v_rows(*args)["v"], fresh) and not torch.equal(fresh, stale)
    if cfg["use_Q"]:
        args = (cols["grid"], cols["vec"], cols["goals"], cols["actions"], cols["obs_self_t"], cols["obs_self_v"])
        new, old = (CheckersComaCritic(w, N, device=DEV).q_rows(*args)["q"] for w in (wq[2], wq[1]))
        assert torch.equal(feeds[("policy_op",)]["Q_evaluated"], new) and not torch.equal(new, old)
        assert torch.equal(feeds[("policy_op",)]["probs_evaluated"], probs)


@pytest.mark.parametrize("N,config", [(2, "iac"), (3, "coma"), (2, "both"), (1, "iac")])
def test_without_networks_device_columns_equal_host_columns(N, config):
    from cm3_amd.batch import baseline_train_step_feeds
    cfg = CONFIGS[config]
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
    a = baseline_train_step_feeds(host, run_on("cpu"), GAMMA, EPS, env="checkers", **cfg)
    b = baseline_train_step_feeds({k: v.to(DEV) for k, v in host.items()}, run_on(DEV), GAMMA, EPS, env="checkers", target_actor=None,
                                  actor=None, v_target=None, v_main=None, q_target=None, q_main=None, **cfg)
    torch.cuda.synchronize()
    moved = [(ops, {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in f.items()}) for ops, f in b]
    assert _same_feeds(moved, a, "host against device") >= 8
