"""GPU: the CM3 Checkers critics over transition rows (cm3_critic_checkers_rows_f32; cm3_amd.critic.CheckersCritic) -- q_rows, q_pairs
and q_counterfactual against tests/critic_checkers_ref.py in float64 evaluated on the TILED feeds of the torch composition
(train_step_feeds(env="checkers", device_tiling=False)), so the kernel's row decoding -- the m-indexed windows and obs_self_v of
the pair forms included -- is checked independently of it; the fixtures recorded from the reference's own function bodies; the bit
identities between the forms, input dtypes and outputs; and the weight updates.

Bound: the project's 2e-5 * max(1, |ref|) per row.  Weights from init_weights(scale=1.5), grids 0 / 1, windows -1 / 0 / 1 and agent
states uniform in +-2 give |Q| up to 8.33 on these cases, so the relative part of the bound is live; the float32 NumPy restatement of
the same rows uses 0.099 of the bound (tests/test_critic_checkers_oracle.py checks <= 0.5 on the CPU and prints the share)."""
import numpy as np
import pytest
import torch

from tests import critic_checkers_feeds as CF
from tests import critic_checkers_ref as CR
from tests.test_critic_checkers_oracle import CASES as FIXTURES
from tests.test_critic_checkers_oracle import load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGENTS = list(CF.AGENTS)
BATCHES = list(CF.BATCHES)
GAMMA = 0.99
_CACHE = {}


def _critics(N):
    """(global critic, credit critic or None) on the weights of CF.weights(N): once per agent count; tests that change weights build
    their own"""
    if N not in _CACHE:
        from cm3_amd.critic import CheckersCritic
        wg, wc = CF.weights(N)
        g = CheckersCritic(wg, N, kind="global", stage=1 if N == 1 else 2, device=DEV)
        _CACHE[N] = (g, CheckersCritic(wc, N, kind="credit", device=DEV) if N > 1 else None)
    return _CACHE[N]


def _dev(N, B):
    key = ("dev", N, B)
    if key not in _CACHE:
        cols, acts, _ = CF.case(N, B)
        _CACHE[key] = ({k: v.to(DEV) for k, v in cols.items()}, acts.to(DEV))
    return _CACHE[key]


def _args(dc, nxt=False, acts=None):
    """the positional arguments of q_rows / q_pairs (with acts) or q_counterfactual (without) from a batch's columns"""
    p = "next_" if nxt else ""
    head = (dc[p + "grid"], dc[p + "vec"], dc["goals"])
    return head + ((acts,) if acts is not None else ()) + (dc[p + "obs_self_t"], dc[p + "obs_self_v"])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ---- against float64 on the composition's feeds ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", AGENTS)
def test_launches_match_float64_on_the_tiled_feeds(N, B):
    from cm3_amd import _lib
    g, c = _critics(N)
    dc, acts = _dev(N, B)
    ref = CF.refs(N, B)
    out = g.q_rows(*_args(dc, True, acts))
    torch.cuda.synchronize()
    v = _lib.last_kernel_variant()
    assert v.startswith("k_critic_checkers_rows<f32,N=%d," % N) and v.endswith(",kind=global,form=rows>"), v
    assert out["q"].dtype == torch.float32 and tuple(out["q"].shape) == (B * N, 1) and "td" not in out
    CF.within(out["q"].cpu().numpy(), ref["Q_global_target"], what="q_rows N=%d B=%d" % (N, B))
    if N == 1:
        cf = g.q_counterfactual(*_args(dc))
        torch.cuda.synchronize()
        assert _lib.last_kernel_variant().endswith(",kind=global,form=cf>")
        assert cf.dtype == torch.float32 and tuple(cf.shape) == (B, 5)
        CF.within(cf.cpu().numpy(), ref["Q_global"], what="q_counterfactual N=1 B=%d" % B)
        return
    out = c.q_pairs(*_args(dc, True, acts))
    torch.cuda.synchronize()
    assert _lib.last_kernel_variant().endswith(",kind=credit,form=pairs>")
    assert tuple(out["q"].shape) == (B * N * N, 1)
    CF.within(out["q"].cpu().numpy(), ref["Q_credit_target"], what="q_pairs N=%d B=%d" % (N, B))
    cf = c.q_counterfactual(*_args(dc))
    torch.cuda.synchronize()
    v = _lib.last_kernel_variant()
    assert v.startswith("k_critic_checkers_rows<f32,N=%d," % N) and v.endswith(",kind=credit,form=cf>"), v
    assert tuple(cf.shape) == (B * N * N, 5)
    CF.within(cf.cpu().numpy(), ref["Q_credit"], what="q_counterfactual N=%d B=%d" % (N, B))


def test_the_pair_forms_take_window_and_obs_self_v_from_agent_m():
    """Changing agent 1's window changes exactly the pair rows with m = 1 (and agent 1's obs_self_v likewise)."""
    N, B = 3, 3
    _, c = _critics(N)
    dc, acts = _dev(N, B)
    base = c.q_pairs(*_args(dc, True, acts))["q"].reshape(B, N, N)
    for name in ("next_obs_self_t", "next_obs_self_v"):
        other = dict(dc)
        other[name] = dc[name].clone()
        other[name][:, 1] = -other[name][:, 1] + 0.5
        q = c.q_pairs(*_args(other, True, acts))["q"].reshape(B, N, N)
        changed = _bits(q) != _bits(base)
        assert bool(changed[:, 1, :].all()) and not bool(changed[:, 0, :].any()) and not bool(changed[:, 2, :].any()), name


# ---- the fixtures' rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", FIXTURES)
def test_fixture_rows(kind, n):
    from cm3_amd.critic import CheckersCritic
    w, x, q = load_case(kind, n)
    critic = CheckersCritic(w, n, kind=kind, stage=1 if n == 1 else 2, device=DEV)
    cols, pick = CR.fixture_base_columns(kind, n, x)
    t = {k: torch.as_tensor(v) for k, v in cols.items()}                                     # (host columns are staged)
    out = (critic.q_rows if kind == "global" else critic.q_pairs)(t["grid"], t["vec"], t["goals"], t["actions"], t["obs_self_t"],
                                                                  t["obs_self_v"])
    torch.cuda.synchronize()
    CF.within(out["q"].cpu().numpy().reshape(-1)[pick], q, what="fixture %s N=%d" % (kind, n))


# ---- bits -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B", [(1, 13), (2, 3), (3, 13), (8, 1)])
def test_narrow_and_wide_inputs_give_equal_bits(N, B):
    """int8 and float64 grids and windows, index (uint8, int64) and one-hot goals, merged leading dimensions"""
    g, c = _critics(N)
    dc, acts = _dev(N, B)
    narrow = dict(dc)
    for name in ("grid", "next_grid", "obs_self_t", "next_obs_self_t"):
        narrow[name] = dc[name].to(torch.int8)
    narrow["goals"] = dc["goals"].argmax(dim=2).to(torch.uint8)
    index64 = dict(dc, goals=dc["goals"].argmax(dim=2))
    flat = dict(dc, next_obs_self_t=dc["next_obs_self_t"].reshape(B * N, 75), next_vec=dc["next_vec"].reshape(B * N, 4),
                obs_self_t=dc["obs_self_t"].reshape(B * N, 75))
    for other in (narrow, index64, flat):
        assert torch.equal(_bits(g.q_rows(*_args(other, True, acts))["q"]), _bits(g.q_rows(*_args(dc, True, acts))["q"]))
        top = g if N == 1 else c
        assert torch.equal(_bits(top.q_counterfactual(*_args(other))), _bits(top.q_counterfactual(*_args(dc))))
        if N > 1:
            assert torch.equal(_bits(c.q_pairs(*_args(other, True, acts))["q"]), _bits(c.q_pairs(*_args(dc, True, acts))["q"]))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", [2, 3, 8])
def test_pairs_row_is_the_counterfactual_row_at_the_action_taken(N, B):
    _, c = _critics(N)
    dc, acts = _dev(N, B)
    pairs = c.q_pairs(*_args(dc, False, acts))["q"].reshape(-1)
    cf = c.q_counterfactual(*_args(dc))
    a_m = acts.reshape(B, N, 1).expand(B, N, N).reshape(-1)                        # row (b, m, n) -> actions[b, m]
    assert torch.equal(_bits(pairs), _bits(cf.gather(1, a_m.reshape(-1, 1)).reshape(-1)))
    assert float(cf.std(dim=1).median()) > 0                                       # (the action matters)


@pytest.mark.parametrize("N", AGENTS)
def test_a_time_step_alone_equals_it_in_a_batch_of_13(N):
    g, c = _critics(N)
    B = 13
    dc, acts = _dev(N, B)
    a = acts.reshape(B, N)
    for b in (0, 7, 12):
        one = {k: v[b:b + 1] for k, v in dc.items()}
        assert torch.equal(_bits(g.q_rows(*_args(one, True, a[b:b + 1]))["q"]), _bits(g.q_rows(*_args(dc, True, a))["q"][b * N:(b + 1) * N]))
        top, per = (g, 1) if N == 1 else (c, N * N)
        assert torch.equal(_bits(top.q_counterfactual(*_args(one))), _bits(top.q_counterfactual(*_args(dc))[b * per:(b + 1) * per]))
        if N > 1:
            assert torch.equal(_bits(c.q_pairs(*_args(one, True, a[b:b + 1]))["q"]),
                               _bits(c.q_pairs(*_args(dc, True, a))["q"][b * per:(b + 1) * per]))


@pytest.mark.parametrize("reward_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B", [3, 13])
@pytest.mark.parametrize("N", AGENTS)
def test_q64_and_td_are_the_bits_of_td_target(N, B, reward_dtype):
    from cm3_amd import batch as BR
    g, c = _critics(N)
    dc, acts = _dev(N, B)
    reward = CF.make_cols(B, N, 99 + N, reward_dtype=reward_dtype)["local_rewards"].to(DEV)
    done = dc["done"]
    assert 0 < int(done.sum()) < B or B < 4
    out = g.q_rows(*_args(dc, True, acts), reward, done, GAMMA)
    assert torch.equal(out["q64"], out["q"].double()) and out["q64"].dtype == torch.float64
    not_done = -(BR.rep_rows(done, N).to(torch.int64) - 1)
    want = BR.td_target(reward.reshape(-1), out["q64"], not_done, GAMMA)
    assert out["td"].dtype == torch.float64 and torch.equal(_bits(out["td"]), _bits(want))
    assert torch.equal(want, reward.reshape(-1).double() + GAMMA * out["q64"].reshape(-1) * not_done)      # (and the torch composition)
    if N > 1:
        out = c.q_pairs(*_args(dc, True, acts), reward, done, GAMMA)
        assert torch.equal(out["q64"], out["q"].double())
        r_rep = BR.repeat_indexed_by_n(reward.reshape(-1, 1), N).reshape(-1).contiguous()
        nd_rep = -(BR.repeat_indexed_by_n(BR.rep_rows(done, N).reshape(-1, 1).to(torch.int64), N).reshape(-1) - 1).contiguous()
        assert torch.equal(_bits(out["td"]), _bits(BR.td_target(r_rep, out["q64"], nd_rep, GAMMA)))


@pytest.mark.parametrize("N,B", [(3, 3), (1, 13), (8, 1)])
def test_rows_past_the_count_are_untouched_and_single_outputs_agree(N, B):
    from cm3_amd import _lib
    g, c = _critics(N)
    dc, acts = _dev(N, B)
    cols = (dc["next_grid"].contiguous(), dc["next_vec"].contiguous(), dc["goals"].contiguous(), dc["next_obs_self_t"].contiguous(),
            dc["next_obs_self_v"].contiguous())
    ac, rw, dn = acts.to(torch.int32), dc["local_rewards"].contiguous(), dc["done"].view(torch.uint8)
    launches = [(g, _lib.CRITIC_ROWS, B * N, True)]
    launches += [(g, _lib.CRITIC_CF, B * 5, False)] if N == 1 else [(c, _lib.CRITIC_PAIRS, B * N * N, True), (c, _lib.CRITIC_CF, B * N * N * 5, False)]
    for critic, form, R, has_td in launches:
        pad = 200                                                                 # more than a workgroup's rows of canaries
        q = torch.full((R + pad,), -7.5, dtype=torch.float32, device=DEV)
        q64 = torch.full((R + pad,), -7.5, dtype=torch.float64, device=DEV)
        td = torch.full((R + pad,), -7.5, dtype=torch.float64, device=DEV) if has_td else None
        critic.enqueue(form, B, *cols, ac, rw if has_td else None, dn if has_td else None, GAMMA, q=q, q64=q64, td=td)
        torch.cuda.synchronize()
        for t in (q, q64) + ((td,) if has_td else ()):
            assert bool((t[R:] == -7.5).all()) and not bool((t[:R] == -7.5).any()), (form, t.dtype)
        alone = torch.full((R + pad,), -7.5, dtype=torch.float32, device=DEV)
        critic.enqueue(form, B, *cols, ac, q=alone)
        assert torch.equal(_bits(alone), _bits(q))
        alone = torch.full((R + pad,), -7.5, dtype=torch.float64, device=DEV)
        critic.enqueue(form, B, *cols, ac, q64=alone)
        assert torch.equal(_bits(alone), _bits(q64))
        if has_td:
            alone = torch.full((R + pad,), -7.5, dtype=torch.float64, device=DEV)
            critic.enqueue(form, B, *cols, ac, rw, dn, GAMMA, td=alone)
            assert torch.equal(_bits(alone), _bits(td))


# ---- weights --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N", [("global", 1), ("global", 3), ("credit", 3), ("credit", 2)])
def test_repack_and_soft_update_follow_the_weights(kind, N):
    from cm3_amd.critic import CK_NAMES, CheckersCritic
    stage = 1 if N == 1 else 2
    w_a = CR.init_weights(np.random.default_rng(1), N, kind, scale=CF.WEIGHT_SCALE)
    w_b = CR.init_weights(np.random.default_rng(2), N, kind, scale=CF.WEIGHT_SCALE)
    target, main = CheckersCritic(w_a, N, kind=kind, stage=stage, device=DEV), CheckersCritic(w_b, N, kind=kind, stage=stage, device=DEV)
    dc, acts = _dev(N, 3)
    feed = CF.case(N, 3)[2]["Q_global_target" if kind == "global" else "Q_credit_target"]
    launch = lambda c: (c.q_rows if kind == "global" else c.q_pairs)(*_args(dc, True, acts))["q"]      # noqa: E731
    before = launch(target)
    CF.within(before.cpu().numpy(), CF.ref_on_feed(w_a, feed, kind, N, np.float64), what="before")
    # in place, as a session that trains the network writes its variables; the launch follows only after repack()
    for short, t in target.w.items():
        t.copy_(torch.as_tensor(w_b[CK_NAMES[short]]))
    assert torch.equal(_bits(launch(target)), _bits(before))
    target.repack()
    assert torch.equal(_bits(launch(target)), _bits(launch(main)))
    # soft update: float32 arithmetic on the TF-shaped tensors, then one pack launch
    tau = 0.01
    for short, t in target.w.items():
        t.copy_(torch.as_tensor(w_a[CK_NAMES[short]]))
    want = {s: tau * main.w[s] + (1.0 - tau) * target.w[s] for s in target.w}
    target.soft_update_from(main, tau)
    for s in want:
        assert want[s].dtype == torch.float32 and torch.equal(_bits(target.w[s]), _bits(want[s])), s
    mixed = {CK_NAMES[s]: v.cpu().numpy() for s, v in want.items()}
    CF.within(launch(target).cpu().numpy(), CF.ref_on_feed(mixed, feed, kind, N, np.float64), what="after the soft update")
    other = CheckersCritic(CR.init_weights(np.random.default_rng(3), 4, "credit"), 4, kind="credit", device=DEV)
    with pytest.raises(Exception, match="soft_update_from"):
        target.soft_update_from(other, tau)
