"""GPU: the CM3 particle critics over transition rows (cm3_critic_particle_rows_f32; cm3_amd.critic.ParticleCritic) -- q_rows,
q_pairs and q_counterfactual against tests/critic_ref.py in float64 evaluated on the TILED feeds of the torch composition (so the
kernel's row decoding is checked independently of it), the fixture recorded from the reference's own function bodies, the bit
identities between the forms and outputs, and the weight updates.

Bound: the project's 2e-5 * max(1, |ref|) per row.  Weights from init_weights(scale=1.5) and states uniform in +-2 give |Q| of
3 .. 9, so the relative part of the bound is live; the float32 NumPy evaluation of the same rows uses at most 0.11 of it."""
import numpy as np
import pytest
import torch

from tests import critic_feeds as CF
from tests import critic_ref as CR
from tests.test_critic_oracle import load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGENTS = [1, 2, 3, 4, 8, 10]
BATCHES = [1, 3, 13]
GAMMA = 0.99
_CACHE = {}


def _critics(N):
    """(global critic, its weights, credit critic or None, its weights): once per agent count; tests that change weights build their own"""
    if N not in _CACHE:
        from cm3_amd.critic import ParticleCritic
        rng = np.random.default_rng(500 + N)
        wg = CR.init_weights(rng, N, "global", scale=1.5, scope="Q_global_target")
        g = ParticleCritic(wg, N, kind="global", stage=1 if N == 1 else 2, device=DEV)
        wc = c = None
        if N > 1:
            wc = CR.init_weights(rng, N, "credit", scale=1.5, scope="Q_credit_main")
            c = ParticleCritic(wc, N, kind="credit", device=DEV)
        _CACHE[N] = (g, wg, c, wc)
    return _CACHE[N]


def _case(N, B):
    """(host columns, device columns, target actions, the composition's tiled feeds): once per shape, left unchanged"""
    key = ("case", N, B)
    if key not in _CACHE:
        cols = CF.make_cols(B, N, 7000 + 31 * N + B)
        acts = torch.as_tensor(np.random.default_rng(N * 100 + B).integers(0, 5, B * N))
        _CACHE[key] = (cols, {k: v.to(DEV) for k, v in cols.items()}, acts, CF.tiled_feeds(cols, acts))
    return _CACHE[key]


# ---- 3. against float64 on the composition's feeds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", AGENTS)
def test_launches_match_float64_on_the_tiled_feeds(N, B):
    from cm3_amd import _lib
    g, wg, c, wc = _critics(N)
    _, dc, acts, feeds = _case(N, B)
    out = g.q_rows(dc["v_global_next"], dc["goals"], acts.to(DEV))
    torch.cuda.synchronize()
    v = _lib.last_kernel_variant()
    assert v.startswith("k_critic_particle_rows<f32,N=%d," % N) and v.endswith(",kind=global,form=rows>"), v
    assert out["q"].dtype == torch.float32 and tuple(out["q"].shape) == (B * N, 1) and "td" not in out
    CF.within(out["q"].cpu().numpy(), CF.ref_on_feed(wg, feeds["Q_global_target"], "global", N, np.float64), what="q_rows N=%d B=%d" % (N, B))
    if N == 1:
        cf = g.q_counterfactual(dc["v_global"], dc["goals"])
        torch.cuda.synchronize()
        assert _lib.last_kernel_variant().endswith(",kind=global,form=cf>")
        assert cf.dtype == torch.float32 and tuple(cf.shape) == (B, 5)
        CF.within(cf.cpu().numpy(), CF.ref_on_feed(wg, feeds["Q_global"], "global", 1, np.float64), what="q_counterfactual N=1 B=%d" % B)
        return
    out = c.q_pairs(dc["v_global_next"], dc["goals"], acts.to(DEV))
    torch.cuda.synchronize()
    assert _lib.last_kernel_variant().endswith(",kind=credit,form=pairs>")
    assert tuple(out["q"].shape) == (B * N * N, 1)
    CF.within(out["q"].cpu().numpy(), CF.ref_on_feed(wc, feeds["Q_credit_target"], "credit", N, np.float64), what="q_pairs N=%d B=%d" % (N, B))
    cf = c.q_counterfactual(dc["v_global"], dc["goals"])
    torch.cuda.synchronize()
    assert _lib.last_kernel_variant().endswith(",kind=credit,form=cf>")
    assert tuple(cf.shape) == (B * N * N, 5)
    CF.within(cf.cpu().numpy(), CF.ref_on_feed(wc, feeds["Q_credit"], "credit", N, np.float64), what="q_counterfactual N=%d B=%d" % (N, B))


# ---- 4. the fixture's rows ----------------------------------------------------------------------------------------------------------
def _base_columns(x, kind, n):
    """Base columns whose decoded rows hold the fixture's inputs: fixture row i is a time step of its own, its row's agent
    n = i % N (the others, ascending, take s_others / a_others); credit rows are the pair with m = (i // N) % N."""
    R = x["s_n"].shape[0]
    i = np.arange(R)
    ni, mi = i % n, (i // n) % n
    state, goals = np.zeros((R, n, 4), np.float32), np.zeros((R, n, 2), np.float32)
    actions = np.zeros((R, n), np.int64)
    for r in range(R):
        others = [j for j in range(n) if j != ni[r]]
        state[r, ni[r]], goals[r, ni[r]] = x["s_n"][r], x["g_n"][r]
        state[r, others] = x["s_others"][r].reshape(n - 1, 4)
        if kind == "global":
            actions[r, ni[r]] = x["a_n"][r].argmax()
            actions[r, others] = x["a_others"][r].reshape(n - 1, 5).argmax(1)
        else:
            actions[r, mi[r]] = x["a_m"][r].argmax()
            assert np.array_equal(state[r, mi[r]], x["s_m"][r])              # s_m IS agent m's state of the time step
    pick = i * n + ni if kind == "global" else (i * n + mi) * n + ni
    return torch.as_tensor(state), torch.as_tensor(goals), torch.as_tensor(actions), pick


@pytest.mark.parametrize("kind,n", [("global", 1), ("global", 2), ("credit", 2), ("global", 4), ("credit", 4), ("global", 10), ("credit", 10)])
def test_fixture_rows(kind, n):
    from cm3_amd.critic import ParticleCritic
    w, x, q = load_case(kind, n)
    critic = ParticleCritic(w, n, kind=kind, stage=1 if n == 1 else 2, device=DEV)
    state, goals, actions, pick = _base_columns(x, kind, n)
    out = (critic.q_rows if kind == "global" else critic.q_pairs)(state, goals, actions)       # (host columns are staged)
    torch.cuda.synchronize()
    CF.within(out["q"].cpu().numpy().reshape(-1)[pick], q, what="fixture %s N=%d" % (kind, n))


# ---- 5. bits ------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", [2, 3, 4, 8, 10])
def test_pairs_row_is_the_counterfactual_row_at_the_action_taken(N, B):
    _, _, c, _ = _critics(N)
    _, dc, acts, _ = _case(N, B)
    pairs = c.q_pairs(dc["v_global"], dc["goals"], acts.to(DEV))["q"].reshape(-1)
    cf = c.q_counterfactual(dc["v_global"], dc["goals"])
    a_m = acts.reshape(B, N, 1).expand(B, N, N).reshape(-1).to(DEV)                # row (b, m, n) -> actions[b, m]
    assert torch.equal(_bits(pairs), _bits(cf.gather(1, a_m.reshape(-1, 1)).reshape(-1)))
    assert float(cf.std(dim=1).median()) > 0                                       # (the action matters)


@pytest.mark.parametrize("N", AGENTS)
def test_whole_batch_equals_its_halves(N):
    g, _, c, _ = _critics(N)
    B, h = 13, 6
    _, dc, acts, _ = _case(N, B)
    a = acts.reshape(B, N).to(DEV)
    s, go = dc["v_global_next"], dc["goals"]
    whole = g.q_rows(s, go, a)["q"]
    assert torch.equal(_bits(whole), _bits(torch.cat([g.q_rows(s[:h], go[:h], a[:h])["q"], g.q_rows(s[h:], go[h:], a[h:])["q"]])))
    top = g if N == 1 else c
    whole = top.q_counterfactual(s, go)
    assert torch.equal(_bits(whole), _bits(torch.cat([top.q_counterfactual(s[:h], go[:h]), top.q_counterfactual(s[h:], go[h:])])))
    if N > 1:
        whole = c.q_pairs(s, go, a)["q"]
        assert torch.equal(_bits(whole), _bits(torch.cat([c.q_pairs(s[:h], go[:h], a[:h])["q"], c.q_pairs(s[h:], go[h:], a[h:])["q"]])))


@pytest.mark.parametrize("reward_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B", [3, 13])
@pytest.mark.parametrize("N", AGENTS)
def test_q64_and_td_are_the_bits_of_td_target(N, B, reward_dtype):
    from cm3_amd import batch as BR
    g, _, c, _ = _critics(N)
    _, dc, acts, _ = _case(N, B)
    reward = CF.make_cols(B, N, 99 + N, reward_dtype=reward_dtype)["reward_local"].to(DEV)
    done = dc["done"]
    assert 0 < int(done.sum()) < B or B < 4
    out = g.q_rows(dc["v_global_next"], dc["goals"], acts.to(DEV), reward, done, GAMMA)
    assert torch.equal(out["q64"], out["q"].double()) and out["q64"].dtype == torch.float64
    not_done = -(BR.rep_rows(done, N).to(torch.int64) - 1)
    want = BR.td_target(reward.reshape(-1), out["q64"], not_done, GAMMA)
    assert out["td"].dtype == torch.float64 and torch.equal(_bits(out["td"]), _bits(want))
    assert torch.equal(want, reward.reshape(-1).double() + GAMMA * out["q64"].reshape(-1) * not_done)      # (and the torch composition)
    if N > 1:
        out = c.q_pairs(dc["v_global_next"], dc["goals"], acts.to(DEV), reward, done, GAMMA)
        assert torch.equal(out["q64"], out["q"].double())
        r_rep = BR.repeat_indexed_by_n(reward.reshape(-1, 1), N).reshape(-1).contiguous()
        nd_rep = -(BR.repeat_indexed_by_n(BR.rep_rows(done, N).reshape(-1, 1).to(torch.int64), N).reshape(-1) - 1).contiguous()
        assert torch.equal(_bits(out["td"]), _bits(BR.td_target(r_rep, out["q64"], nd_rep, GAMMA)))


@pytest.mark.parametrize("N,B", [(4, 3), (1, 13), (10, 1)])
def test_rows_past_the_count_are_untouched_and_single_outputs_agree(N, B):
    from cm3_amd import _lib
    g, _, c, _ = _critics(N)
    _, dc, acts, _ = _case(N, B)
    st, go = dc["v_global_next"].contiguous(), dc["goals"].contiguous()
    ac, rw, dn = acts.to(DEV).to(torch.int32), dc["reward_local"].contiguous(), dc["done"].view(torch.uint8)
    launches = [(g, _lib.CRITIC_ROWS, B * N, True)]
    launches += [(g, _lib.CRITIC_CF, B * 5, False)] if N == 1 else [(c, _lib.CRITIC_PAIRS, B * N * N, True), (c, _lib.CRITIC_CF, B * N * N * 5, False)]
    for critic, form, R, has_td in launches:
        pad = 200                                                                 # more than a workgroup's rows of canaries
        q = torch.full((R + pad,), -7.5, dtype=torch.float32, device=DEV)
        q64 = torch.full((R + pad,), -7.5, dtype=torch.float64, device=DEV)
        td = torch.full((R + pad,), -7.5, dtype=torch.float64, device=DEV) if has_td else None
        critic.enqueue(form, B, st, go, ac, rw if has_td else None, dn if has_td else None, GAMMA, q=q, q64=q64, td=td)
        torch.cuda.synchronize()
        for t in (q, q64) + ((td,) if has_td else ()):
            assert bool((t[R:] == -7.5).all()) and not bool((t[:R] == -7.5).any()), (form, t.dtype)
        alone = torch.full((R + pad,), -7.5, dtype=torch.float32, device=DEV)
        critic.enqueue(form, B, st, go, ac, q=alone)
        assert torch.equal(_bits(alone), _bits(q))
        alone = torch.full((R + pad,), -7.5, dtype=torch.float64, device=DEV)
        critic.enqueue(form, B, st, go, ac, q64=alone)
        assert torch.equal(_bits(alone), _bits(q64))
        if has_td:
            alone = torch.full((R + pad,), -7.5, dtype=torch.float64, device=DEV)
            critic.enqueue(form, B, st, go, ac, rw, dn, GAMMA, td=alone)
            assert torch.equal(_bits(alone), _bits(td))


# ---- 6. weights ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N", [("global", 1), ("global", 4), ("credit", 4), ("credit", 3)])
def test_repack_and_soft_update_follow_the_weights(kind, N):
    from cm3_amd.critic import NAMES, ParticleCritic
    stage = 1 if N == 1 else 2
    w_a = CR.init_weights(np.random.default_rng(1), N, kind, scale=1.5)
    w_b = CR.init_weights(np.random.default_rng(2), N, kind, scale=1.5)
    target, main = ParticleCritic(w_a, N, kind=kind, stage=stage, device=DEV), ParticleCritic(w_b, N, kind=kind, stage=stage, device=DEV)
    _, dc, acts, feeds = _case(N, 3)
    op = "Q_global_target" if kind == "global" else "Q_credit_target"
    launch = lambda c: (c.q_rows if kind == "global" else c.q_pairs)(dc["v_global_next"], dc["goals"], acts.to(DEV))["q"]      # noqa: E731
    before = launch(target)
    CF.within(before.cpu().numpy(), CF.ref_on_feed(w_a, feeds[op], kind, N, np.float64), what="before")
    # in place, as a session that trains the network writes its variables; the launch follows only after repack()
    for short, t in target.w.items():
        t.copy_(torch.as_tensor(w_b[NAMES[short]]))
    assert torch.equal(_bits(launch(target)), _bits(before))
    target.repack()
    assert torch.equal(_bits(launch(target)), _bits(launch(main)))
    # soft update: float32 arithmetic on the TF-shaped tensors, then one pack launch
    tau = 0.01
    for short, t in target.w.items():
        t.copy_(torch.as_tensor(w_a[NAMES[short]]))
    want = {s: tau * main.w[s] + (1.0 - tau) * target.w[s] for s in target.w}
    target.soft_update_from(main, tau)
    for s in want:
        assert want[s].dtype == torch.float32 and torch.equal(_bits(target.w[s]), _bits(want[s])), s
    mixed = {NAMES[s]: v.cpu().numpy() for s, v in want.items()}
    CF.within(launch(target).cpu().numpy(), CF.ref_on_feed(mixed, feeds[op], kind, N, np.float64), what="after the soft update")
    other = ParticleCritic(CR.init_weights(np.random.default_rng(3), 2, "credit"), 2, kind="credit", device=DEV)
    with pytest.raises(Exception, match="soft_update_from"):
        target.soft_update_from(other, tau)
