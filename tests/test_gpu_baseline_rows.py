"""GPU: the IAC / COMA baseline critics over transition rows (cm3_value_particle_rows_f32, cm3_coma_particle_rows_f32;
cm3_amd.baseline.ParticleValue / ParticleComaCritic) -- v_rows and q_rows against tests/baseline_ref.py in float64 evaluated on the
TILED feeds of the torch composition (so the kernels' row decoding is checked independently of it), the fixture recorded from the
reference's own function bodies, the bit identities between launches and outputs, and the weight updates.

Bound: the project's 2e-5 * max(1, |ref|) per element.  Weights from init_*_weights(scale=1.5) and states uniform in +-2.  Measured
on the CPU with these inputs (N = 1, 2, 3, 4, 8, 10; B = 1, 3, 13, 64): the value networks' mean |V| is 0.5 .. 4.0 (local) and
0.65 .. 1.6 (global), and a float32 NumPy evaluation stays at or below 0.13 of the bound -- 0.121 in BLAS order, 0.124 as a sequential
k-ordered chain (local), 0.092 / 0.108 (global); the COMA critic's mean |Q| is 1.8 .. 2.4 at 0.07 of the bound."""
import numpy as np
import pytest
import torch

from tests import baseline_feeds as BF
from tests import baseline_ref as BR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGENTS = [1, 2, 3, 4, 8, 10]
COMA_AGENTS = [2, 3, 4, 8, 10]
BATCHES = [1, 3, 13]
KINDS = ["local", "global"]
GAMMA = 0.99
CANARY, PAD = -7.5, 200                                     # more than a workgroup's rows of canaries
_CACHE = {}


def _value(N, kind):
    """(network, its weights): once per agent count and kind; tests that change weights build their own"""
    key = ("value", N, kind)
    if key not in _CACHE:
        from cm3_amd.baseline import ParticleValue
        w = BR.init_value_weights(np.random.default_rng(600 + N), N, kind, scale=1.5, scope="V_target")
        _CACHE[key] = (ParticleValue(w, N, kind=kind, stage=1 if N == 1 else 2, device=DEV), w)
    return _CACHE[key]


def _coma(N):
    key = ("coma", N)
    if key not in _CACHE:
        from cm3_amd.baseline import ParticleComaCritic
        w = BR.init_coma_weights(np.random.default_rng(700 + N), N, scale=1.5, scope="Q_target")
        _CACHE[key] = (ParticleComaCritic(w, N, device=DEV), w)
    return _CACHE[key]


def _case(N, B):
    """(host columns, device columns, target actions, {IAC: the composition's tiled feeds}): once per shape, left unchanged"""
    key = ("case", N, B)
    if key not in _CACHE:
        cols = BF.make_cols(B, N, 7000 + 31 * N + B)
        cols["done"] = torch.arange(B) % 3 == 1              # both values from two time steps on, whatever the seed
        acts = torch.as_tensor(np.random.default_rng(N * 100 + B).integers(0, 5, B * N))
        _CACHE[key] = (cols, {k: v.to(DEV) for k, v in cols.items()}, acts,
                       {iac: BF.tiled_feeds(cols, acts, iac) for iac in (True, False)})
    return _CACHE[key]


def _value_args(dc, kind, nxt=True):
    s = "_next" if nxt else ""
    return (dc["obs_others" + s], dc["v_local" + s], dc["goals"]) if kind == "local" else (dc["v_global" + s], dc["goals"])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ---- against float64 on the composition's feeds ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", AGENTS)
@pytest.mark.parametrize("kind", KINDS)
def test_value_launches_match_float64_on_the_tiled_feeds(kind, N, B):
    from cm3_amd import _lib
    net, w = _value(N, kind)
    _, dc, _, feeds = _case(N, B)
    out = net.v_rows(*_value_args(dc, kind))
    torch.cuda.synchronize()
    v = _lib.last_kernel_variant()
    assert v.startswith("k_value_particle_rows<f32,N=%d," % N) and v.endswith(",kind=%s>" % kind), v
    assert out["v"].dtype == torch.float32 and tuple(out["v"].shape) == (B * N, 1) and "td" not in out
    BF.within(out["v"].cpu().numpy(), BF.value_ref_on_feed(w, feeds[kind == "local"]["V_target"], kind, N, np.float64),
              what="v_rows %s N=%d B=%d" % (kind, N, B))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", COMA_AGENTS)
def test_coma_launches_match_float64_on_the_tiled_feeds(N, B):
    from cm3_amd import _lib
    critic, w = _coma(N)
    _, dc, acts, feeds = _case(N, B)
    out = critic.q_rows(dc["v_global_next"], dc["goals"], acts.to(DEV), dc["v_local_next"])
    torch.cuda.synchronize()
    assert _lib.last_kernel_variant().startswith("k_coma_particle_rows<f32,N=%d," % N), _lib.last_kernel_variant()
    assert out["q"].dtype == torch.float32 and tuple(out["q"].shape) == (B * N, 5) and "td" not in out
    BF.within(out["q"].cpu().numpy(), BF.coma_ref_on_feed(w, feeds[False]["Q_target"], np.float64), what="q_rows (target) N=%d B=%d" % (N, B))
    out = critic.q_rows(dc["v_global"], dc["goals"], dc["actions"], dc["v_local"])
    BF.within(out["q"].cpu().numpy(), BF.coma_ref_on_feed(w, feeds[False]["Q"], np.float64), what="q_rows (main) N=%d B=%d" % (N, B))


# ---- the fixture's rows ---------------------------------------------------------------------------------------------------------------
def _base_columns(tag, x):
    """Base columns whose decoded rows hold the fixture's inputs: fixture row i is a time step of its own and its row's agent is
    n = i % N; the other agents, ascending, take the "others" inputs.  Returns (columns, the launch's row of each fixture row)."""
    kind, n = tag.split("_n")
    n = int(n)
    R = x["v_goal"].shape[0]
    ni = np.arange(R) % n
    c = {k: np.zeros((R, n, d), np.float32) for k, d in (("state", 4), ("goals", 2), ("v_obs", 4), ("obs_others", 4 * max(n - 1, 1)))}
    c["actions"] = np.zeros((R, n), np.int64)
    for r in range(R):
        me, others = ni[r], [j for j in range(n) if j != ni[r]]
        c["goals"][r, me] = x["v_goal"][r]
        if "v_goal_others" in x and n > 1:
            c["goals"][r, others] = x["v_goal_others"][r].reshape(n - 1, 2)
        if kind == "local":
            c["v_obs"][r, me] = x["v_obs"][r]
            if n > 1:
                c["obs_others"][r, me] = x["obs_others"][r]
        elif kind == "global":
            c["state"][r, me] = x["v_state_one_agent"][r]
            if n > 1:
                c["state"][r, others] = x["v_state_other_agents"][r].reshape(n - 1, 4)
        else:
            assert np.array_equal(x["v_labels"][r], np.eye(n, dtype=np.float32)[me])
            c["state"][r] = x["v_state"][r].reshape(n, 4)
            c["v_obs"][r, me] = x["v_obs"][r]
            c["actions"][r, others] = x["action_others"][r].reshape(n - 1, 5).argmax(1)
    return {k: torch.as_tensor(v) for k, v in c.items()}, np.arange(R) * n + ni


@pytest.mark.parametrize("tag", BR.VALUE_CASES + BR.COMA_CASES)
def test_fixture_rows(tag):
    import os
    from cm3_amd.baseline import ParticleComaCritic, ParticleValue
    w, x, want = BR.load_case(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), tag)
    kind, n = tag.split("_n")[0], int(tag.split("_n")[1])
    c, pick = _base_columns(tag, x)
    if kind == "coma":
        got = ParticleComaCritic(w, n, device=DEV).q_rows(c["state"], c["goals"], c["actions"], c["v_obs"])["q"]      # (host columns are staged)
    else:
        net = ParticleValue(w, n, kind=kind, stage=1 if n == 1 else 2, device=DEV)
        got = net.v_rows(c["obs_others"], c["v_obs"], c["goals"])["v"] if kind == "local" else net.v_rows(c["state"], c["goals"])["v"]
    torch.cuda.synchronize()
    BF.within(got.cpu().numpy()[pick], want, what="fixture %s" % tag)


# ---- bits -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", AGENTS)
def test_whole_batch_equals_its_halves(N):
    B, h = 13, 6
    _, dc, acts, _ = _case(N, B)
    for kind in KINDS:
        net, _ = _value(N, kind)
        args = _value_args(dc, kind)
        whole = net.v_rows(*args)["v"]
        parts = [net.v_rows(*(a[:h] for a in args))["v"], net.v_rows(*(a[h:] for a in args))["v"]]
        assert torch.equal(_bits(whole), _bits(torch.cat(parts))), kind
    if N > 1:
        critic, _ = _coma(N)
        a = acts.reshape(B, N).to(DEV)
        args = (dc["v_global_next"], dc["goals"], a, dc["v_local_next"])
        whole = critic.q_rows(*args)
        parts = [critic.q_rows(*(t[:h] for t in args)), critic.q_rows(*(t[h:] for t in args))]
        for name in ("q", "q_taken"):
            assert torch.equal(_bits(whole[name]), _bits(torch.cat([p[name] for p in parts]))), name


@pytest.mark.parametrize("reward_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B", [3, 13])
@pytest.mark.parametrize("N", AGENTS)
def test_widened_outputs_and_td_are_the_bits_of_td_target(N, B, reward_dtype):
    from cm3_amd import batch as BT
    _, dc, acts, _ = _case(N, B)
    done = dc["done"]
    assert 0 < int(done.sum()) < B                                                # the done column holds both values
    not_done = -(BT.rep_rows(done, N).to(torch.int64) - 1)
    reward_local = BF.make_cols(B, N, 99 + N, reward_dtype=reward_dtype)["reward_local"].to(DEV)
    for kind in KINDS:
        net, _ = _value(N, kind)
        out = net.v_rows(*_value_args(dc, kind), reward_local, done, GAMMA)
        assert out["v64"].dtype == torch.float64 and torch.equal(out["v64"], out["v"].double())
        want = BT.td_target(reward_local.reshape(-1), out["v64"], not_done, GAMMA)
        assert out["td"].dtype == torch.float64 and torch.equal(_bits(out["td"]), _bits(want)), kind
        assert torch.equal(want, reward_local.reshape(-1).double() + GAMMA * out["v64"].reshape(-1) * not_done)      # (the torch composition)
    if N > 1:
        critic, _ = _coma(N)
        reward = dc["reward"].to(reward_dtype)                                    # the GLOBAL reward [B]
        a = acts.to(DEV)
        out = critic.q_rows(dc["v_global_next"], dc["goals"], a, dc["v_local_next"], reward, done, GAMMA)
        assert out["q_taken64"].dtype == torch.float64 and torch.equal(out["q_taken64"], out["q_taken"].double())
        assert torch.equal(_bits(out["q_taken"]), _bits(out["q"].gather(1, a.reshape(-1, 1))))
        want = BT.td_target(BT.rep_rows(reward, N).contiguous(), out["q_taken64"], not_done, GAMMA)
        assert out["td"].dtype == torch.float64 and torch.equal(_bits(out["td"]), _bits(want))


@pytest.mark.parametrize("B", [3, 13])
@pytest.mark.parametrize("N", COMA_AGENTS)
def test_q_taken_is_the_own_action_and_the_others_actions_matter(N, B):
    critic, _ = _coma(N)
    _, dc, acts, _ = _case(N, B)
    a = acts.reshape(B, N).to(DEV)
    args = lambda a: (dc["v_global_next"], dc["goals"], a, dc["v_local_next"])      # noqa: E731
    out = critic.q_rows(*args(a))
    assert torch.equal(_bits(out["q_taken"]), _bits(out["q"].gather(1, a.reshape(-1, 1))))
    assert len(set(a.reshape(-1).tolist())) > 1 or B * N < 3
    # agent 0 of step 0 takes another action: its own row keeps its q (the input holds the OTHERS' actions) and moves only along
    # its row of q for q_taken; the rows of the other agents of that step change; every other step keeps its bits
    a2 = a.clone()
    a2[0, 0] = (a2[0, 0] + 1) % 5
    out2 = critic.q_rows(*args(a2))
    assert torch.equal(_bits(out2["q"][0]), _bits(out["q"][0]))
    assert torch.equal(_bits(out2["q_taken"][0]), _bits(out["q"][0, a2[0, 0]].reshape(1)))
    assert bool((out2["q"][1:N] != out["q"][1:N]).any(dim=1).all())
    assert torch.equal(_bits(out2["q"][N:]), _bits(out["q"][N:]))


@pytest.mark.parametrize("N,B", [(4, 3), (1, 13), (10, 1), (1, 1)])
def test_rows_past_the_count_are_untouched_and_single_outputs_agree(N, B):
    _, dc, acts, _ = _case(N, B)
    R = B * N
    full = lambda dt: torch.full((R + PAD,), CANARY, dtype=dt, device=DEV)      # noqa: E731
    go, dn = dc["goals"].contiguous(), dc["done"].view(torch.uint8)
    rw = dc["reward_local"].contiguous()
    for kind in KINDS:
        net, _ = _value(N, kind)
        st = (dc["v_local_next"] if kind == "local" else dc["v_global_next"]).contiguous()
        oo = dc["obs_others_next"].contiguous() if kind == "local" else None
        v, v64, td = full(torch.float32), full(torch.float64), full(torch.float64)
        net.enqueue(B, st, go, oo, rw, dn, GAMMA, v=v, v64=v64, td=td)
        torch.cuda.synchronize()
        for t in (v, v64, td):
            assert bool((t[R:] == CANARY).all()) and not bool((t[:R] == CANARY).any()), (kind, t.dtype)
        alone = full(torch.float32)
        net.enqueue(B, st, go, oo, v=alone)
        assert torch.equal(_bits(alone), _bits(v))
        alone = full(torch.float64)
        net.enqueue(B, st, go, oo, v64=alone)
        assert torch.equal(_bits(alone), _bits(v64))
        alone = full(torch.float64)
        net.enqueue(B, st, go, oo, rw, dn, GAMMA, td=alone)
        assert torch.equal(_bits(alone), _bits(td))
    if N == 1:
        return
    critic, _ = _coma(N)
    st, vo, ac = dc["v_global_next"].contiguous(), dc["v_local_next"].contiguous(), acts.to(DEV).to(torch.int32)
    rg = dc["reward"].contiguous()
    q = torch.full((R + PAD, 5), CANARY, dtype=torch.float32, device=DEV)
    qt, qt64, td = full(torch.float32), full(torch.float64), full(torch.float64)
    critic.enqueue(B, st, go, vo, ac, ac, rg, dn, GAMMA, q=q, q_taken=qt, q_taken64=qt64, td=td)
    torch.cuda.synchronize()
    for t in (q, qt, qt64, td):
        assert bool((t[R:] == CANARY).all()) and not bool((t[:R] == CANARY).any()), t.dtype
    alone = torch.full((R + PAD, 5), CANARY, dtype=torch.float32, device=DEV)
    critic.enqueue(B, st, go, vo, ac, q=alone)                                    # (q alone needs no own action)
    assert torch.equal(_bits(alone), _bits(q))
    for name, ref, dt in (("q_taken", qt, torch.float32), ("q_taken64", qt64, torch.float64)):
        alone = full(dt)
        critic.enqueue(B, st, go, vo, ac, ac, **{name: alone})
        assert torch.equal(_bits(alone), _bits(ref)), name
    alone = full(torch.float64)
    critic.enqueue(B, st, go, vo, ac, ac, rg, dn, GAMMA, td=alone)
    assert torch.equal(_bits(alone), _bits(td))


# ---- weights --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,N", [("local", 1), ("local", 4), ("global", 4), ("global", 3), ("coma", 4), ("coma", 3)])
def test_repack_and_soft_update_follow_the_weights(net, N):
    from cm3_amd.baseline import COMA_NAMES, VALUE_NAMES, ParticleComaCritic, ParticleValue
    _, dc, acts, feeds = _case(N, 3)
    if net == "coma":
        names = COMA_NAMES
        init = lambda seed: BR.init_coma_weights(np.random.default_rng(seed), N, scale=1.5)      # noqa: E731
        make = lambda w: ParticleComaCritic(w, N, device=DEV)      # noqa: E731
        launch = lambda c: c.q_rows(dc["v_global_next"], dc["goals"], acts.to(DEV), dc["v_local_next"])["q"]      # noqa: E731
        ref = lambda w: BF.coma_ref_on_feed(w, feeds[False]["Q_target"], np.float64)      # noqa: E731
    else:
        names = VALUE_NAMES[net]
        init = lambda seed: BR.init_value_weights(np.random.default_rng(seed), N, net, scale=1.5)      # noqa: E731
        make = lambda w: ParticleValue(w, N, kind=net, stage=1 if N == 1 else 2, device=DEV)      # noqa: E731
        launch = lambda c: c.v_rows(*_value_args(dc, net))["v"]      # noqa: E731
        ref = lambda w: BF.value_ref_on_feed(w, feeds[net == "local"]["V_target"], net, N, np.float64)      # noqa: E731
    w_a, w_b = init(1), init(2)
    target, main = make(w_a), make(w_b)
    before = launch(target)
    BF.within(before.cpu().numpy(), ref(w_a), what="before")
    # in place, as a session that trains the network writes its variables; the launch follows only after repack()
    for short, t in target.w.items():
        t.copy_(torch.as_tensor(w_b[names[short]]))
    assert torch.equal(_bits(launch(target)), _bits(before))
    target.repack()
    assert torch.equal(_bits(launch(target)), _bits(launch(main)))
    # soft update: float32 arithmetic on the TF-shaped tensors, then one pack launch
    tau = 0.01
    for short, t in target.w.items():
        t.copy_(torch.as_tensor(w_a[names[short]]))
    want = {s: tau * main.w[s] + (1.0 - tau) * target.w[s] for s in target.w}
    target.soft_update_from(main, tau)
    for s in want:
        assert want[s].dtype == torch.float32 and torch.equal(_bits(target.w[s]), _bits(want[s])), s
    mixed = {names[s]: v.cpu().numpy() for s, v in want.items()}
    BF.within(launch(target).cpu().numpy(), ref(mixed), what="after the soft update")
    other = ParticleComaCritic(BR.init_coma_weights(np.random.default_rng(3), 2), 2, device=DEV) if net == "coma" else \
        ParticleValue(BR.init_value_weights(np.random.default_rng(3), 2, net), 2, kind=net, device=DEV)
    with pytest.raises(Exception, match="soft_update_from"):
        target.soft_update_from(other, tau)
