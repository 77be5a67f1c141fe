"""GPU: the Checkers IAC / COMA baseline critics over transition rows (cm3_value_checkers_rows_f32, cm3_coma_checkers_rows_f32;
cm3_amd.baseline.CheckersValue / CheckersComaCritic) -- v_rows and q_rows against tests/baseline_checkers_ref.py in float64 evaluated
on the TILED feeds of the torch composition (so the kernels' row decoding is checked independently of it), the fixtures recorded from
the reference's own function bodies, the bit identities between input forms, launches and outputs, and the weight updates.

Bound: the project's 2e-5 * max(1, |ref|) per element.  Weights scale / sqrt(fan_in) at scale 1.5, grids 0 / 1, windows -1 / 0 / 1,
states uniform in +-2.  tests/test_baseline_checkers_oracle.py measures on the CPU what a float32 NumPy evaluation uses of the bound on
these very cases: 0.078 (local), 0.093 (global), 0.093 (COMA), with max |ref| 6.4 .. 7.5."""
import os

import numpy as np
import pytest
import torch

from tests import baseline_checkers_feeds as BF
from tests import baseline_checkers_ref as BR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.99
CANARY, PAD = -7.5, 200                                     # more than a workgroup's rows of canaries
_CACHE = {}


def _value(N, kind):
    """the network of BF.value_weights: once per agent count and kind; tests that change weights build their own"""
    if ("value", N, kind) not in _CACHE:
        from cm3_amd.baseline import CheckersValue
        _CACHE[("value", N, kind)] = CheckersValue(BF.value_weights(N, kind), N, kind=kind, stage=1 if N == 1 else 2, device=DEV)
    return _CACHE[("value", N, kind)]


def _coma(N):
    if ("coma", N) not in _CACHE:
        from cm3_amd.baseline import CheckersComaCritic
        _CACHE[("coma", N)] = CheckersComaCritic(BF.coma_weights(N), N, device=DEV)
    return _CACHE[("coma", N)]


def _dev(N, B):
    """the device copy of BF.case(N, B)'s columns"""
    if ("dev", N, B) not in _CACHE:
        _CACHE[("dev", N, B)] = {k: v.to(DEV) for k, v in BF.case(N, B)[0].items()}
    return _CACHE[("dev", N, B)]


def _value_args(c, kind, nxt=True):
    p = "next_" if nxt else ""
    if kind == "local":
        return (c[p + "obs_self_t"], c[p + "obs_self_v"], c[p + "obs_others"], c["goals"])
    return (c[p + "grid"], c[p + "vec"], c["goals"])


def _coma_args(c, actions, nxt=True):
    p = "next_" if nxt else ""
    return (c[p + "grid"], c[p + "vec"], c["goals"], actions, c[p + "obs_self_t"], c[p + "obs_self_v"])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ---- against float64 on the composition's feeds ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BF.BATCHES)
@pytest.mark.parametrize("N", BF.VALUE_AGENTS)
@pytest.mark.parametrize("kind", BF.KINDS)
def test_value_launches_match_float64_on_the_tiled_feeds(kind, N, B):
    from cm3_amd import _lib
    out = _value(N, kind).v_rows(*_value_args(_dev(N, B), kind))
    torch.cuda.synchronize()
    v = _lib.last_kernel_variant()
    assert v.startswith("k_value_checkers_rows<f32,N=%d," % N) and v.endswith(",kind=%s>" % kind), v
    assert out["v"].dtype == torch.float32 and tuple(out["v"].shape) == (B * N, 1) and "td" not in out
    BF.within(out["v"].cpu().numpy(), BF.refs(N, B)[kind], what="v_rows %s N=%d B=%d" % (kind, N, B))


@pytest.mark.parametrize("B", BF.BATCHES)
@pytest.mark.parametrize("N", BF.COMA_AGENTS)
def test_coma_launches_match_float64_on_the_tiled_feeds(N, B):
    from cm3_amd import _lib
    critic, dc, acts = _coma(N), _dev(N, B), BF.case(N, B)[1]
    out = critic.q_rows(*_coma_args(dc, acts.to(DEV)))
    torch.cuda.synchronize()
    assert _lib.last_kernel_variant().startswith("k_coma_checkers_rows<f32,N=%d," % N), _lib.last_kernel_variant()
    assert out["q"].dtype == torch.float32 and tuple(out["q"].shape) == (B * N, 5) and "td" not in out
    BF.within(out["q"].cpu().numpy(), BF.refs(N, B)["Q_target"], what="q_rows (target) N=%d B=%d" % (N, B))
    out = critic.q_rows(*_coma_args(dc, dc["actions"], nxt=False))
    BF.within(out["q"].cpu().numpy(), BF.refs(N, B)["Q"], what="q_rows (main) N=%d B=%d" % (N, B))


# ---- the fixtures' rows, as decodings of base columns --------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", BR.CASES)
def test_fixture_rows(tag):
    from cm3_amd.baseline import CheckersComaCritic, CheckersValue
    w, x, want = BR.load_case(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), tag)
    kind, n = tag.split("_n")[0], int(tag.split("_n")[1])
    c, pick = BR.fixture_base_columns(tag, x)
    c = {k: torch.as_tensor(v) for k, v in c.items()}      # (host columns are staged)
    if kind == "coma":
        got = CheckersComaCritic(w, n, device=DEV).q_rows(*_coma_args(c, c["actions"], nxt=False))["q"]
    else:
        got = CheckersValue(w, n, kind=kind, stage=1 if n == 1 else 2, device=DEV).v_rows(*_value_args(c, kind, nxt=False))["v"]
    torch.cuda.synchronize()
    BF.within(got.cpu().numpy()[pick], want, what="fixture %s" % tag)


# ---- bits -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", BF.VALUE_AGENTS)
def test_input_forms_give_the_same_bits(N):
    """int8 against float64 grids and windows, uint8 index against int64 one-hot goals (a flat index column of another dtype is
    staged to one-hot): the same values, so the same bits"""
    B = 13
    dc, acts = _dev(N, B), BF.case(N, B)[1].to(DEV)
    narrow = dict(dc)
    for k in ("next_grid", "next_obs_self_t"):
        narrow[k] = dc[k].to(torch.int8)
    idx = dc["goals"].argmax(dim=2)
    for goals in (idx.to(torch.uint8), idx):
        narrow["goals"] = goals
        for kind in BF.KINDS:
            net = _value(N, kind)
            assert torch.equal(_bits(net.v_rows(*_value_args(narrow, kind))["v"]), _bits(net.v_rows(*_value_args(dc, kind))["v"])), kind
        if N > 1:
            assert torch.equal(_bits(_coma(N).q_rows(*_coma_args(narrow, acts))["q"]), _bits(_coma(N).q_rows(*_coma_args(dc, acts))["q"]))


@pytest.mark.parametrize("N", BF.VALUE_AGENTS)
def test_a_row_has_the_same_bits_alone_and_inside_67_time_steps(N):
    """time step 0 (first workgroup) and time step 66 (the partial last tile) as launches of their own against the whole batch"""
    B = 67
    dc, acts = _dev(N, B), BF.case(N, B)[1].reshape(B, N).to(DEV)
    for b in (0, B - 1):
        for kind in BF.KINDS:
            args = _value_args(dc, kind)
            whole, alone = _value(N, kind).v_rows(*args)["v"], _value(N, kind).v_rows(*(a[b:b + 1] for a in args))["v"]
            assert torch.equal(_bits(whole[b * N:(b + 1) * N]), _bits(alone)), (kind, b)
        if N > 1:
            args = _coma_args(dc, acts)
            whole, alone = _coma(N).q_rows(*args), _coma(N).q_rows(*(a[b:b + 1] for a in args))
            for name in ("q", "q_taken"):
                assert torch.equal(_bits(whole[name][b * N:(b + 1) * N]), _bits(alone[name])), (name, b)


@pytest.mark.parametrize("reward_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B", [3, 67])
@pytest.mark.parametrize("N", BF.VALUE_AGENTS)
def test_widened_outputs_and_td_are_the_bits_of_td_target(N, B, reward_dtype):
    from cm3_amd import batch as BT
    dc, acts = _dev(N, B), BF.case(N, B)[1].to(DEV)
    done = dc["done"]
    assert 0 < int(done.sum()) < B                                                # the done column holds both values
    not_done = -(BT.rep_rows(done, N).to(torch.int64) - 1)
    reward_local = dc["local_rewards"].to(reward_dtype)
    for kind in BF.KINDS:
        out = _value(N, kind).v_rows(*_value_args(dc, kind), reward_local, done, GAMMA)
        assert out["v64"].dtype == torch.float64 and torch.equal(out["v64"], out["v"].double())
        want = BT.td_target(reward_local.reshape(-1), out["v64"], not_done, GAMMA)
        assert out["td"].dtype == torch.float64 and torch.equal(_bits(out["td"]), _bits(want)), kind
        assert torch.equal(want, reward_local.reshape(-1).double() + GAMMA * out["v64"].reshape(-1) * not_done)      # (the torch composition)
    if N > 1:
        reward = dc["reward"].to(reward_dtype)                                    # the GLOBAL reward [B]
        out = _coma(N).q_rows(*_coma_args(dc, acts), reward, done, GAMMA)
        assert out["q_taken64"].dtype == torch.float64 and torch.equal(out["q_taken64"], out["q_taken"].double())
        assert torch.equal(_bits(out["q_taken"]), _bits(out["q"].gather(1, acts.reshape(-1, 1))))
        want = BT.td_target(BT.rep_rows(reward, N).contiguous(), out["q_taken64"], not_done, GAMMA)
        assert out["td"].dtype == torch.float64 and torch.equal(_bits(out["td"]), _bits(want))


@pytest.mark.parametrize("N", BF.COMA_AGENTS)
def test_q_taken_is_the_own_action_and_the_others_actions_matter(N):
    B = 13
    critic, dc = _coma(N), _dev(N, B)
    a = BF.case(N, B)[1].reshape(B, N).to(DEV)
    out = critic.q_rows(*_coma_args(dc, a))
    assert torch.equal(_bits(out["q_taken"]), _bits(out["q"].gather(1, a.reshape(-1, 1))))
    # agent 0 of step 0 takes another action: its own row keeps its q (the input holds the OTHERS' actions) and moves only along
    # its row of q for q_taken; the rows of the other agents of that step change; every other step keeps its bits
    a2 = a.clone()
    a2[0, 0] = (a2[0, 0] + 1) % 5
    out2 = critic.q_rows(*_coma_args(dc, a2))
    assert torch.equal(_bits(out2["q"][0]), _bits(out["q"][0]))
    assert torch.equal(_bits(out2["q_taken"][0]), _bits(out["q"][0, a2[0, 0]].reshape(1)))
    assert bool((out2["q"][1:N] != out["q"][1:N]).any(dim=1).all())
    assert torch.equal(_bits(out2["q"][N:]), _bits(out["q"][N:]))


@pytest.mark.parametrize("N,B", [(3, 3), (1, 13), (8, 1), (1, 1), (5, 67)])
def test_rows_past_the_count_are_untouched_and_single_outputs_agree(N, B):
    dc, acts = _dev(N, B), BF.case(N, B)[1]
    R = B * N
    full = lambda dt: torch.full((R + PAD,), CANARY, dtype=dt, device=DEV)      # noqa: E731
    go, dn, rw = dc["goals"].contiguous(), dc["done"].view(torch.uint8), dc["local_rewards"].contiguous()
    for kind in BF.KINDS:
        net = _value(N, kind)
        cols = (dict(windows=dc["next_obs_self_t"], obs_self_v=dc["next_obs_self_v"], obs_others=dc["next_obs_others"] if N > 1 else None)
                if kind == "local" else dict(grid=dc["next_grid"], vec=dc["next_vec"]))
        v, v64, td = full(torch.float32), full(torch.float64), full(torch.float64)
        net.enqueue(B, go, reward=rw, done=dn, gamma=GAMMA, v=v, v64=v64, td=td, **cols)
        torch.cuda.synchronize()
        for t in (v, v64, td):
            assert bool((t[R:] == CANARY).all()) and not bool((t[:R] == CANARY).any()), (kind, t.dtype)
        alone = full(torch.float32)
        net.enqueue(B, go, v=alone, **cols)
        assert torch.equal(_bits(alone), _bits(v))
        alone = full(torch.float64)
        net.enqueue(B, go, v64=alone, **cols)
        assert torch.equal(_bits(alone), _bits(v64))
        alone = full(torch.float64)
        net.enqueue(B, go, reward=rw, done=dn, gamma=GAMMA, td=alone, **cols)
        assert torch.equal(_bits(alone), _bits(td))
    if N == 1:
        return
    critic = _coma(N)
    ac, rg = acts.to(DEV).to(torch.int32), dc["reward"].contiguous()
    ins = (dc["next_grid"], dc["next_vec"], go, dc["next_obs_self_t"], dc["next_obs_self_v"], ac)
    q = torch.full((R + PAD, 5), CANARY, dtype=torch.float32, device=DEV)
    qt, qt64, td = full(torch.float32), full(torch.float64), full(torch.float64)
    critic.enqueue(B, *ins, ac, rg, dn, GAMMA, q=q, q_taken=qt, q_taken64=qt64, td=td)
    torch.cuda.synchronize()
    for t in (q, qt, qt64, td):
        assert bool((t[R:] == CANARY).all()) and not bool((t[:R] == CANARY).any()), t.dtype
    alone = torch.full((R + PAD, 5), CANARY, dtype=torch.float32, device=DEV)
    critic.enqueue(B, *ins, q=alone)                                             # (q alone needs no own action)
    assert torch.equal(_bits(alone), _bits(q))
    for name, ref, dt in (("q_taken", qt, torch.float32), ("q_taken64", qt64, torch.float64)):
        alone = full(dt)
        critic.enqueue(B, *ins, ac, **{name: alone})
        assert torch.equal(_bits(alone), _bits(ref)), name
    alone = full(torch.float64)
    critic.enqueue(B, *ins, ac, rg, dn, GAMMA, td=alone)
    assert torch.equal(_bits(alone), _bits(td))


# ---- weights --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,N", [("local", 1), ("local", 3), ("global", 2), ("global", 8), ("coma", 2), ("coma", 5)])
def test_repack_and_soft_update_follow_the_weights(net, N):
    from cm3_amd.baseline import CK_COMA_NAMES, CK_VALUE_NAMES, CheckersComaCritic, CheckersValue
    B = 3
    dc, acts, feeds = _dev(N, B), BF.case(N, B)[1].to(DEV), BF.case(N, B)[2]
    if net == "coma":
        names = CK_COMA_NAMES
        init = lambda seed, n=N: BR.init_coma_weights(np.random.default_rng(seed), n)      # noqa: E731
        make = lambda w, n=N: CheckersComaCritic(w, n, device=DEV)      # noqa: E731
        launch = lambda c: c.q_rows(*_coma_args(dc, acts))["q"]      # noqa: E731
        ref = lambda w: BF.ref_on_feed(w, feeds[False]["Q_target"], "coma", N, np.float64)      # noqa: E731
    else:
        names = CK_VALUE_NAMES[net]
        init = lambda seed, n=N: BR.init_value_weights(np.random.default_rng(seed), n, net)      # noqa: E731
        make = lambda w, n=N: CheckersValue(w, n, kind=net, stage=1 if n == 1 else 2, device=DEV)      # noqa: E731
        launch = lambda c: c.v_rows(*_value_args(dc, net))["v"]      # noqa: E731
        ref = lambda w: BF.ref_on_feed(w, feeds[net == "local"]["V_target"], net, N, np.float64)      # noqa: E731
    w_a, w_b = init(1), init(2)
    target, main = make(w_a), make(w_b)
    assert sorted(target.w) == sorted(s for s in names if names[s] in w_a)      # short names
    before = launch(target)
    BF.within(before.cpu().numpy(), ref(w_a), what="before")
    # in place, as a session that trains the network writes its variables; the launch follows only after repack()
    for short, t in target.w.items():
        t.copy_(torch.as_tensor(w_b[names[short]]))
    assert torch.equal(_bits(launch(target)), _bits(before))
    target.repack()
    assert torch.equal(_bits(launch(target)), _bits(launch(main)))
    # soft update: float32 arithmetic on the TF-shaped tensors (the torch formula), then one pack launch
    tau = 0.01
    for short, t in target.w.items():
        t.copy_(torch.as_tensor(w_a[names[short]]))
    want = {s: tau * main.w[s] + (1.0 - tau) * target.w[s] for s in target.w}
    target.soft_update_from(main, tau)
    for s in want:
        assert want[s].dtype == torch.float32 and torch.equal(_bits(target.w[s]), _bits(want[s])), s
    mixed = {names[s]: v.cpu().numpy() for s, v in want.items()}
    BF.within(launch(target).cpu().numpy(), ref(mixed), what="after the soft update")
    other_n = 3 if N == 2 else 2
    with pytest.raises(Exception, match="soft_update_from"):
        target.soft_update_from(make(init(3, other_n), other_n), tau)


def test_scope_prefixes_and_suffixes_are_ignored_and_the_classes_are_exported_lazily():
    import cm3_amd
    N, B = 2, 3
    dc = _dev(N, B)
    w = BF.value_weights(N, "global")                                             # keys "V_target/..."
    renamed = {"V_main/" + BR.canon(k) + ":0": v for k, v in w.items()}
    a = cm3_amd.CheckersValue(renamed, N, kind="global", device=DEV).v_rows(*_value_args(dc, "global"))["v"]
    assert torch.equal(_bits(a), _bits(_value(N, "global").v_rows(*_value_args(dc, "global"))["v"]))
    wq = {"Q_main/" + BR.canon(k) + ":0": v for k, v in BF.coma_weights(N).items()}
    acts = BF.case(N, B)[1].to(DEV)
    q = cm3_amd.CheckersComaCritic(wq, N, device=DEV).q_rows(*_coma_args(dc, acts))["q"]
    assert torch.equal(_bits(q), _bits(_coma(N).q_rows(*_coma_args(dc, acts))["q"]))
