"""GPU: the Checkers QMIX mixer over transition rows (cm3_qmix_mixer_checkers_rows_f32; cm3_amd.qmix.CheckersQmixMixer) -- q_tot
against tests/qmix_mixer_checkers_ref.py in float64, the fixtures recorded from the reference's own function body, the bit identities
between the input forms, the outputs, the TD target and launches of different sizes, and the weight updates.

Bound: the project's 2e-5 * max(1, |ref|) per row (tests/critic_feeds.py:within).  Cases: MR.gpu_case / MR.gpu_weights -- weights from
init_weights(scale=0.5), grids in {0, 1}, states uniform in +-2, one-hot goals, agent_qs in +-5; |q_tot| runs from 0.098 to 145 over
the cases, so both the absolute and the relative part of the bound are live.  The float32 NumPy restatement of the same rows uses at
most 0.063 of the bound in the shim's matmul order and 0.039 in the kernel's order (both at N = 5, B = 67; every other case less;
tests/test_qmix_mixer_checkers_oracle.py asserts at most half).  The device's convolution and hyper-network are one chain per output
in the tile loop's k order where NumPy's are blocked matmuls, so its share is its own; each test prints it.

The kernel gives 16 rows to a workgroup: B = 67 is four whole workgroups and a partial fifth."""
import numpy as np
import pytest
import torch

from tests import critic_feeds as CF
from tests import qmix_mixer_checkers_ref as MR
from tests.test_qmix_mixer_checkers_oracle import load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGENTS = list(MR.GPU_AGENTS)
BATCHES = list(MR.GPU_BATCHES)
GAMMA = 0.99
_CACHE = {}


def _mixer(N):
    """the mixer of MR.gpu_weights: once per agent count; tests that change weights build their own"""
    if N not in _CACHE:
        from cm3_amd.qmix import CheckersQmixMixer
        _CACHE[N] = CheckersQmixMixer(MR.gpu_weights(N), N, device=DEV)
    return _CACHE[N]


def _case(N, B):
    """(host columns, device columns in the compact forms, float64 reference [B]): once per shape, left unchanged"""
    key = ("case", N, B)
    if key not in _CACHE:
        h = MR.gpu_case(N, B)
        _CACHE[key] = (h, {k: torch.as_tensor(v).to(DEV) for k, v in h.items()}, MR.gpu_ref(N, B))
    return _CACHE[key]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _q(mixer, d, **kw):
    cols = dict(d, **kw)
    return mixer.q_tot(cols["grid"], cols["vec"], cols["goals"], cols["agent_qs"])["q_tot"]


# ---- against float64 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", AGENTS)
def test_launch_matches_float64(N, B):
    from cm3_amd import _lib
    mixer = _mixer(N)
    _, d, ref = _case(N, B)
    out = mixer.q_tot(d["grid"], d["vec"], d["goals"], d["agent_qs"])
    torch.cuda.synchronize()
    assert _lib.last_kernel_variant().startswith("k_ck_qmix_mixer_rows<f32,N=%d," % N), _lib.last_kernel_variant()
    assert sorted(out) == ["q_tot", "q_tot64"]
    assert out["q_tot"].dtype == torch.float32 and tuple(out["q_tot"].shape) == (B, 1)
    assert out["q_tot64"].dtype == torch.float64 and tuple(out["q_tot64"].shape) == (B, 1)
    CF.within(out["q_tot"].cpu().numpy(), ref, what="q_tot N=%d B=%d" % (N, B))
    assert torch.equal(_bits(out["q_tot64"]), _bits(out["q_tot"].double()))


@pytest.mark.parametrize("B", [3, 67])
@pytest.mark.parametrize("N", AGENTS)
def test_input_forms_give_the_same_bits(N, B):
    """int8 / float64 grids, uint8 index / int64 one-hot (and int64 index) goals, flattened column shapes, float64 agent_qs"""
    mixer = _mixer(N)
    _, d, _ = _case(N, B)
    base = _q(mixer, d)
    onehot = torch.nn.functional.one_hot(d["goals"].long(), 2)
    assert onehot.dtype == torch.int64 and tuple(onehot.shape) == (B, N, 2)
    assert torch.equal(_bits(_q(mixer, d, grid=d["grid"].double())), _bits(base))
    assert torch.equal(_bits(_q(mixer, d, goals=onehot)), _bits(base))
    assert torch.equal(_bits(_q(mixer, d, goals=d["goals"].long())), _bits(base))
    assert torch.equal(_bits(_q(mixer, d, grid=d["grid"].double(), goals=onehot)), _bits(base))
    # the flattened forms (the feeds' state_env [B, 3, 9, 2], v_state [B, 4N] and v_goal_all [B, 2N]) are the same launch
    flat = _q(mixer, d, grid=d["grid"].double().reshape(B, 54), vec=d["vec"].reshape(B, -1), goals=onehot.reshape(B, -1),
              agent_qs=d["agent_qs"].reshape(-1).double())
    assert torch.equal(_bits(flat), _bits(base))


@pytest.mark.parametrize("N", [1, 2, 3, 5])
def test_fixture_rows(N):
    from cm3_amd.qmix import CheckersQmixMixer
    w, x, q = load_case(N)
    mixer = CheckersQmixMixer(w, N, device=DEV)
    t = lambda a: torch.as_tensor(a)                                   # noqa: E731  (host columns are staged)
    out = mixer.q_tot(t(x["state_env"]), t(x["state"]), t(x["goals_all"]), t(x["agent_qs"]))
    torch.cuda.synchronize()
    assert tuple(out["q_tot"].shape) == q.shape
    CF.within(out["q_tot"].cpu().numpy(), q, what="fixture N=%d" % N)


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reward_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B", [13, 67])
@pytest.mark.parametrize("N", AGENTS)
def test_q64_and_td_are_the_bits_of_qmix_td_target(N, B, reward_dtype):
    from cm3_amd import batch as BR
    mixer = _mixer(N)
    h, d, _ = _case(N, B)
    reward = d["local_rewards"].to(reward_dtype)
    done = d["done"]
    assert 0 < int(done.sum()) < B
    args = (d["grid"], d["vec"], d["goals"], d["agent_qs"])
    out = mixer.q_tot(*args, reward, done, GAMMA)
    assert sorted(out) == ["q_tot", "q_tot64", "td"]
    assert torch.equal(_bits(out["q_tot64"]), _bits(out["q_tot"].double()))
    want = BR.qmix_td_target(reward, out["q_tot"], done, GAMMA)
    assert out["td"].dtype == torch.float64 and tuple(out["td"].shape) == (B,)
    assert torch.equal(_bits(out["td"]), _bits(want))
    # ... which is NumPy's expression of alg_qmix_checkers.py:377-379 on a session's float32 q_tot
    q = out["q_tot"].cpu().numpy()
    numpy_td = np.sum(h["local_rewards"].astype(np.float64), axis=1) + GAMMA * np.squeeze(q) * (-(h["done"].astype(np.int64) - 1))
    assert np.array_equal(out["td"].cpu().numpy(), numpy_td)
    # integer done is the same launch; without the TD arguments the mixer's own outputs keep their bits
    again = mixer.q_tot(*args, reward, done.to(torch.int64), GAMMA)
    assert torch.equal(_bits(again["td"]), _bits(out["td"]))
    assert torch.equal(_bits(mixer.q_tot(*args)["q_tot"]), _bits(out["q_tot"]))
    with pytest.raises(Exception, match="come together"):
        mixer.q_tot(*args, reward, done)


@pytest.mark.parametrize("N", AGENTS)
def test_a_row_of_a_large_launch_has_the_bits_of_a_launch_of_its_own(N):
    mixer = _mixer(N)
    B = 67
    _, d, _ = _case(N, B)
    cols = ("grid", "vec", "goals", "agent_qs", "local_rewards", "done")
    whole = mixer.q_tot(*[d[k] for k in cols], GAMMA)
    for b in (0, 15, 16, 31, 32, 63, 64, 66):                             # (16 rows per workgroup)
        one = mixer.q_tot(*[d[k][b:b + 1] for k in cols], GAMMA)
        for k in ("q_tot", "q_tot64", "td"):
            assert torch.equal(_bits(one[k].reshape(-1)), _bits(whole[k].reshape(-1)[b:b + 1])), (b, k)


@pytest.mark.parametrize("N,B", [(2, 3), (1, 13), (8, 67), (3, 1)])
def test_rows_past_the_count_are_untouched_and_single_outputs_agree(N, B):
    mixer = _mixer(N)
    _, d, _ = _case(N, B)
    gr, ve, go, aq = (d[k].contiguous() for k in ("grid", "vec", "goals", "agent_qs"))
    rw, dn = d["local_rewards"].contiguous(), d["done"].contiguous().view(torch.uint8)
    pad = 200                                                            # more than a workgroup's rows of canaries
    full = lambda dt: torch.full((B + pad,), -7.5, dtype=dt, device=DEV)  # noqa: E731
    q, q64, td = full(torch.float32), full(torch.float64), full(torch.float64)
    mixer.enqueue(B, gr, ve, go, aq, rw, dn, GAMMA, q_tot=q, q_tot64=q64, td=td)
    torch.cuda.synchronize()
    for t in (q, q64, td):
        assert bool((t[B:] == -7.5).all()) and not bool((t[:B] == -7.5).any()), t.dtype
    alone = full(torch.float32)
    mixer.enqueue(B, gr, ve, go, aq, q_tot=alone)
    assert torch.equal(_bits(alone), _bits(q))
    alone = full(torch.float64)
    mixer.enqueue(B, gr, ve, go, aq, q_tot64=alone)
    assert torch.equal(_bits(alone), _bits(q64))
    alone = full(torch.float64)
    mixer.enqueue(B, gr, ve, go, aq, rw, dn, GAMMA, td=alone)
    assert torch.equal(_bits(alone), _bits(td))


# ---- weights ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
def test_repack_and_soft_update_follow_the_weights(N):
    from cm3_amd.qmix import CK_MIXER_NAMES, CheckersQmixMixer
    w_a = MR.init_weights(np.random.default_rng(1), N)
    w_b = MR.init_weights(np.random.default_rng(2), N, scope="Mixer_main")
    target, main = CheckersQmixMixer(w_a, N, device=DEV), CheckersQmixMixer(w_b, N, device=DEV)
    h, d, _ = _case(N, 13)
    ref = lambda w: MR.q_tot(w, h["agent_qs"], h["grid"], h["vec"], np.eye(2)[h["goals"]], dtype=np.float64)      # noqa: E731
    launch = lambda m: _q(m, d)                                                                                    # noqa: E731
    before = launch(target)
    CF.within(before.cpu().numpy(), ref(w_a), what="before")
    # in place, as a session that trains the network writes its variables; the launch follows only after repack()
    for short, t in target.w.items():
        t.copy_(torch.as_tensor(w_b["Mixer_main/" + CK_MIXER_NAMES[short]]))
    assert torch.equal(_bits(launch(target)), _bits(before))
    target.repack()
    after = launch(target)
    assert torch.equal(_bits(after), _bits(launch(main))) and not torch.equal(_bits(after), _bits(before))
    CF.within(after.cpu().numpy(), ref(w_b), what="after repack")
    # soft update: float32 arithmetic on the TF-shaped tensors, then one pack launch
    tau = 0.01
    for short, t in target.w.items():
        t.copy_(torch.as_tensor(w_a[CK_MIXER_NAMES[short]]))
    want = {s: tau * main.w[s] + (1.0 - tau) * target.w[s] for s in target.w}
    target.soft_update_from(main, tau)
    assert sorted(want) == sorted(CK_MIXER_NAMES) and len(want) == 7
    for s in want:
        assert want[s].dtype == torch.float32 and torch.equal(_bits(target.w[s]), _bits(want[s])), s
    mixed = {CK_MIXER_NAMES[s]: v.cpu().numpy() for s, v in want.items()}
    CF.within(launch(target).cpu().numpy(), ref(mixed), what="after the soft update")
    other = CheckersQmixMixer(MR.init_weights(np.random.default_rng(3), N + 1), N + 1, device=DEV)
    with pytest.raises(Exception, match="soft_update_from"):
        target.soft_update_from(other, tau)
    with pytest.raises(Exception, match="soft_update_from"):
        target.soft_update_from(object(), tau)


def test_missing_names_and_wrong_shapes_are_refused():
    from cm3_amd import Cm3Error
    from cm3_amd.qmix import CheckersQmixMixer
    w = MR.init_weights(np.random.default_rng(0), 2)
    with pytest.raises(Cm3Error, match="missing mixer weight 'hyper_b_1'"):
        CheckersQmixMixer({k: v for k, v in w.items() if k != "hyper_b_1"}, 2, device=DEV)
    with pytest.raises(Cm3Error, match="missing mixer weight 'conv/Conv/weights'"):
        CheckersQmixMixer({k: v for k, v in w.items() if k != "conv/Conv/weights"}, 2, device=DEV)
    with pytest.raises(Cm3Error, match="has shape"):
        CheckersQmixMixer(w, 3, device=DEV)
    with pytest.raises(Cm3Error, match="supports 1..8 agents"):
        CheckersQmixMixer(w, 9, device=DEV)
    with pytest.raises(Cm3Error, match="agent_qs"):
        _mixer(2).q_tot(torch.zeros(3, 3, 9, 2), torch.zeros(3, 2, 4), torch.zeros(3, 2, 2), torch.zeros(3, 3))
