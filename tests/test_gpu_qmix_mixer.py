"""GPU: the particle QMIX mixer over transition rows (cm3_qmix_mixer_particle_rows_f32; cm3_amd.qmix.ParticleQmixMixer) -- q_tot
against tests/qmix_mixer_ref.py in float64, the fixture recorded from the reference's own function body, the bit identities between
the outputs, the TD target and launches of different sizes, and the weight updates.

Bound: the project's 2e-5 * max(1, |ref|) per row (tests/critic_feeds.py:within).  Inputs as in the fixture: weights from
init_weights(scale=0.5), states uniform in +-2, goals in +-1, agent_qs in +-5; |q_tot| runs from 0.005 to 222 over the cases, so both
the absolute and the relative part of the bound are live.  The float32 NumPy restatement of the same rows uses at most 0.14 of the
bound in the shim's matmul order and 0.18 in the kernel's order (both at N = 3, B = 67; every other case less).  The device's
hyper-network is a k-ordered chain per output where NumPy's is a blocked matmul, so its share is its own; each test prints it."""
import numpy as np
import pytest
import torch

from tests import critic_feeds as CF
from tests import qmix_mixer_ref as MR
from tests.test_qmix_mixer_oracle import load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGENTS = [1, 2, 3, 4, 8, 10]
BATCHES = [1, 3, 13, 67]
GAMMA = 0.99
_CACHE = {}


def _mixer(N):
    """(mixer, its weights): once per agent count; tests that change weights build their own"""
    if N not in _CACHE:
        from cm3_amd.qmix import ParticleQmixMixer
        w = MR.init_weights(np.random.default_rng(700 + N), N, scale=0.5, scope="Mixer_target")
        _CACHE[N] = (ParticleQmixMixer(w, N, device=DEV), w)
    return _CACHE[N]


def host_case(N, B):
    """the columns of B transitions as NumPy arrays: state [B, N, 4], goals [B, N, 2], agent_qs [B, N], reward_local [B, N], done [B]"""
    rng = np.random.default_rng(9000 + 131 * N + B)
    u = lambda lo, *s: rng.uniform(-lo, lo, s).astype(np.float32)      # noqa: E731
    return {"state": u(2, B, N, 4), "goals": u(1, B, N, 2), "agent_qs": u(5, B, N), "reward_local": u(1, B, N), "done": rng.random(B) < 0.4}


def _case(N, B):
    """(host columns, device columns, float64 reference [B]): once per shape, left unchanged"""
    key = ("case", N, B)
    if key not in _CACHE:
        h = host_case(N, B)
        w = _mixer(N)[1]
        ref = MR.q_tot(w, h["agent_qs"], h["state"], h["goals"], dtype=np.float64).reshape(-1)
        _CACHE[key] = (h, {k: torch.as_tensor(v).to(DEV) for k, v in h.items()}, ref)
    return _CACHE[key]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ---- against float64 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", AGENTS)
def test_launch_matches_float64(N, B):
    from cm3_amd import _lib
    mixer, _ = _mixer(N)
    _, d, ref = _case(N, B)
    out = mixer.q_tot(d["state"], d["goals"], d["agent_qs"])
    torch.cuda.synchronize()
    assert _lib.last_kernel_variant().startswith("k_qmix_mixer_rows<f32,N=%d," % N), _lib.last_kernel_variant()
    assert sorted(out) == ["q_tot", "q_tot64"]
    assert out["q_tot"].dtype == torch.float32 and tuple(out["q_tot"].shape) == (B, 1)
    assert out["q_tot64"].dtype == torch.float64 and tuple(out["q_tot64"].shape) == (B, 1)
    CF.within(out["q_tot"].cpu().numpy(), ref, what="q_tot N=%d B=%d" % (N, B))
    # the flattened forms of the columns (the feeds' v_state [B, 4N] and v_goal_all [B, 2N]) are the same launch
    flat = mixer.q_tot(d["state"].reshape(B, -1), d["goals"].reshape(B, -1), d["agent_qs"].reshape(-1).double())
    assert torch.equal(_bits(flat["q_tot"]), _bits(out["q_tot"]))


@pytest.mark.parametrize("N", AGENTS)
def test_fixture_rows(N):
    from cm3_amd.qmix import ParticleQmixMixer
    w, x, q = load_case(N)
    mixer = ParticleQmixMixer(w, N, device=DEV)
    t = lambda a: torch.as_tensor(a)                                   # noqa: E731  (host columns are staged)
    out = mixer.q_tot(t(x["state"]), t(x["goals_all"]), t(x["agent_qs"]))
    torch.cuda.synchronize()
    assert tuple(out["q_tot"].shape) == q.shape
    CF.within(out["q_tot"].cpu().numpy(), q, what="fixture N=%d" % N)


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reward_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B", [13, 67])
@pytest.mark.parametrize("N", AGENTS)
def test_q64_and_td_are_the_bits_of_qmix_td_target(N, B, reward_dtype):
    from cm3_amd import batch as BR
    mixer, _ = _mixer(N)
    h, d, ref = _case(N, B)
    reward = d["reward_local"].to(reward_dtype)
    done = d["done"]
    assert 0 < int(done.sum()) < B
    out = mixer.q_tot(d["state"], d["goals"], d["agent_qs"], reward, done, GAMMA)
    assert sorted(out) == ["q_tot", "q_tot64", "td"]
    assert torch.equal(_bits(out["q_tot64"]), _bits(out["q_tot"].double()))
    want = BR.qmix_td_target(reward, out["q_tot"], done, GAMMA)
    assert out["td"].dtype == torch.float64 and tuple(out["td"].shape) == (B,)
    assert torch.equal(_bits(out["td"]), _bits(want))
    # ... which is NumPy's expression of alg_qmix.py:367-369 on a session's float32 q_tot
    q = out["q_tot"].cpu().numpy()
    numpy_td = np.sum(h["reward_local"].astype(np.float64), axis=1) + GAMMA * np.squeeze(q) * (-(h["done"].astype(np.int64) - 1))
    assert np.array_equal(out["td"].cpu().numpy(), numpy_td)
    # integer done is the same launch; without the TD arguments the mixer's own outputs keep their bits
    again = mixer.q_tot(d["state"], d["goals"], d["agent_qs"], reward, done.to(torch.int64), GAMMA)
    assert torch.equal(_bits(again["td"]), _bits(out["td"]))
    assert torch.equal(_bits(mixer.q_tot(d["state"], d["goals"], d["agent_qs"])["q_tot"]), _bits(out["q_tot"]))
    with pytest.raises(Exception, match="come together"):
        mixer.q_tot(d["state"], d["goals"], d["agent_qs"], reward, done)


@pytest.mark.parametrize("N", AGENTS)
def test_a_row_of_a_large_launch_has_the_bits_of_a_launch_of_its_own(N):
    mixer, _ = _mixer(N)
    B = 67
    _, d, _ = _case(N, B)
    whole = mixer.q_tot(d["state"], d["goals"], d["agent_qs"], d["reward_local"], d["done"], GAMMA)
    for b in (0, 5, 15, 16, 63, 64, 66):
        one = mixer.q_tot(d["state"][b:b + 1], d["goals"][b:b + 1], d["agent_qs"][b:b + 1], d["reward_local"][b:b + 1], d["done"][b:b + 1], GAMMA)
        for k in ("q_tot", "q_tot64", "td"):
            assert torch.equal(_bits(one[k].reshape(-1)), _bits(whole[k].reshape(-1)[b:b + 1])), (b, k)


@pytest.mark.parametrize("N,B", [(4, 3), (1, 13), (10, 67), (3, 1)])
def test_rows_past_the_count_are_untouched_and_single_outputs_agree(N, B):
    mixer, _ = _mixer(N)
    _, d, _ = _case(N, B)
    st, go, aq = d["state"].contiguous(), d["goals"].contiguous(), d["agent_qs"].contiguous()
    rw, dn = d["reward_local"].contiguous(), d["done"].contiguous().view(torch.uint8)
    pad = 200                                                            # more than a workgroup's rows of canaries
    full = lambda dt: torch.full((B + pad,), -7.5, dtype=dt, device=DEV)  # noqa: E731
    q, q64, td = full(torch.float32), full(torch.float64), full(torch.float64)
    mixer.enqueue(B, st, go, aq, rw, dn, GAMMA, q_tot=q, q_tot64=q64, td=td)
    torch.cuda.synchronize()
    for t in (q, q64, td):
        assert bool((t[B:] == -7.5).all()) and not bool((t[:B] == -7.5).any()), t.dtype
    alone = full(torch.float32)
    mixer.enqueue(B, st, go, aq, q_tot=alone)
    assert torch.equal(_bits(alone), _bits(q))
    alone = full(torch.float64)
    mixer.enqueue(B, st, go, aq, q_tot64=alone)
    assert torch.equal(_bits(alone), _bits(q64))
    alone = full(torch.float64)
    mixer.enqueue(B, st, go, aq, rw, dn, GAMMA, td=alone)
    assert torch.equal(_bits(alone), _bits(td))


# ---- weights ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 4])
def test_repack_and_soft_update_follow_the_weights(N):
    from cm3_amd.qmix import MIXER_NAMES, ParticleQmixMixer
    w_a = MR.init_weights(np.random.default_rng(1), N)
    w_b = MR.init_weights(np.random.default_rng(2), N, scope="Mixer_main")
    target, main = ParticleQmixMixer(w_a, N, device=DEV), ParticleQmixMixer(w_b, N, device=DEV)
    h, d, _ = _case(N, 13)
    ref = lambda w: MR.q_tot(w, h["agent_qs"], h["state"], h["goals"], dtype=np.float64)      # noqa: E731
    launch = lambda m: m.q_tot(d["state"], d["goals"], d["agent_qs"])["q_tot"]                # noqa: E731
    before = launch(target)
    CF.within(before.cpu().numpy(), ref(w_a), what="before")
    # in place, as a session that trains the network writes its variables; the launch follows only after repack()
    for short, t in target.w.items():
        t.copy_(torch.as_tensor(w_b["Mixer_main/" + MIXER_NAMES[short]]))
    assert torch.equal(_bits(launch(target)), _bits(before))
    target.repack()
    after = launch(target)
    assert torch.equal(_bits(after), _bits(launch(main))) and not torch.equal(_bits(after), _bits(before))
    CF.within(after.cpu().numpy(), ref(w_b), what="after repack")
    # soft update: float32 arithmetic on the TF-shaped tensors, then one pack launch
    tau = 0.01
    for short, t in target.w.items():
        t.copy_(torch.as_tensor(w_a[MIXER_NAMES[short]]))
    want = {s: tau * main.w[s] + (1.0 - tau) * target.w[s] for s in target.w}
    target.soft_update_from(main, tau)
    assert sorted(want) == sorted(MIXER_NAMES)
    for s in want:
        assert want[s].dtype == torch.float32 and torch.equal(_bits(target.w[s]), _bits(want[s])), s
    mixed = {MIXER_NAMES[s]: v.cpu().numpy() for s, v in want.items()}
    CF.within(launch(target).cpu().numpy(), ref(mixed), what="after the soft update")
    other = ParticleQmixMixer(MR.init_weights(np.random.default_rng(3), N + 1), N + 1, device=DEV)
    with pytest.raises(Exception, match="soft_update_from"):
        target.soft_update_from(other, tau)
    with pytest.raises(Exception, match="soft_update_from"):
        target.soft_update_from(object(), tau)


def test_missing_names_and_wrong_shapes_are_refused():
    from cm3_amd import Cm3Error
    from cm3_amd.qmix import ParticleQmixMixer
    w = MR.init_weights(np.random.default_rng(0), 2)
    with pytest.raises(Cm3Error, match="missing mixer weight 'hyper_b_1'"):
        ParticleQmixMixer({k: v for k, v in w.items() if k != "hyper_b_1"}, 2, device=DEV)
    with pytest.raises(Cm3Error, match="has shape"):
        ParticleQmixMixer(w, 3, device=DEV)
    with pytest.raises(Cm3Error, match="n_agents must be in 1..10"):
        ParticleQmixMixer(w, 11, device=DEV)
    with pytest.raises(Cm3Error, match="agent_qs"):
        _mixer(2)[0].q_tot(torch.zeros(3, 2, 4), torch.zeros(3, 2, 2), torch.zeros(3, 3))
