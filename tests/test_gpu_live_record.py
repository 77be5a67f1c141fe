"""GPU: packed live records (cm3_particle_traj.live_record) -- the per-tick, random-action, float32, live-state collection of the
lane-per-pair kernel steps on ONE 128-byte record per env instead of the env's five live arrays.

Every array of the collected trajectory, and the env's own state / goals / meta / episode buffers after the collect, must equal
bit for bit what the slot-chained path of the same build gives (ParticleRollout(..., live_state=False): kernels the record variant
does not touch), and cm3_last_kernel_variant must say which build ran.  Shapes are the smallest that can go wrong: partial wave,
partial workgroup, more than one workgroup (E = 1, 5, 37, 259), every agent count a record holds (N = 2, 3, 4), max_steps = 3 over
T = 8 ticks so that every env restarts at least twice (terminal slots, sparse goal slots, the counters of the record), a global
env id base, a sub-batch, consecutive collects, and a buffer-parity flip.  One case goes straight against the float64 oracle."""
import numpy as np
import pytest
import torch

from oracle import philox
from oracle.particle_oracle import VecParticleOracle
from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu

CFG = "particle_merge8.json"       # (presets for eight agents: serves every N here)
SEED, BASE, T, MAX_STEPS, P_RANDOM = 77, 1000, 8, 3, 0.5
ARRAYS = ("state", "goals", "obs_others", "actions", "reward", "reward_n", "done", "term_state", "term_obs_others", "collisions")


def _env(N, E, dtype=torch.float32, kernel="auto"):
    from cm3_amd.particle import VecParticleEnv
    env = VecParticleEnv(load_cfg(CFG), N, P_RANDOM, MAX_STEPS, E, device="cuda:0", dtype=dtype, seed=SEED, auto_reset=True,
                         env_id_base=BASE, kernel=kernel)
    env.reset()
    return env


def _pair(N, E, **kw):
    """(envs, collectors): [0] live state (packed records where they apply), [1] slot-chained."""
    from cm3_amd.rollout import ParticleRollout
    envs = [_env(N, E, **kw) for _ in range(2)]
    return envs, [ParticleRollout(env, n_ticks=T, use_graph=True, live_state=live) for env, live in zip(envs, (True, False))]


def _variant():
    from cm3_amd import _lib
    return _lib.last_kernel_variant()


def _collect(ros, want_record=True):
    """One collect on both collectors, asserting which build stepped each (where this call captured the graph: a replay calls no
    launcher, so cm3_last_kernel_variant then still names an earlier call)."""
    caps = [ro.n_captures for ro in ros]
    a = ros[0].collect(reset=False)
    va = _variant()
    b = ros[1].collect(reset=False)
    vb = _variant()
    assert a._live and not b._live
    if a.n_captures > caps[0]:
        assert va.startswith("k_particle_step_pairs<") and ",live=1," in va and (",rec=1" in va) == want_record, va
    if b.n_captures > caps[1]:
        assert ",live=0," in vb and ",rec=1" not in vb, vb
    return a, b


def _assert_same(a, b, envs, tag, sel=slice(None)):
    """Trajectories and env buffers of the two paths, bit for bit, over the envs `sel`."""
    done = a.done.bool()
    for name in ARRAYS:
        x, y = getattr(a, name), getattr(b, name)
        if name in ("state", "goals", "term_state"):
            x, y = x.permute(0, 2, 1, 3), y.permute(0, 2, 1, 3)      # -> [slot, E, N, .]
        x, y = x[:, sel], y[:, sel]
        if name in ("term_state", "term_obs_others"):                # defined where an episode ended
            x, y = x[done[:, sel]], y[done[:, sel]]
        assert torch.equal(x, y), (name, tag)
    for attr in ("global_state", "goals", "steps", "collisions", "episode"):
        assert torch.equal(getattr(envs[0], attr)[sel], getattr(envs[1], attr)[sel]), (attr, tag)
    assert torch.equal(envs[0]._meta[sel], envs[1]._meta[sel]), tag


@pytest.mark.parametrize("N", [2, 3, 4])
@pytest.mark.parametrize("E", [1, 5, 37, 259])
def test_record_collection_equals_slot_chained(N, E):
    """Two consecutive collect(reset=False) calls on one object (pack -> 8 ticks -> unpack, twice)."""
    envs, ros = _pair(N, E)
    for rep in range(2):
        a, b = _collect(ros)
        _assert_same(a, b, envs, (N, E, rep))
        assert int(a.done.sum(0).min()) >= 2          # every env restarted at least twice
        assert torch.equal(envs[0].get_obs()[1], envs[1].get_obs()[1])
    assert ros[0].n_captures == 1
    for ro in ros:
        ro.close()


def test_record_sub_batch_leaves_other_envs_alone():
    """desc->env_offset / env_count: the launches -- pack and unpack included -- cover envs [37, 167) of 259 only."""
    N, E, lo, cnt = 4, 259, 37, 130
    envs, ros = _pair(N, E)
    for env in envs:
        env._desc.env_offset, env._desc.env_count = lo, cnt
    before = [t.clone() for t in (envs[0]._state[envs[0]._cur], envs[0]._goals, envs[0]._meta, envs[0]._episode)]
    a, b = _collect(ros)
    sel = slice(lo, lo + cnt)
    _assert_same(a, b, envs, "sub-batch", sel)
    assert int(a.done[:, sel].sum(0).min()) >= 2 and not bool(a.done[:, :lo].any()) and not bool(a.done[:, lo + cnt:].any())
    out = torch.ones(E, dtype=torch.bool, device="cuda:0")
    out[sel] = False
    after = (envs[0]._state[envs[0]._cur], envs[0]._goals, envs[0]._meta, envs[0]._episode)
    for k, (x, y) in enumerate(zip(before, after)):
        env_axis = 1 if k < 2 else 0
        assert torch.equal(x.index_select(env_axis, out.nonzero().flatten()), y.index_select(env_axis, out.nonzero().flatten())), k
    for ro in ros:
        ro.close()


def test_record_follows_buffer_parity_flip():
    """collect, env.step(), collect: the env's current state buffer changes, the graph is captured again, and the records are
    packed from -- and unpacked into -- the new one."""
    N, E = 4, 37
    envs, ros = _pair(N, E)
    a, b = _collect(ros)
    _assert_same(a, b, envs, "before the flip")
    for env in envs:
        env.step()
    assert torch.equal(envs[0].global_state, envs[1].global_state) and envs[0]._cur == 1
    a, b = _collect(ros)
    _assert_same(a, b, envs, "after the flip")
    assert ros[0].n_captures == 2
    for ro in ros:
        ro.close()


@pytest.mark.parametrize("N,dtype,kernel", [(5, torch.float32, "auto"), (4, torch.float64, "auto"), (4, torch.float32, "agent"),
                                            (4, torch.float32, "env")])
def test_other_shapes_keep_the_plain_live_path(N, dtype, kernel):
    """Five agents do not fit a record, float64 is the parity path, and the other mappings have no record variant: all of them
    collect as before (and still equal the slot-chained path)."""
    envs, ros = _pair(N, 37, dtype=dtype, kernel=kernel)
    a = ros[0].collect(reset=False)
    v = _variant()
    b = ros[1].collect(reset=False)
    assert a._live and ",rec=1" not in v, v
    assert ",live=1," in v or kernel == "env", v      # (the lane-per-env kernel has no live variant to report: a run-time pointer)
    assert v.startswith({"auto": "k_particle_step_pairs<", "agent": "k_particle_step_agents<", "env": "k_particle_step<"}[kernel]), v
    assert ("<f64," in v) == (dtype == torch.float64)
    _assert_same(a, b, envs, (N, dtype, kernel))
    for ro in ros:
        ro.close()


def test_record_collection_vs_f64_oracle_teacher_forced():
    """The record variant against the float64 oracle directly: every tick the oracle is given slot t of the device trajectory
    (state, goals, counters) and the kernel's actions; slot t + 1 / the terminal capture, rewards, done and collision counts must
    equal its step within the project's float32 bound (1e-5).  The in-kernel actions -- stage 1 now read from the record -- and the
    same-launch resets are checked against the Philox specification with GLOBAL env ids."""
    from cm3_amd.rollout import ParticleRollout
    N, E, TOL, EDGE = 4, 259, 1e-5, 2e-6
    cfg = load_cfg(CFG)
    env = _env(N, E)
    ro = ParticleRollout(env, n_ticks=T, use_graph=True, live_state=True).collect(reset=False)
    assert ",rec=1" in _variant()
    f64 = lambda x: x.detach().cpu().numpy().astype(np.float64)     # noqa: E731
    state, goals = f64(ro.state).transpose(0, 2, 1, 3), f64(ro.goals).transpose(0, 2, 1, 3)       # [T+1, E, N, .]
    obs, term_state, term_obs = f64(ro.obs_others), f64(ro.term_state).transpose(0, 2, 1, 3), f64(ro.term_obs_others)
    acts, rew, rew_n = ro.actions.cpu().numpy(), f64(ro.reward), f64(ro.reward_n)
    done, coll = ro.done.cpu().numpy().astype(bool), ro.collisions.cpu().numpy()
    ro.close()
    orc = VecParticleOracle(N, cfg, P_RANDOM, MAX_STEPS, E)
    ids = BASE + np.arange(E)
    steps, prev_coll, episode = np.zeros(E, np.int64), np.zeros(E, np.int64), np.ones(E, np.int64)   # after the first reset
    n_done = 0
    for t in range(T):
        for ep in np.unique(episode):
            for st in np.unique(steps[episode == ep]):
                m = (episode == ep) & (steps == st)
                assert np.array_equal(acts[t][m], philox.expected_actions(SEED, ids[m], int(ep), int(st), N)), t
        orc.set_from_global_state(state[t], goals[t], steps=steps, collisions=prev_coll)
        w_gs, w_oo, _, w_rew, w_rn, w_done = orc.step(acts[t])
        m_col, m_reach = orc.pair_margins()
        safe = (m_col > EDGE) & (m_reach > EDGE)
        d = done[t]
        got_gs = np.where(d[:, None, None], term_state[t], state[t + 1])
        got_oo = np.where(d[:, None, None], term_obs[t], obs[t + 1])
        assert np.abs(got_gs - w_gs).max() < TOL and np.abs(got_oo - w_oo).max() < TOL, t
        assert np.abs(rew_n[t][safe] - w_rn[safe]).max() < TOL and np.abs(rew[t][safe] - w_rew[safe]).max() < 4 * TOL, t
        assert np.array_equal(d[safe], w_done[safe]), t
        assert np.array_equal(coll[t][safe], orc.collisions[safe]), t
        if d.any():
            n_done += int(d.sum())
            episode = episode + d
            for ep in np.unique(episode[d]):
                m = d & (episode == ep)
                pos, lm, _ = philox.expected_reset(SEED, ids[m], int(ep), cfg, N, P_RANDOM)
                assert np.abs(state[t + 1][m][..., 2:4] - pos).max() < 1e-6 and np.abs(goals[t + 1][m] - lm).max() < 1e-6
                assert np.abs(state[t + 1][m][..., 0:2]).max() == 0.0
        steps = np.where(d, 0, steps + 1)
        prev_coll = np.where(d, 0, coll[t])
    assert n_done >= 2 * E
