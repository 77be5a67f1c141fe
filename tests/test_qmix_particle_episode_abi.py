"""CPU: the C ABI of the particle QMIX agent's one-launch rollout (cm3_policy_rollout_qmix_f32, additive part of ABI 9) -- declared,
exported, bound, and every invalid argument refused with a readable error before anything touches a GPU.  Also here, because it needs
no GPU: the float64 restatement (tests/qmix_ref.py) driving the oracle env by its own choices keeps the share of clearly decided rows
that tests/test_gpu_qmix_particle_episode.py asks of every tick."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "cm3_policy_rollout_qmix_f32"
FAKE = 0x1000                                   # never dereferenced: validation fails first
SHAPES = [(1, 70), (2, 37), (4, 37), (8, 19)]   # (N, E) of the GPU tests


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    return _lib


def test_header_declares_and_library_exports_the_entry(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cm3_amd.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % ENTRY, text, flags=re.S)
    assert m, "not declared"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["const cm3_particle_desc *desc", "const cm3_particle_traj *traj", "const cm3_actor_particle_desc *agent",
                    "const void *packed", "float *q_values", "size_t q_stride", "const float *epsilon_dev", "int32_t n_ticks",
                    "void *stream"]
    handle = built.lib()
    assert hasattr(handle, ENTRY) and ENTRY in built.SYMBOLS
    res, bound = built.SYMBOLS[ENTRY]
    assert res is ctypes.c_int and len(bound) == len(args)
    assert bound[:3] == built.SYMBOLS["cm3_policy_rollout_f32"][1][:3]          # desc, traj, agent: the actor entry's types
    assert bound[5] is ctypes.c_size_t and bound[7] is ctypes.c_int32
    assert "#define CM3_ABI_VERSION 9" in text
    assert built.ABI_VERSION == 9 and handle.cm3_abi_version() == 9


def _env_desc(built, **kw):
    d = built.ParticleDesc()
    d.n_envs, d.n_agents, d.max_steps, d.flags = 16, 4, 33, 0
    d.seed, d.env_id_base, d.prob_random = 7, 0, 0.2
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _agent_desc(built, **kw):
    d = built.ActorParticleDesc()
    d.n_envs, d.n_agents, d.stage = 16, 4, 2
    d.n_h1_self, d.n_h1_others, d.n_h2, d.n_actions = 64, 0, 64, 5
    d.epsilon, d.precision = 0.1, 0
    d.seed, d.env_id_base = 7, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _traj(built, **kw):
    t = built.ParticleTraj()
    for name, ctype in t._fields_:
        if ctype is ctypes.c_void_p and name not in ("state_live", "goals_live", "live_record"):
            setattr(t, name, FAKE)
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _call(built, env=None, agent=None, traj=None, packed=FAKE, n_ticks=4, null=()):
    handle = built.lib()
    args = dict(env=_env_desc(built) if env is None else env, traj=_traj(built) if traj is None else traj,
                agent=_agent_desc(built) if agent is None else agent)
    ref = {k: (None if k in null else ctypes.byref(v)) for k, v in args.items()}
    rc = handle.cm3_policy_rollout_qmix_f32(ref["env"], ref["traj"], ref["agent"], packed, None, 0, None, n_ticks, None)
    return rc, handle.cm3_last_error()


@pytest.mark.parametrize("null", ["env", "traj", "agent"])
def test_null_arguments_are_refused(built, null):
    rc, msg = _call(built, null=(null,))
    assert rc == -1 and b"null" in msg, msg


def test_invalid_arguments_are_refused_without_a_gpu(built):
    rc, msg = _call(built, packed=None)
    assert rc == -1 and b"packed" in msg and b"cm3_qmix_particle_pack" in msg, msg
    rc, msg = _call(built, env=_env_desc(built, n_agents=3), agent=_agent_desc(built, n_agents=3))
    assert rc == -1 and b"{1, 2, 4, 8}" in msg and b"got 3" in msg, msg
    rc, msg = _call(built, agent=_agent_desc(built, n_agents=2))
    assert rc == -1 and b"disagree" in msg, msg
    rc, msg = _call(built, agent=_agent_desc(built, n_envs=8))
    assert rc == -1 and b"disagree" in msg, msg
    rc, msg = _call(built, agent=_agent_desc(built, seed=8))
    assert rc == -1 and b"seed" in msg and b"env_id_base" in msg, msg
    rc, msg = _call(built, agent=_agent_desc(built, env_id_base=16))
    assert rc == -1 and b"env_id_base" in msg, msg
    rc, msg = _call(built, agent=_agent_desc(built, precision=1))
    assert rc == -1 and b"precision" in msg and b"float32" in msg, msg
    for widths in (dict(n_h1_self=128), dict(n_h2=32), dict(n_actions=4)):
        rc, msg = _call(built, agent=_agent_desc(built, **widths))
        assert rc == -1 and b"64/64/5" in msg, msg
    rc, msg = _call(built, n_ticks=0)
    assert rc == -1 and b"n_ticks" in msg, msg
    rc, msg = _call(built, agent=_agent_desc(built, epsilon=1.5))
    assert rc == -1 and b"epsilon" in msg, msg
    rc, msg = _call(built, env=_env_desc(built, flags=built.FLAG_GEN_ACTIONS))
    assert rc == -1 and b"GEN_ACTIONS" in msg, msg
    rc, msg = _call(built, traj=_traj(built, actions=None))
    assert rc == -1 and b"trajectory base pointers" in msg, msg


def test_agent_takes_the_keyword_and_has_the_hooks():
    import inspect
    from cm3_amd.qmix import ParticleQmixAgent
    sig = inspect.signature(ParticleQmixAgent.__init__)
    assert sig.parameters["episode_kernel"].default is False
    for name in ("episode_ok", "episode_refusal", "enqueue_episode"):
        assert callable(getattr(ParticleQmixAgent, name))
    assert ParticleQmixAgent.fused_kernels is False        # fused=True / fused_policy_tick=True stay refused


def _start(cfg, N, E, rng):
    pos = np.stack([np.asarray(cfg["agents_x"][:N], np.float64), np.asarray(cfg["agents_y"][:N], np.float64)], axis=1)
    lm = np.stack([np.asarray(cfg["landmarks_x"][:N], np.float64), np.asarray(cfg["landmarks_y"][:N], np.float64)], axis=1)
    pos = pos[None] + rng.normal(0.0, float(cfg.get("initial_std", 0.0)), (E, N, 2))
    return pos, np.zeros((E, N, 2)), np.broadcast_to(lm, (E, N, 2)).copy()


@pytest.mark.parametrize("eps", [0.0, 0.3])
@pytest.mark.parametrize("N,E", SHAPES)
def test_restatement_alone_decides_nine_rows_in_ten(N, E, eps):
    """The weights, shapes and tick count of the teacher-forced GPU test: the float64 restatement + the oracle env, driven by the
    restatement's own epsilon-greedy choices for 12 ticks (finished envs restart from the config's start: episode + 1, step 0),
    leave more than 0.9 of every tick's rows with top-two Q values 1e-4 apart.  (The host starts from the config's positions and
    draws its own start noise: the same law as the device run, not the same states.)"""
    from oracle.particle_oracle import VecParticleOracle
    from tests import qmix_ref as QR
    from tests.helpers import load_cfg
    name = {1: "particle_stage1.json", 2: "particle_stage2_merge.json"}.get(N, "particle_merge8.json")
    cfg = load_cfg(name)
    T, seed, S = 12, 11, 5
    w = QR.init_weights(np.random.default_rng(100 + N), N)
    rng = np.random.default_rng(3)
    orc = VecParticleOracle(N, cfg, 0.2, S, E)
    orc.set_state(*_start(cfg, N, E, rng))
    episode, step = np.zeros(E, np.int64), np.zeros(E, np.int64)
    worst = 1.0
    for t in range(T):
        gs, oo = orc.observe()
        f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)  # noqa: E731
        q = QR.q_values(w, f32(oo).reshape(E * N, -1), f32(gs).reshape(E * N, 4), f32(orc.landmarks).reshape(E * N, 2))
        top2 = np.sort(q, axis=1)[:, -2:]
        worst = min(worst, float((top2[:, 1] - top2[:, 0] > 1e-4).mean()))
        a = QR.epsilon_greedy(np.argmax(q, axis=1).reshape(E, N), seed, np.arange(E), episode, step, eps)
        *_, done = orc.step(a)
        if done.any():
            pos, vel, lm = _start(cfg, N, E, rng)
            d = done[:, None, None]
            orc.set_state(np.where(d, pos, orc.pos), np.where(d, vel, orc.vel), np.where(d, lm, orc.landmarks),
                          steps=np.where(done, 0, orc.steps), collisions=np.where(done, 0, orc.collisions))
        episode, step = episode + done, np.where(done, 0, step + 1)
    assert episode.min() >= 2                     # max_steps = 5: every env restarted at least twice inside the 12 ticks
    assert worst > 0.9, worst
