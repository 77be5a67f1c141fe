"""CPU: the C ABI of the Checkers QMIX agent's one-launch rollout (cm3_policy_rollout_checkers_qmix, additive part of ABI 9) --
declared, exported, bound with the argument list of cm3_policy_rollout_checkers, and invalid arguments refused with a readable
error before anything touches a GPU.  Also here, because it needs no GPU: the float64 restatement driven by its own choices keeps
the share of clearly decided rows that tests/test_gpu_qmix_checkers_rollout.py asks of every tick."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, TWIN = "cm3_policy_rollout_checkers_qmix", "cm3_policy_rollout_checkers"
FAKE = 0x1000                                   # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    return _lib


def _declared_args(text, name):
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_entry(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cm3_amd.h")).read(), flags=re.S)
    handle = built.lib()
    assert hasattr(handle, ENTRY) and ENTRY in built.SYMBOLS
    args, twin = _declared_args(text, ENTRY), _declared_args(text, TWIN)
    assert len(args) == len(twin) == 12
    res, bound = built.SYMBOLS[ENTRY]
    assert res is ctypes.c_int and len(bound) == len(args)
    assert bound == built.SYMBOLS[TWIN][1]                                # the argument list of the actor's entry point
    assert [re.sub(r"\w+$", "", a).strip() for a in args] == [re.sub(r"\w+$", "", a).strip() for a in twin]   # the same C types
    assert built.ABI_VERSION == 9 and handle.cm3_abi_version() == 9


def _env_desc(built, **kw):
    d = built.CheckersDesc()
    d.n_envs, d.n_agents, d.n_rows, d.n_columns, d.n_obs, d.max_steps = 16, 2, 3, 8, 2, 33
    d.grid_stride, d.obs_self_t_stride = 56, 152
    d.agents_r[0], d.agents_c[0], d.agents_r[1], d.agents_c[1] = 0, 8, 2, 8
    d.seed = 7
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _agent_desc(built, **kw):
    d = built.ActorCheckersDesc()
    d.n_envs, d.n_agents, d.stage, d.n_obs = 16, 2, 2, 2
    d.conv_f, d.n_conv_linear, d.n_h1, d.n_h2, d.n_actions = 6, 32, 256, 256, 5
    d.epsilon, d.precision = 0.1, 2
    d.obs_self_t_stride = 152
    d.seed = 7
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _filled(cls, **kw):
    x = cls()
    for name, ctype in x._fields_:
        if ctype is ctypes.c_void_p:
            setattr(x, name, FAKE)
    for k, v in kw.items():
        setattr(x, k, v)
    return x


def _call(built, env=None, agent=None, traj=None, weights=None, n_ticks=4, null=()):
    handle = built.lib()
    args = dict(env=_env_desc(built) if env is None else env, traj=_filled(built.CheckersTraj) if traj is None else traj,
                agent=_agent_desc(built) if agent is None else agent,
                weights=_filled(built.ActorCheckersWeights) if weights is None else weights)
    ref = {k: (None if k in null else ctypes.byref(v)) for k, v in args.items()}
    rc = handle.cm3_policy_rollout_checkers_qmix(ref["env"], ref["traj"], ref["agent"], ref["weights"], None, None, None, 0, None, None,
                                                 n_ticks, None)
    return rc, handle.cm3_last_error()


@pytest.mark.parametrize("null", ["env", "traj", "agent", "weights"])
def test_null_arguments_are_refused(built, null):
    rc, msg = _call(built, null=(null,))
    assert rc == -1 and b"null" in msg, msg


def test_invalid_arguments_are_refused_without_a_gpu(built):
    rc, msg = _call(built, n_ticks=0)
    assert rc == -1 and b"n_ticks" in msg, msg
    rc, msg = _call(built, env=_env_desc(built, n_agents=3), agent=_agent_desc(built, n_agents=3))
    assert rc == -1 and b"one or two agents" in msg and b"cm3_qmix_checkers_f32" in msg, msg
    rc, msg = _call(built, agent=_agent_desc(built, precision=0))
    assert rc == -1 and b"precision" in msg and b"launch-pair" in msg, msg
    rc, msg = _call(built, agent=_agent_desc(built, precision=1))
    assert rc == -1 and b"precision" in msg, msg
    rc, msg = _call(built, agent=_agent_desc(built, n_h1=64))
    assert rc == -1 and b"widths" in msg, msg
    rc, msg = _call(built, agent=_agent_desc(built, n_envs=8))
    assert rc == -1 and b"disagree" in msg, msg
    rc, msg = _call(built, agent=_agent_desc(built, seed=8))
    assert rc == -1 and b"seed" in msg and b"env_id_base" in msg, msg
    rc, msg = _call(built, agent=_agent_desc(built, env_id_base=16))
    assert rc == -1 and b"env_id_base" in msg, msg
    rc, msg = _call(built, agent=_agent_desc(built, epsilon=1.5))
    assert rc == -1 and b"epsilon" in msg, msg
    rc, msg = _call(built, weights=_filled(built.ActorCheckersWeights, packed=None))
    assert rc == -1 and b"cm3_qmix_checkers_pack" in msg, msg
    rc, msg = _call(built, traj=_filled(built.CheckersTraj, actions=None))
    assert rc == -1 and b"action slot" in msg, msg
    # desc->stage is not read: a stage-1 descriptor with two agents passes the agent checks (the actor's entry point refuses it)
    rc, msg = _call(built, agent=_agent_desc(built, stage=1), weights=_filled(built.ActorCheckersWeights, packed=None))
    assert rc == -1 and b"packed" in msg, msg


def test_agent_hooks_do_not_flip_policy_mode_auto():
    """"auto" picks the one-launch kernel for a policy that has enqueue_rollout: the QMIX agent's opt-in hooks carry other names."""
    from cm3_amd.actor import CheckersActor
    from cm3_amd.qmix import CheckersQmixAgent
    assert hasattr(CheckersQmixAgent, "enqueue_episode") and hasattr(CheckersQmixAgent, "episode_ok")
    assert not hasattr(CheckersQmixAgent, "enqueue_rollout") and hasattr(CheckersActor, "enqueue_rollout")


@pytest.mark.parametrize("N", [1, 2])
def test_restatement_alone_decides_nine_rows_in_ten(N):
    """The weights, sizes and episode length of the teacher-forced GPU test (E = 128, T = 33, max_steps = 12, epsilon 0.3,
    continuous collection): the float64 restatement + the oracle env, driven by the restatement's own epsilon-greedy choices,
    with finished envs restarted as the device env restarts them (episode + 1, step 0, actions_prev zeros, a fresh random goal
    at N = 1), leave more than 0.9 of every tick's rows with top-two Q values 1e-4 apart.  (The host draws its own goals and
    exploration words: the same law as the device run, not the same states.)"""
    from oracle.checkers_oracle import VecCheckersOracle
    from tests import qmix_checkers_ref as QC
    from tests.helpers import load_cfg
    E, T, eps, seed, S = 128, 33, 0.3, 53, 12
    rows = E * N
    w = QC.init_weights(np.random.default_rng(200 + N), N)
    i = load_cfg("checkers_stage%d.json" % N)["init"]
    orc = VecCheckersOracle(i["n_rows"], i["n_columns"], i["n_obs"], i["agents_r"], i["agents_c"], N, S, E)
    rng = np.random.default_rng(2)
    goals = np.eye(2)[rng.integers(0, 2, (E, N))] if N == 1 else np.broadcast_to(np.eye(N), (E, N, 2)).copy()
    grid, vec, oo, ot, ov = orc.reset(goals)
    prev = np.zeros((E, N), np.int64)
    episode, step = np.ones(E, np.int64), np.zeros(E, np.int64)
    worst, restarts = 1.0, np.zeros(E, np.int64)
    for t in range(T):
        q = QC.q_values(w, prev.reshape(rows), np.asarray(ot, np.float64).reshape(rows, 5, 5, 3), np.asarray(ov).reshape(rows, 4),
                        np.asarray(oo).reshape(rows, -1), np.eye(2)[orc.goal.reshape(rows)])
        top2 = np.sort(q, axis=1)[:, -2:]
        worst = min(worst, float((top2[:, 1] - top2[:, 0] > 1e-4).mean()))
        a = QC.epsilon_greedy(np.argmax(q, axis=1).reshape(E, N), seed, np.arange(E), episode, step, eps)
        grid, vec, oo, ot, ov, _, _, done = orc.step(a)
        if done.any():
            fresh = rng.integers(0, 2, (E, N)) if N == 1 else orc.goal
            grid, vec, oo, ot, ov = orc.reset_envs(done, fresh)
        prev = np.where(done[:, None], 0, a)
        episode, step, restarts = episode + done, np.where(done, 0, step + 1), restarts + done
    assert restarts.min() >= 2
    assert worst > 0.9, worst
