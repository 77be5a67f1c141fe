"""TEST INFRASTRUCTURE ONLY -- float64 restatement of the QMIX baseline's agent network and of the device agent's epsilon-greedy
choice (the QMIX counterpart of oracle/actor_oracle.py; test helper, not a test module).

  networks.Qmix_single_particle   alg/networks.py:581-594
      concat(o_others[L], o_self[4], goal[2]) -> dense 64 relu ("h") -> dense 64 relu ("h2") -> dense 5 ("out")
  alg_qmix.Alg.run_actor          alg/alg_qmix.py:160-184
      per agent: with probability epsilon a uniform action, else argmax Q (tf.argmax: the first index on ties)

The exploration draws are the build's own (csrc/actor.hip, kPurposeExplore): per (seed, global env id, episode, step, agent)
one Philox4x32-10 block over (env id lo, env id hi, 0, 0x20000000 | (agent >> 1) << 24), words 2 (agent & 1) and
2 (agent & 1) + 1 mixed with the episode / step counters (philox.action_word); explore iff u01(first) < epsilon (in double),
the uniform action is rand5(second).
"""
import numpy as np

from oracle import philox

PURPOSE_EXPLORE = 0x20000000
NAMES = ("h/kernel", "h/bias", "h2/kernel", "h2/bias", "out/kernel", "out/bias")


def canon(name):
    name = name.split(":")[0]
    for prefix in ("Agent_main/", "Agent_target/"):
        if name.startswith(prefix):
            name = name[len(prefix):]
    return name


def init_weights(rng, n_agents, scale=0.5):
    """Random weights under the reference's variable names (Agent_main scope, alg_qmix.py:87-96)."""
    k = 4 * max(n_agents - 1, 1) + 6
    f = lambda *shape: (rng.standard_normal(shape) * scale / np.sqrt(shape[0] if len(shape) > 1 else 4)).astype(np.float32)  # noqa: E731
    return {"Agent_main/h/kernel": f(k, 64), "Agent_main/h/bias": f(64), "Agent_main/h2/kernel": f(64, 64),
            "Agent_main/h2/bias": f(64), "Agent_main/out/kernel": f(64, 5), "Agent_main/out/bias": f(5)}


def q_values(w, obs_others, v_obs, v_goal, dtype=np.float64):
    """Q [rows, 5]: the network in `dtype` (float64: the reference the device agent is measured against)."""
    w = {canon(k): v for k, v in w.items()}
    f = np.dtype(dtype).type
    W = lambda k: np.asarray(w[k], dtype=f)  # noqa: E731
    x = np.concatenate([obs_others, v_obs, v_goal], axis=1).astype(f)
    h = np.maximum(x @ W("h/kernel") + W("h/bias"), f(0))
    h = np.maximum(h @ W("h2/kernel") + W("h2/bias"), f(0))
    return h @ W("out/kernel") + W("out/bias")


def explore_words(seed, env_ids, episode, step, n_agents):
    """(explore word, action word) uint32 [E, N] of (env, episode, step): see the module docstring."""
    env_ids = np.asarray(env_ids)
    lo, hi = philox._split(env_ids)
    we = np.zeros((env_ids.shape[0], n_agents), np.uint32)
    wa = np.zeros_like(we)
    for i in range(n_agents):
        c3 = np.uint64(PURPOSE_EXPLORE | ((i >> 1) << 24))
        b = philox.philox4x32_10(lo, hi, np.uint64(0), c3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        q = 2 * (i & 1)
        we[:, i] = philox.action_word(b[q], episode, step)
        wa[:, i] = philox.action_word(b[q + 1], episode, step)
    return we, wa


def epsilon_greedy(greedy, seed, env_ids, episode, step, epsilon):
    """int64 [E, N]: the device agent's choice given its greedy actions [E, N]."""
    greedy = np.asarray(greedy)
    we, wa = explore_words(seed, env_ids, episode, step, greedy.shape[1])
    explore = philox.u01(we) < float(np.float32(epsilon))
    return np.where(explore, philox.rand5(wa), greedy)
