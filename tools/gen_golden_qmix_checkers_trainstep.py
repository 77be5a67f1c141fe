"""TEST INFRASTRUCTURE ONLY -- records every feed_dict the REAL reference Checkers QMIX train_step builds (build container only).

alg_qmix_checkers.Alg.train_step (alg/alg_qmix_checkers.py:342-393) is NumPy data movement around four sess.run calls:
argmax_Q_target, mixer_target, mixer_op, list_update_target_ops.  As tools/gen_golden_qmix_trainstep.py does for the particle env,
the reference module is imported with a permissive stub `tensorflow` and train_step is driven on an Alg.__new__ object with a
RECORDING stand-in for the session: placeholders / ops are their own attribute names, argmax_Q_target returns seeded int64 [T * N]
in 0..4, mixer_target seeded float32 [T, 1] (what a TF session returns), and each call's (ops, feed_dict, result) is stored.  The
fixtures pin cm3_amd.batch.qmix_train_step_feeds(env="checkers") and process_batch_qmix_checkers bit for bit
(tests/test_qmix_checkers_train_feeds.py).  n1 / n2 come from episode 1 of the recorded Checkers fixtures; n4 from seeded synthetic
columns of the same shapes, so that an agent count above two pins the row order.

    python tools/gen_golden_qmix_checkers_trainstep.py   ->  tests/golden/trainstep_qmix_checkers_n{1,2,4}.npz
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle.gen_golden_trainstep import REF, checkers_cols, save  # noqa: E402

PLACEHOLDERS = ("state_env", "v_state", "v_goal_all", "actions_1hot", "actions_prev", "obs_others", "obs_self_t", "obs_self_v",
                "v_goal", "td_target")
OPS = ("argmax_Q_target", "mixer_target", "mixer_op", "list_update_target_ops")
SOURCES = (("n1", "checkers_stage1_uniform.npz", 1), ("n2", "checkers_stage2_uniform.npz", 2))
GAMMA = 0.99


class RecordingSession(object):
    """sess.run(op, feed_dict) stand-in for the four calls of alg_qmix_checkers.train_step."""

    def __init__(self, n_steps, n_agents, seed):
        self.calls = []
        self.rng = np.random.default_rng(seed)
        self.n_steps, self.n = n_steps, n_agents

    def _one(self, op):
        if op == "argmax_Q_target":
            return self.rng.integers(0, 5, self.n_steps * self.n)                                  # tf.argmax: int64 [rows]
        if op == "mixer_target":
            return self.rng.standard_normal((self.n_steps, 1)).astype(np.float32)                  # Q_tot: float32 [n_steps, 1]
        return None

    def run(self, ops, feed_dict=None):
        many = isinstance(ops, (list, tuple))
        names = list(ops) if many else [ops]
        res = [self._one(op) for op in names]
        self.calls.append((names, dict(feed_dict or {}), res))
        return res if many else res[0]


def synthetic_cols(T, N, seed):
    """Columns shaped like checkers_cols() for N agents (3 x 8 band + border: grid [3, 9, 2]; Lo = 2 (N - 1)), seeded."""
    rng = np.random.default_rng(seed)
    Lo = 2 * max(N - 1, 1)
    grid = rng.integers(0, 2, (T + 1, 3, 9, 2)).astype(np.float64)
    vec = rng.uniform(-0.5, 1.0, (T + 1, N, 4))
    oo = rng.uniform(-1.0, 1.0, (T + 1, N, Lo))
    ot = rng.integers(-1, 2, (T + 1, N, 5, 5, 3)).astype(np.float64)
    ov = rng.uniform(-0.5, 1.0, (T + 1, N, 4))
    acts = rng.integers(0, 5, (T, N))
    prev = np.concatenate([np.zeros((1, N), acts.dtype), acts[:-1]])
    done = np.zeros(T, dtype=bool)
    done[-1] = True
    return dict(grid=grid[:-1], vec=vec[:-1], obs_others=oo[:-1], obs_self_t=ot[:-1], obs_self_v=ov[:-1], actions_prev=prev,
                actions=acts, reward=rng.standard_normal(T), local_rewards=rng.standard_normal((T, N)), next_grid=grid[1:],
                next_vec=vec[1:], next_obs_others=oo[1:], next_obs_self_t=ot[1:], next_obs_self_v=ov[1:], done=done,
                goals=np.eye(2)[rng.integers(0, 2, N)][None].repeat(T, axis=0).astype(float))


def main():
    from cm3_amd.rollout import CHECKERS_ORDER, rows_from_columns        # torch BEFORE the tensorflow stub

    class _Any(types.ModuleType):
        def __getattr__(self, k):
            return _Any(k)

        def __call__(self, *a, **k):
            return _Any("call")
    sys.modules.setdefault("tensorflow", _Any("tensorflow"))
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(REF, "alg"))
    if not hasattr(np, "int"):
        np.int = int
    import alg_qmix_checkers
    out = os.path.join(ROOT, "tests", "golden")
    batches = [(tag, checkers_cols(fixture, 1, N)[0], N) for tag, fixture, N in SOURCES]
    batches.append(("n4", synthetic_cols(10, 4, seed=404), 4))
    for tag, cols, N in batches:
        T = len(cols["actions"])
        alg = alg_qmix_checkers.Alg.__new__(alg_qmix_checkers.Alg)
        for name in PLACEHOLDERS + OPS:
            setattr(alg, name, name)
        alg.list_update_target_ops = ["list_update_target_ops"]          # (sess.run takes the LIST of assign ops, :393)
        alg.n_agents, alg.l_action, alg.gamma, alg.experiment = N, 5, GAMMA, "checkers"
        alg.l_obs_others, alg.l_obs_self, alg.l_goal = 2 * max(N - 1, 1), 4, 2
        alg.rows_obs, alg.columns_obs, alg.channels_obs = 5, 5, 3
        alg.l_state_one_agent, alg.l_state = 4, 4 * N
        sess = RecordingSession(T, N, seed=60 + N)
        alg.train_step(sess, rows_from_columns({k: np.array(v) for k, v in cols.items()}, CHECKERS_ORDER), 0.25, 7,
                       summarize=False, writer=None)
        save(os.path.join(out, "trainstep_qmix_checkers_%s.npz" % tag), cols, sess, dict(n_agents=N, gamma=GAMMA, env="checkers"))


if __name__ == "__main__":
    main()
