"""TEST INFRASTRUCTURE ONLY -- records every feed_dict the REAL reference QMIX train_step builds (build container only).

alg_qmix.Alg.train_step (alg/alg_qmix.py:338-380) is NumPy data movement around four sess.run calls: argmax_Q_target, mixer_target,
mixer_op, list_update_target_ops.  As oracle/gen_golden_trainstep.py does for the CM3 learners, the reference module is imported
with a permissive stub `tensorflow` and train_step is driven on an Alg.__new__ object with a RECORDING stand-in for the session:
placeholders / ops are their own attribute names, argmax_Q_target returns seeded integers in 0..4 of shape [rows], mixer_target
seeded float32 [n_steps, 1] (what a TF session returns), and each call's (ops, feed_dict, result) is stored.  The fixtures pin
cm3_amd.batch.qmix_train_step_feeds and process_batch_qmix bit for bit (tests/test_qmix_train_feeds.py); the eight- and ten-agent
ones make the reference's own np.sum pin the eight-accumulator tree of the TD target's row sum and its tail.

    python tools/gen_golden_qmix_trainstep.py   ->  tests/golden/trainstep_qmix_particle_n{1,4,8,10}.npz
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle.gen_golden_trainstep import REF, particle_cols, save  # noqa: E402

PLACEHOLDERS = ("v_state", "v_goal_all", "actions_1hot", "obs_others", "v_obs", "v_goal", "td_target")
OPS = ("argmax_Q_target", "mixer_target", "mixer_op", "list_update_target_ops")
SOURCES = (("n1", "particle_stage1_greedy.npz", 1), ("n4", "particle_cross_greedy.npz", 4),
           ("n8", "particle_merge8_greedy.npz", 8), ("n10", "particle_ring10_greedy.npz", 10))
GAMMA = 0.99


class RecordingSession(object):
    """sess.run(op, feed_dict) stand-in for the four calls of alg_qmix.train_step."""

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


def main():
    from cm3_amd.rollout import PARTICLE_ORDER, rows_from_columns        # torch BEFORE the tensorflow stub

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
    import alg_qmix
    out = os.path.join(ROOT, "tests", "golden")
    for tag, fixture, N in SOURCES:
        cols = particle_cols(fixture, 1, N)
        T = len(cols["actions"])
        alg = alg_qmix.Alg.__new__(alg_qmix.Alg)
        for name in PLACEHOLDERS + OPS:
            setattr(alg, name, name)
        alg.list_update_target_ops = ["list_update_target_ops"]          # (sess.run takes the LIST of assign ops, :380)
        alg.n_agents, alg.l_action, alg.gamma, alg.experiment = N, 5, GAMMA, "particle"
        alg.l_obs_others, alg.l_obs, alg.l_goal = 4 * max(N - 1, 1), 4, 2
        alg.l_state_one_agent, alg.l_state = 4, 4 * N
        sess = RecordingSession(T, N, seed=40 + N)
        alg.train_step(sess, rows_from_columns(cols, PARTICLE_ORDER), 0.25, 7, summarize=False, writer=None)
        save(os.path.join(out, "trainstep_qmix_particle_%s.npz" % tag), cols, sess, dict(n_agents=N, gamma=GAMMA, env="particle"))


if __name__ == "__main__":
    main()
