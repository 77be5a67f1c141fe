"""TEST INFRASTRUCTURE ONLY (build container) -- golden vectors for the Checkers QMIX mixer, produced by executing the REFERENCE's own
function body networks.Qmix_mixer_checkers (networks.py:688-734) under oracle/tf_numpy_shim.py inside the scope alg_qmix_checkers.py
builds the target copy in (variable_scope("Mixer_target"), alg_qmix_checkers.py:105-106) at Q_conv_f 4, Q_conv_k [3, 5]
(config_checkers_stage{1,2}.json): weights under the variable names the reference's code creates, the placeholders' inputs and the
output.  Writes ONE file per case, tests/golden/qmix_mixer_checkers_n<N>.npz (N = 1, 2, 3, 5; at N = 8 the weights alone pass the size
of the largest committed fixture, so that count is covered by the float64 restatement only), each with
  names               the variable names, sorted
  w/<name>            each variable (float32, as TensorFlow shapes it)
  in/<argument>       agent_qs [rows, N], state_env [rows, 3, 9, 2], state [rows, 4 N], goals_all [rows, 2 N]
  q_tot               the shim's float32 output [rows, 1]
Weights at the shim's default scale (0.5 / sqrt(shape[0])), grids in {0, 1}, states uniform in +-2, one-hot goals, agent_qs in +-5.
Run once where the reference sources are readable: python tools/gen_golden_qmix_mixer_checkers.py [output directory]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import tf_numpy_shim as S  # noqa: E402

CASES = ((1, 40), (2, 48), (3, 56), (5, 67))


class Shim(S.Shim):
    """the mixer takes absolute values of its hyper-network's outputs and an ELU: tf.abs, tf.nn.elu (float32, like the rest)"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.nn.elu = self._elu

    @staticmethod
    def abs(x, name=None):
        return S._t(np.abs(x))

    @staticmethod
    def _elu(x, name=None):
        x = np.asarray(x, np.float32)
        return S._t(np.where(x > 0, x, np.expm1(np.minimum(x, np.float32(0)))))


def mixer_case(rng, n_agents, rows):
    shim = Shim(rng=rng)
    net = S.load_networks(shim)
    u = lambda lo, *shape: rng.uniform(-lo, lo, shape).astype(np.float32)  # noqa: E731
    x = {"agent_qs": u(5, rows, n_agents), "state_env": rng.integers(0, 2, (rows, 3, 9, 2)).astype(np.float32),
         "state": u(2, rows, 4 * n_agents),
         "goals_all": np.eye(2, dtype=np.float32)[rng.integers(0, 2, (rows, n_agents))].reshape(rows, 2 * n_agents)}
    with shim.variable_scope("Mixer_target"):
        q = net.Qmix_mixer_checkers(S._t(x["agent_qs"]), S._t(x["state_env"]), S._t(x["state"]), S._t(x["goals_all"]), 4 * n_agents, 2,
                                    n_agents, f1=4, k1=[3, 5])
    return shim.weights, x, np.asarray(q, dtype=np.float32)


def records():
    """{N: the arrays of that case's file}"""
    rng = np.random.default_rng(20261021)
    out = {}
    for n, rows in CASES:
        w, inputs, q = mixer_case(rng, n, rows)
        rec = {"names": np.array(sorted(w))}
        for k, v in w.items():
            rec["w/" + k] = v
        for k, v in inputs.items():
            rec["in/" + k] = v
        rec["q_tot"] = q
        out[n] = rec
    return out


def main(out_dir=None):
    paths = []
    for n, rec in records().items():
        q = rec["q_tot"]
        print("n%d" % n, list(rec["names"]), q.shape, float(np.abs(q).min()), float(np.abs(q).max()))
        path = os.path.join(out_dir or os.path.join(ROOT, "tests", "golden"), "qmix_mixer_checkers_n%d.npz" % n)
        np.savez_compressed(path, **rec)
        paths.append(path)
    return paths


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
