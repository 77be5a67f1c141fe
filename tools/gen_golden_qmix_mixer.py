"""TEST INFRASTRUCTURE ONLY (build container) -- golden vectors for the particle QMIX mixer, produced by executing the REFERENCE's own
function body networks.Qmix_mixer (networks.py:640-685) under oracle/tf_numpy_shim.py inside the scope alg_qmix.py builds the target
copy in (variable_scope("Mixer_target"), alg_qmix.py:112-113): weights under the variable names the reference's code creates, the
placeholders' inputs and the output.  Writes tests/golden/qmix_mixer_particle.npz with, per case "n<N>":
  <case>/names               the variable names, sorted
  <case>/w/<name>            each variable (float32, [in][out])
  <case>/in/<argument>       agent_qs [rows, N], state [rows, 4 N], goals_all [rows, 2 N]
  <case>/q_tot               the shim's float32 output [rows, 1]
Weights at the shim's default scale (0.5 / sqrt(fan_in)), states uniform in +-2, goals in +-1, agent_qs in +-5.
Run once where the reference sources are readable: python tools/gen_golden_qmix_mixer.py [output directory]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import tf_numpy_shim as S  # noqa: E402

CASES = ((1, 40), (2, 48), (3, 56), (4, 96), (8, 64), (10, 72))


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
    x = {"agent_qs": u(5, rows, n_agents), "state": u(2, rows, 4 * n_agents), "goals_all": u(1, rows, 2 * n_agents)}
    with shim.variable_scope("Mixer_target"):
        q = net.Qmix_mixer(S._t(x["agent_qs"]), S._t(x["state"]), S._t(x["goals_all"]), 4 * n_agents, 2, n_agents)
    return shim.weights, x, np.asarray(q, dtype=np.float32)


def records():
    rng = np.random.default_rng(20261020)
    rec = {}
    for n, rows in CASES:
        w, inputs, q = mixer_case(rng, n, rows)
        tag = "n%d" % n
        rec[tag + "/names"] = np.array(sorted(w))
        for k, v in w.items():
            rec[tag + "/w/" + k] = v
        for k, v in inputs.items():
            rec[tag + "/in/" + k] = v
        rec[tag + "/q_tot"] = q
    return rec


def main(out_dir=None):
    rec = records()
    for tag in sorted({k.split("/")[0] for k in rec}, key=lambda t: int(t[1:])):
        q = rec[tag + "/q_tot"]
        print(tag, list(rec[tag + "/names"]), q.shape, float(np.abs(q).min()), float(np.abs(q).max()))
    path = os.path.join(out_dir or os.path.join(ROOT, "tests", "golden"), "qmix_mixer_particle.npz")
    np.savez_compressed(path, **rec)
    return path


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
