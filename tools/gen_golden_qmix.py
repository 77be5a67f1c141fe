"""TEST INFRASTRUCTURE ONLY (build container) -- golden vectors for the QMIX baseline's agent network, produced by executing the
REFERENCE's own function body networks.Qmix_single_particle (networks.py:581-594) under oracle/tf_numpy_shim.py inside the
"Agent_main" scope alg_qmix.py:87-96 builds it in: weights under the variable names the reference's code creates, inputs, the
Q values and tf.argmax of them (alg_qmix.py:98).  Writes tests/golden/qmix_particle.npz with, per case "n<N>":
  n<N>/names                 the variable names, sorted
  n<N>/w/<name>              each variable (float32, [in][out] / [out])
  n<N>/in/{obs_others, v_obs, v_goal}
  n<N>/q, n<N>/argmax        the shim's float32 Q values [rows, 5] and their argmax (the first index on ties)
Run once where the reference sources are readable: python tools/gen_golden_qmix.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import tf_numpy_shim as S  # noqa: E402


def qmix_case(rng, n_agents, rows):
    shim = S.Shim(rng=rng, scale=1.0)
    net = S.load_networks(shim)
    lo = 4 * max(n_agents - 1, 1)
    oo = rng.uniform(-2, 2, (rows, lo)).astype(np.float32)
    vo = rng.uniform(-1.5, 1.5, (rows, 4)).astype(np.float32)
    vg = rng.uniform(-1, 1, (rows, 2)).astype(np.float32)
    with shim.variable_scope("Agent_main"):
        q = np.asarray(net.Qmix_single_particle(S._t(oo), S._t(vo), S._t(vg)), dtype=np.float32)
    return shim.weights, dict(obs_others=oo, v_obs=vo, v_goal=vg), q


def main():
    rng = np.random.default_rng(20261016)
    rec = {}
    for n, rows in ((1, 40), (4, 96), (8, 64), (10, 80)):
        w, inputs, q = qmix_case(rng, n, rows)
        tag = "n%d" % n
        rec[tag + "/names"] = np.array(sorted(w))
        for k, v in w.items():
            rec[tag + "/w/" + k] = v
        for k, v in inputs.items():
            rec[tag + "/in/" + k] = v
        rec[tag + "/q"] = q
        rec[tag + "/argmax"] = np.argmax(q, axis=1).astype(np.int64)
        print(tag, sorted(w), q.shape, float(np.ptp(q, axis=1).mean()), np.bincount(rec[tag + "/argmax"], minlength=5))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "qmix_particle.npz"), **rec)


if __name__ == "__main__":
    main()
