"""TEST INFRASTRUCTURE ONLY (build container) -- golden vectors for the QMIX baseline's Checkers agent network, produced by executing
the REFERENCE's own function body networks.Qmix_single_checkers (networks.py:617-637) under oracle/tf_numpy_shim.py inside the
"Agent_main" scope alg_qmix_checkers.py:84-88 builds it in, with the actor's nn block (f1 = 6, k1 = [3, 3], n_h1 = n_h2 = 256):
weights under the variable names the reference's code creates, inputs, the Q values and tf.argmax of them (alg_qmix_checkers.py:90).
Both cases share one set of weights (v_obs_others has 2 values at N = 1 and at N = 2, so every variable has the same shape; two
sets of the two 256 x 256 matrices would not fit the size limit of a committed file).  Writes tests/golden/qmix_checkers.npz with
  names                      the variable names, sorted (thirteen: the others branch exists at every N)
  w/<name>                   each variable (float32, TF shapes)
and per case "n<N>":
  n<N>/in/{a_prev, obs_self_t, obs_self_v, obs_others, goals}
                             a_prev int [rows], obs_self_t [rows, 5, 5, 3] in {-1, 0, 1}, obs_self_v [rows, 4],
                             obs_others [rows, 2 max(N-1, 1)], goals one-hot [rows, 2]
  n<N>/q, n<N>/argmax        the shim's float32 Q values [rows, 5] and their argmax (the first index on ties)
Run once where the reference sources are readable: python tools/gen_golden_qmix_checkers.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import tf_numpy_shim as S  # noqa: E402


def qmix_checkers_case(rng, n_agents, rows, weight_seed):
    shim = S.Shim(rng=np.random.default_rng(weight_seed), scale=1.0)
    net = S.load_networks(shim)
    lo = 2 * max(n_agents - 1, 1)
    a_prev = rng.integers(0, 5, rows)
    a1 = np.eye(5, dtype=np.float32)[a_prev]
    t = rng.integers(-1, 2, (rows, 5, 5, 3)).astype(np.float32)
    v = rng.uniform(-0.5, 1.0, (rows, 4)).astype(np.float32)
    oo = rng.uniform(-0.5, 0.5, (rows, lo)).astype(np.float32)
    g = np.eye(2, dtype=np.float32)[rng.integers(0, 2, rows)]
    with shim.variable_scope("Agent_main"):
        q = net.Qmix_single_checkers(S._t(a1), S._t(t), S._t(v), S._t(oo), S._t(g), f1=6, k1=[3, 3], n_h1=256, n_h2=256,
                                     n_actions=5)
    q = np.asarray(q, dtype=np.float32)
    return shim.weights, dict(a_prev=a_prev, obs_self_t=t, obs_self_v=v, obs_others=oo, goals=g), q


def main():
    rng = np.random.default_rng(20261017)
    rec = {}
    for n, rows in ((1, 40), (2, 96)):
        w, inputs, q = qmix_checkers_case(rng, n, rows, weight_seed=20261018)
        tag = "n%d" % n
        if "names" in rec:
            assert list(rec["names"]) == sorted(w) and all(np.array_equal(rec["w/" + k], v) for k, v in w.items())
        rec["names"] = np.array(sorted(w))
        for k, v in w.items():
            rec["w/" + k] = v
        for k, v in inputs.items():
            rec[tag + "/in/" + k] = v
        rec[tag + "/q"] = q
        rec[tag + "/argmax"] = np.argmax(q, axis=1).astype(np.int64)
        print(tag, sorted(w), q.shape, float(np.ptp(q, axis=1).mean()), np.bincount(rec[tag + "/argmax"], minlength=5))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "qmix_checkers.npz"), **rec)


if __name__ == "__main__":
    main()
