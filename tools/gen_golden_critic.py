"""TEST INFRASTRUCTURE ONLY (build container) -- golden vectors for the CM3 particle critics, produced by executing the REFERENCE's own
function bodies networks.Q_global_1output (networks.py:97-122) and networks.Q_credit (:186-211) under oracle/tf_numpy_shim.py inside
the scopes alg_credit.py builds them in: weights under the variable names the reference's code creates, the placeholders' inputs and
the outputs.  Writes tests/golden/critic_particle.npz with, per case "<kind>_n<N>" (global_n1 is stage 1, the others stage 2):
  <case>/names               the variable names, sorted
  <case>/w/<name>            each variable (float32, [in][out] / [out])
  <case>/in/<placeholder>    global: s_n, g_n, a_n, s_others, a_others ([rows, N-1, 5]); credit: s_n, g_n, a_m, s_m, s_others
                             (credit row i is the pair n = i % N, m = (i // N) % N of a time step of its own: s_m is the state of
                             agent m among s_n / s_others, see base_state)
  <case>/q                   the shim's float32 output [rows, 1]
Run once where the reference sources are readable: python tools/gen_golden_critic.py [output directory]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import tf_numpy_shim as S  # noqa: E402

CASES = (("global", 1, 40), ("global", 2, 48), ("credit", 2, 64), ("global", 4, 96), ("credit", 4, 80), ("global", 10, 60),
         ("credit", 10, 72))


class Shim(S.Shim):
    """the critics name their sum: tf.add_n(list_mult, name='Q_h2')"""

    @staticmethod
    def add_n(xs, name=None):
        return S.Shim.add_n(xs)


def onehot(rng, shape):
    return np.eye(5, dtype=np.float32)[rng.integers(0, 5, shape)]


def pair_agents(rows, n_agents):
    """(n, m) of fixture row i: n = i % N, m = (i // N) % N -- every pair, m == n included"""
    i = np.arange(rows)
    return i % n_agents, (i // n_agents) % n_agents


def base_state(s_n, s_others, n_agents):
    """[rows, N, 4]: the time step whose agent n = i % N has s_n and whose other agents, in ascending order, have s_others.  In a
    batch s_m IS the state of agent m of the same time step, so the credit records take s_m from here: a row is then the decoding
    of base columns, which is what the device critic evaluates."""
    rows = s_n.shape[0]
    n = pair_agents(rows, n_agents)[0]
    state = np.zeros((rows, n_agents, 4), np.float32)
    for i in range(rows):
        state[i, n[i]] = s_n[i]
        state[i, [j for j in range(n_agents) if j != n[i]]] = s_others[i].reshape(n_agents - 1, 4)
    return state


def critic_case(rng, kind, n_agents, rows):
    shim = Shim(rng=rng, scale=1.0)
    net = S.load_networks(shim)
    u = lambda lo, *shape: rng.uniform(-lo, lo, shape).astype(np.float32)  # noqa: E731
    x = {"s_n": u(2, rows, 4), "g_n": u(1, rows, 2)}
    if kind == "global":
        x["a_n"] = onehot(rng, rows)
        x["s_others"] = u(2, rows, 4 * (n_agents - 1))
        x["a_others"] = onehot(rng, (rows, n_agents - 1))
        with shim.variable_scope("Q_global_main"):
            q = net.Q_global_1output(S._t(x["s_n"]), S._t(x["g_n"]), S._t(x["a_n"]), S._t(x["s_others"]), S._t(x["a_others"]),
                                     stage=1 if n_agents == 1 else 2)
    else:
        x["a_m"] = onehot(rng, rows)
        x["s_others"] = u(2, rows, 4 * (n_agents - 1))
        x["s_m"] = base_state(x["s_n"], x["s_others"], n_agents)[np.arange(rows), pair_agents(rows, n_agents)[1]]
        with shim.variable_scope("Q_credit_main"):
            q = net.Q_credit(S._t(x["s_n"]), S._t(x["g_n"]), S._t(x["a_m"]), S._t(x["s_m"]), S._t(x["s_others"]), stage=2)
    return shim.weights, x, np.asarray(q, dtype=np.float32)


def records():
    rng = np.random.default_rng(20261020)
    rec = {}
    for kind, n, rows in CASES:
        w, inputs, q = critic_case(rng, kind, n, rows)
        tag = "%s_n%d" % (kind, n)
        rec[tag + "/names"] = np.array(sorted(w))
        for k, v in w.items():
            rec[tag + "/w/" + k] = v
        for k, v in inputs.items():
            rec[tag + "/in/" + k] = v
        rec[tag + "/q"] = q
    return rec


def main(out_dir=None):
    rec = records()
    for tag in sorted({k.split("/")[0] for k in rec}):
        print(tag, list(rec[tag + "/names"]), rec[tag + "/q"].shape, float(np.abs(rec[tag + "/q"]).max()))
    path = os.path.join(out_dir or os.path.join(ROOT, "tests", "golden"), "critic_particle.npz")
    np.savez_compressed(path, **rec)
    return path


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
