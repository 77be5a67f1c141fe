"""TEST INFRASTRUCTURE ONLY (build container) -- golden vectors for the CM3 Checkers critics, produced by executing the REFERENCE's
own function bodies networks.Q_global_checkers (networks.py:155-183) and networks.Q_credit_checkers (:244-272) under
oracle/tf_numpy_shim.py inside the scopes alg_credit_checkers.py:120-134 builds them in, at the widths of
config_checkers_stage{1,2}.json (Q_conv_f 4, Q_conv_k [3, 5], f2 6, k2 [3, 3], Q_n_h1_1 256, Q_n_h1_2 32, Q_n_h2 256).  Writes ONE file
per case, tests/golden/critic_checkers_<kind>_n<N>.npz (global_n1 is stage 1, the others stage 2; the weights are ~0.55 MB per case
and do not compress), with
  names               the variable names, sorted
  w/<name>            each variable (float32, TF shapes)
  in/<placeholder>    s_grid [rows, 3, 9, 2] in {0, 1}; s_n, g_n (one-hot), t_obs [rows, 5, 5, 3] in {-1, 0, 1}, v_obs;
                      global: a_n, s_others, a_others ([rows, N-1, 5]); credit: a_m, s_m, s_others
                      (credit row i is the pair n = i % N, m = (i // N) % N of a time step of its own: s_m is the state of agent m
                      among s_n / s_others, see base_state; t_obs and v_obs are then agent m's, global: agent n's)
  q                   the shim's float32 output [rows, 1]
Run once where the reference sources are readable: python tools/gen_golden_critic_checkers.py [output directory]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import tf_numpy_shim as S  # noqa: E402

CASES = (("global", 1, 40), ("global", 2, 48), ("credit", 2, 64), ("global", 8, 56), ("credit", 8, 64))
NN = dict(f1=4, k1=[3, 5], n_h1_1=256, n_h1_2=32, n_h2=256)        # config_checkers_stage{1,2}.json; f2, k2 are the defaults


class Shim(S.Shim):
    """the critics name their sum: tf.add_n(list_mult, name='Q_h2')"""

    @staticmethod
    def add_n(xs, name=None):
        return S.Shim.add_n(xs)


def onehot(rng, shape, width=5):
    return np.eye(width, dtype=np.float32)[rng.integers(0, width, shape)]


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
    x = {"s_grid": rng.integers(0, 2, (rows, 3, 9, 2)).astype(np.float32), "s_n": u(2, rows, 4), "g_n": onehot(rng, rows, 2),
         "t_obs": rng.integers(-1, 2, (rows, 5, 5, 3)).astype(np.float32), "v_obs": u(1, rows, 4)}
    if kind == "global":
        x["a_n"] = onehot(rng, rows)
        x["s_others"] = u(2, rows, 4 * (n_agents - 1))
        x["a_others"] = onehot(rng, (rows, n_agents - 1))
        with shim.variable_scope("Q_global_main"):
            q = net.Q_global_checkers(S._t(x["s_grid"]), S._t(x["s_n"]), S._t(x["g_n"]), S._t(x["a_n"]), S._t(x["s_others"]),
                                      S._t(x["a_others"]), S._t(x["t_obs"]), S._t(x["v_obs"]), stage=1 if n_agents == 1 else 2, **NN)
    else:
        x["a_m"] = onehot(rng, rows)
        x["s_others"] = u(2, rows, 4 * (n_agents - 1))
        x["s_m"] = base_state(x["s_n"], x["s_others"], n_agents)[np.arange(rows), pair_agents(rows, n_agents)[1]]
        with shim.variable_scope("Q_credit_main"):
            q = net.Q_credit_checkers(S._t(x["s_grid"]), S._t(x["s_n"]), S._t(x["g_n"]), S._t(x["a_m"]), S._t(x["s_m"]),
                                      S._t(x["s_others"]), S._t(x["t_obs"]), S._t(x["v_obs"]), stage=2, **NN)
    return shim.weights, x, np.asarray(q, dtype=np.float32)


def records():
    """case tag -> the arrays of its file"""
    rng = np.random.default_rng(20261021)
    out = {}
    for kind, n, rows in CASES:
        w, inputs, q = critic_case(rng, kind, n, rows)
        rec = {"names": np.array(sorted(w)), "q": q}
        for k, v in w.items():
            rec["w/" + k] = v
        for k, v in inputs.items():
            rec["in/" + k] = v
        out["%s_n%d" % (kind, n)] = rec
    return out


def main(out_dir=None):
    out_dir = out_dir or os.path.join(ROOT, "tests", "golden")
    paths = {}
    for tag, rec in records().items():
        print(tag, list(rec["names"]), rec["q"].shape, float(np.abs(rec["q"]).max()))
        paths[tag] = os.path.join(out_dir, "critic_checkers_%s.npz" % tag)
        np.savez_compressed(paths[tag], **rec)
    return paths


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
