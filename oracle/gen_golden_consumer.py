"""TEST INFRASTRUCTURE ONLY -- records what the REAL reference batch reshapers return when they consume the exporter's rows
(build container only; tests/test_reference_consumer.py checks against the record).

Imports alg/alg_credit.py and alg/alg_credit_checkers.py from the reference tree with a permissive stub `tensorflow` (TF1 is not
installed; only the pure-NumPy methods run), packs one recorded episode of each env with cm3_amd.rollout.rows_from_columns and
stores what process_batch (alg_credit.py:445-499, alg_credit_checkers.py:414-470), process_goals and process_global_state return.

    python oracle/gen_golden_consumer.py  ->  tests/golden/reference_consumer.npz
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
REF = os.environ.get("CM3_REFERENCE_ROOT", "/root/reference")

PARTICLE_FIXTURE, CHECKERS_FIXTURE, EPISODE = "particle_antipodal_greedy", "checkers_stage2_uniform", 0


def _import_alg(name):
    if "tensorflow" not in sys.modules:
        class _Any(types.ModuleType):
            def __getattr__(self, k):
                return _Any(k)

            def __call__(self, *a, **k):
                return _Any("call")
        sys.modules["tensorflow"] = _Any("tensorflow")
    sys.dont_write_bytecode = True
    p = os.path.join(REF, "alg")
    if p not in sys.path:
        sys.path.insert(0, p)
    if not hasattr(np, "int"):
        np.int = int
    return __import__(name)


def particle():
    from cm3_amd.rollout import PARTICLE_ORDER, rows_from_columns
    from tests.helpers import load_golden, particle_transition_columns
    alg_credit = _import_alg("alg_credit")
    cols, T, N = particle_transition_columns(load_golden(PARTICLE_FIXTURE), EPISODE)
    alg = alg_credit.Alg.__new__(alg_credit.Alg)
    alg.n_agents, alg.l_action, alg.experiment = N, 5, "particle"
    alg.l_obs_others, alg.l_obs, alg.l_goal = 4 * (N - 1), 4, 2
    alg.l_state_one_agent, alg.l_state = 4, 4 * N
    out = alg.process_batch(rows_from_columns(cols, PARTICLE_ORDER))
    rec = {"particle/pb_%02d" % i: np.asarray(v) for i, v in enumerate(out)}
    gself, gothers = alg.process_goals(out[12], out[0])
    one, others, state = alg.process_global_state(out[1], out[0])
    rec.update({"particle/goals_self": gself, "particle/goals_others": gothers, "particle/gs_one": one,
                "particle/gs_others": others, "particle/gs_state": state})
    return rec


def checkers():
    from cm3_amd.rollout import CHECKERS_ORDER, rows_from_columns
    from tests.helpers import checkers_transition_columns, load_golden
    mod = _import_alg("alg_credit_checkers")
    g = load_golden(CHECKERS_FIXTURE)
    cols, T, N = checkers_transition_columns(g, EPISODE)
    alg = mod.Alg.__new__(mod.Alg)
    d = g["meta"]["config"]["dimensions"]
    alg.n_agents, alg.l_action, alg.experiment = N, d["l_action"], "checkers"
    for k, v in d.items():
        setattr(alg, k, v)
    alg.l_obs_others, alg.l_obs_self, alg.l_goal = d["l_obs_others"], d["l_obs_self"], d["l_goal"]
    alg.rows_obs, alg.columns_obs, alg.channels_obs = d["rows_obs"], d["columns_obs"], d["channels_obs"]
    alg.l_state_one_agent = d["l_state_one"]
    out = alg.process_batch(rows_from_columns(cols, CHECKERS_ORDER))
    # (only the arrays: what else process_batch returns is not an array of the batch)
    return {"checkers/pb_%02d" % i: v for i, v in enumerate(out) if i == 0 or isinstance(v, np.ndarray)}


def main():
    import cm3_amd.rollout  # noqa: F401  (imports torch BEFORE the tensorflow stub exists)
    rec = particle()
    rec.update(checkers())
    rec = {k: np.asarray(v) for k, v in rec.items()}
    path = os.path.join(ROOT, "tests", "golden", "reference_consumer.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, {k: (v.shape, str(v.dtype)) for k, v in rec.items()})


if __name__ == "__main__":
    main()
