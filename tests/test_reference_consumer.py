"""CPU: the REAL alg_credit.process_batch / alg_credit_checkers.process_batch (alg_credit.py:445-499,
alg_credit_checkers.py:414-470) consume the exporter's rows unchanged.

The transition columns are taken from the golden vectors, packed by cm3_amd.rollout.rows_from_columns exactly as
ParticleRollout.as_reference_rows / CheckersRollout.as_reference_rows pack device trajectories.  What the reference's methods
returned for these rows was recorded by oracle/gen_golden_consumer.py (tests/golden/reference_consumer.npz); process_batch
reads field k of the rows as np.stack(rows[:, k]), which is checked here on the rows packed now."""
import os

import numpy as np

from cm3_amd.rollout import CHECKERS_ORDER, PARTICLE_ORDER, rows_from_columns
from tests.helpers import GOLDEN, checkers_transition_columns, load_golden, particle_transition_columns


def _recorded(prefix):
    z = np.load(os.path.join(GOLDEN, "reference_consumer.npz"))
    return {k[len(prefix) + 1:]: z[k] for k in z.files if k.startswith(prefix + "/")}


def _fields_read_back(rows, cols, order):
    """What the reference's process_batch stacks out of each field of the rows is the exported column."""
    assert rows.shape == (len(cols[order[0]]), len(order))
    for k, name in enumerate(order):
        got = np.stack(rows[:, k])
        assert got.dtype == cols[name].dtype and np.array_equal(got, cols[name]), name


def test_real_particle_process_batch_consumes_rows():
    cols, T, N = particle_transition_columns(load_golden("particle_antipodal_greedy"), 0)
    rows = rows_from_columns(cols, PARTICLE_ORDER)
    _fields_read_back(rows, cols, PARTICLE_ORDER)
    rec = _recorded("particle")
    out = [rec["pb_%02d" % i] for i in range(13)]
    (n_steps, v_global, obs_others, v_local, a_1hot, a_others_1hot, reward, reward_local, v_global_next,
     obs_others_next, v_local_next, done, goals) = out
    assert n_steps == T
    assert np.array_equal(v_global, cols["v_global"]) and np.array_equal(v_global_next, cols["v_global_next"])
    assert np.array_equal(obs_others, cols["obs_others"].reshape(T * N, -1))
    assert np.array_equal(v_local, cols["v_local"].reshape(T * N, 4))
    assert np.array_equal(reward, np.repeat(cols["reward"], N))
    assert np.array_equal(reward_local, cols["reward_local"].reshape(-1))
    assert np.array_equal(done, np.repeat(cols["done"], N))
    assert np.array_equal(goals, cols["goals"])
    assert a_1hot.shape == (T * N, 5) and a_others_1hot.shape == (T * N, N - 1, 5)
    assert np.array_equal(a_1hot.argmax(1), cols["actions"].reshape(-1))
    gself, gothers = rec["goals_self"], rec["goals_others"]
    assert gself.shape == (T * N, 2) and gothers.shape == (T * N, (N - 1) * 2)
    others, state = rec["gs_others"], rec["gs_state"]
    assert state.shape == (T * N, 4 * N) and others.shape == (T * N, (N - 1) * 4)


def test_real_checkers_process_batch_consumes_rows():
    cols, T, N = checkers_transition_columns(load_golden("checkers_stage2_uniform"), 0)
    rows = rows_from_columns(cols, CHECKERS_ORDER)
    _fields_read_back(rows, cols, CHECKERS_ORDER)
    rec = _recorded("checkers")
    assert rec["pb_00"] == T
    flat = [rec[k] for k in sorted(rec) if k != "pb_00"]
    assert any(o.shape == (T * N, 3, 9, 2) and np.array_equal(o, np.repeat(cols["grid"], N, axis=0)) for o in flat)
    assert any(o.shape == (T, N, 4) and np.array_equal(o, cols["vec"]) for o in flat)
    assert any(o.shape == (T * N, 5, 5, 3) and np.array_equal(o, cols["obs_self_t"].reshape(T * N, 5, 5, 3)) for o in flat)
