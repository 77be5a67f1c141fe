"""GPU: bench.py --dump-outputs writes what the last timed step computed -- the same arrays on every run with the same arguments,
float32 / float64 only, at most 64 MB -- and --steps sets the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, tag, steps):
    out = tmp_path / tag
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--no-extras",
                        "--no-sweep", "--no-cpu-baseline", "--no-other-configs", "--extras-file", str(tmp_path / (tag + ".json")),
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    with open(tmp_path / (tag + ".json")) as fh:
        line.update(ticks_timed=json.load(fh)["ticks_timed"])       # (the full record; the stdout line is the compact one)
    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out)) if f.endswith(".npy")}
    return line, arrays, sum(os.path.getsize(out / f) for f in os.listdir(out))


def test_dumped_outputs_repeat_and_follow_the_step_count(tmp_path):
    line, a, size = _bench(tmp_path, "a", 2)
    assert line["steps"] == 2 and line["ticks_timed"] == 2 * 330
    assert size <= 64 * 10 ** 6
    assert {"state", "obs_others", "actions", "reward", "reward_n", "done", "goals", "env_index"} <= set(a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    n = len(a["env_index"])
    assert 0 < n <= 4096 and a["state"].shape == (331, 4, n, 4) and a["obs_others"].shape == (331, n, 4, 12)
    assert np.isfinite(a["state"]).all() and set(np.unique(a["actions"])) <= set(range(5))
    _, b, _ = _bench(tmp_path, "b", 2)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k                  # same arguments: same inputs, same outputs
    line, c, _ = _bench(tmp_path, "c", 3)
    assert line["steps"] == 3 and line["ticks_timed"] == 3 * 330
    assert not np.array_equal(a["state"], c["state"])        # one more collection phase: a later trajectory
