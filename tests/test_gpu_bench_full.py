"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run measures the headline alone and writes nothing but its line;
everything that takes runs of its own (bandwidth, CPU baselines, launch floor, other configs, launch modes, policy rollouts,
sweep, host-side timings) comes with --full."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cpu_baseline", "other_configs", "launch_modes", "fused_rollout", "policy_rollout", "sweep", "host_side")


def _bench(args):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"] + args, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.strip().splitlines()


def test_plain_run_measures_the_headline_alone():
    record = os.path.join(ROOT, "bench_extras.json")
    before = os.stat(record).st_mtime_ns if os.path.exists(record) else None
    lines = _bench([])
    assert len(lines) == 1, lines[:-1]                     # no extras_summary line before the driver's
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 1e6 and line["ms_per_step"] > 0
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert 0 < line["roofline"]["frac"] < 1
    assert not set(FULL_ONLY) & set(line), sorted(set(FULL_ONLY) & set(line))
    assert not {"measured_read_GBps", "launch_floor", "ceiling_frac"} & set(line["roofline"])
    assert (os.stat(record).st_mtime_ns if os.path.exists(record) else None) == before     # the record is --full's


def test_full_run_adds_the_extras(tmp_path):
    record = tmp_path / "record.json"
    lines = _bench(["--full", "--no-sweep", "--no-cpu-baseline", "--no-other-configs", "--extras-file", str(record)])
    line = json.loads(lines[-1])
    assert "extras_summary" in json.loads(lines[-2])
    with open(record) as fh:
        out = json.load(fh)
    assert out["value"] == pytest.approx(line["value"], rel=1e-5)
    for k in ("launch_modes", "fused_rollout", "policy_rollout", "host_side"):
        assert k in out, k
    assert "error" not in out["host_side"], out["host_side"]
    assert out["roofline"]["measured_read_GBps"] > 0 and out["roofline"]["launch_floor"]["same_traffic_us"] > 0
    assert line["policy_rollout"]["us_per_tick"] > 0 and line["roofline"]["launch_floor"]["frac_of_floor"] > 0
