"""CPU: which build of the particle step kernels a launch runs (cm3::plan_step, csrc/particle_plan.h), checked without a GPU.

The choice is a pure function of a handful of integers in a header that needs no HIP, so a small program with its own main() --
written here, compiled with the host compiler under AddressSanitizer and UBSan -- prints the plan of every shape it reads, and the
plans are compared with the independent restatement of the table in tests/test_gpu_dispatch_sizes.py (which the GPU tests assert
against what really ran), with the builds the collector tests expect, and with three properties over a sweep of shapes.
"""
import os
import shutil
import subprocess

import pytest

import tests.test_gpu_dispatch_sizes as dispatch
from tests.test_gpu_dispatch_sizes import CROSSOVERS, ONE_WAVE_MAX, expected_variant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cm3_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

FLAG_GEN_ACTIONS, FLAG_NT = 0x2, 0x100000
FORCED = {None: 0, "env": 0x100, "pair": 0x200, "agent": 0x800}
KERNELS = ["k_particle_step", "k_particle_step_pairs", "k_particle_step_agents", "k_particle_step_agents2"]
SP = ["plain", "nt", "wt"]
FIELDS = ("refused", "map", "waves", "fused", "sp", "live", "rec", "early", "ilp", "raw_blocks", "grid_blocks", "xcd", "exists",
          "takes_record")

PROGRAM = r"""
#include <stdio.h>
#include "particle_plan.h"
static_assert(CM3_FLAG_GEN_ACTIONS == 0x2 && CM3_FLAG_KERNEL_LANE_PER_ENV == 0x100 && CM3_FLAG_KERNEL_LANE_PER_PAIR == 0x200 &&
              CM3_FLAG_KERNEL_LANE_PER_AGENT == 0x800 && cm3::kFlagObsStoreNt == 0x100000, "the flag values the test writes");
int main() {
  cm3::StepShape s;
  unsigned flags;
  int copy, record;
  while (scanf("%d %d %d %d %d %d %u %d %d", &s.real_bytes, &s.n_agents, &s.E, &s.E0, &s.EN, &s.n_ticks, &flags, &copy, &record) == 9) {
    s.flags = flags;
    s.slot_copy = copy != 0;
    s.live_record = record != 0;
    cm3::StepPlan p = {};
    const int why = cm3::plan_step(s, p);
    const bool exists = why == cm3::kPlanOk &&
                        cm3::step_variant_exists(p.map, s.real_bytes, s.n_agents, p.waves, p.fused, p.sp, p.live, p.rec, p.early);
    printf("%d %d %d %d %d %d %d %d %d %u %u %u %d %d\n", why, p.map, p.waves, p.fused, p.sp, p.live, p.rec, p.early, p.ilp,
           p.raw_blocks, p.grid_blocks, (unsigned)(p.xcd_flags >> 24), (int)exists, (int)cm3::plan_takes_record(s));
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """plans(shapes) -> one dict per shape; a shape is (real_bytes, N, E, E0, EN, n_ticks, flags, slot_copy, live_record)."""
    tmp = tmp_path_factory.mktemp("step_plan")
    src, exe = tmp / "plan.cpp", tmp / "plan"
    src.write_text(PROGRAM)
    san = ["-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe)]
    if shutil.which("g++"):
        subprocess.check_call(["g++"] + san + [str(src)])
    elif os.path.exists(HIPCC):
        subprocess.check_call([HIPCC, "-x", "c++"] + san + [str(src)])      # host only: the header holds no device code
    else:
        pytest.skip("no host C++ compiler")

    def plans(shapes):
        text = "".join(" ".join(str(int(v)) for v in s) + "\n" for s in shapes)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr          # (a sanitizer report ends the program with a non-zero status)
        rows = [dict(zip(FIELDS, map(int, line.split()))) for line in out.stdout.splitlines()]
        assert len(rows) == len(shapes)
        return rows
    return plans


def _shape(N, E, real_bytes=4, n_ticks=1, flags=0, forced=None, copy=0, record=0, E0=0, EN=None):
    return (real_bytes, N, E, E0, E if EN is None else EN, n_ticks, flags | FORCED[forced], copy, record)


def _as_variant(p):
    return dict(kernel=KERNELS[p["map"]], waves=p["waves"], sp=SP[p["sp"]], early=p["early"], tu="ilp" if p["ilp"] else "default",
                fused=p["fused"], live=p["live"])


def _rows(test):
    """the (N, E, ...) rows a GPU test of test_gpu_dispatch_sizes.py is parametrised with"""
    return [tuple(r) for m in test.pytestmark if m.name == "parametrize" and m.args[0].startswith("N,E") for r in m.args[1]]


TEACHER_FORCED = _rows(dispatch.test_large_batch_builds_vs_f64_oracle_teacher_forced)     # (N, E, forced)
COLLECTOR = _rows(dispatch.test_collector_at_streaming_sizes_equals_stepwise)             # (N, E, T, want)


def test_plan_agrees_with_the_restated_table(planner):
    """(a) float32, n_ticks = 1: both sides of every listed crossover and the 14 teacher-forced rows."""
    cases = [(N, cross + side, None) for N, cross in CROSSOVERS for side in (0, 1)] + TEACHER_FORCED
    got = planner([_shape(N, E, forced=forced) for N, E, forced in cases])
    assert len(TEACHER_FORCED) == 14 and len(COLLECTOR) == 9 and len(cases) == 2 * len(CROSSOVERS) + 14
    for (N, E, forced), p in zip(cases, got):
        assert p["refused"] == 0 and p["exists"] == 1, (N, E, forced, p)
        want = dict(expected_variant(N, E, forced), fused=0, live=0)
        assert _as_variant(p) == want, (N, E, forced)


def test_plan_gives_the_collector_rows_their_builds(planner):
    """(b) the per-tick launches of ParticleRollout at streaming sizes: the non-temporal bit is set (>= 128 MB of observation
    slots), a slot copy is present where the collector keeps live state."""
    for N, E, T, want in COLLECTOR:
        assert E * N * 4 * (N - 1) * 4 * T >= (128 << 20)
    got = planner([_shape(N, E, flags=FLAG_NT | FLAG_GEN_ACTIONS, copy=want["live"]) for N, E, T, want in COLLECTOR])
    for (N, E, T, want), p in zip(COLLECTOR, got):
        assert p["refused"] == 0 and p["exists"] == 1 and p["rec"] == 0, (N, E, p)
        have = dict(_as_variant(p), fused=p["fused"])
        assert {k: have[k] for k in want} == want and p["fused"] == 0, (N, E, have, want)


def _probe_sizes(N):
    """the sizes test_the_crossover_list_covers_every_change_of_the_table scans"""
    marks = sorted(c for n, c in CROSSOVERS if n == N)
    return sorted(set([1, 2, 3] + [m + d for m in marks for d in (-1, 0, 1, 2)] + [1 << k for k in range(3, 22)] +
                      [3 << k for k in range(3, 20)] + [2 ** 21 + 1]))


def test_properties_of_every_plan_over_a_sweep(planner):
    """(c) N 1..10, both reals, the probe sizes of the crossover scan, fused and per-tick, streaming bit, slot copy, live record,
    every forced mapping."""
    shapes = [_shape(N, E, rb, T, nt | FLAG_GEN_ACTIONS, forced, copy, record)
              for N in range(1, 11) for rb in (4, 8) for E in _probe_sizes(N) for T in (1, 5) for nt in (0, FLAG_NT)
              for copy, record in ((0, 0), (1, 0), (1, 1)) for forced in FORCED]
    got = planner(shapes)
    seen = set()
    for s, p in zip(shapes, got):
        rb, N, E, _, _, T, flags, copy, record = s
        if T > 1 and record:
            assert p["refused"] != 0, s                                     # no record build of the tick loop
        if p["refused"]:
            continue
        assert p["exists"] == 1, (s, p)                                     # every plan names a build the library contains
        seen.add((p["map"], p["waves"], p["fused"], p["sp"], p["live"], p["rec"], p["early"], p["ilp"]))
        if rb == 8:
            assert p["sp"] == 0 and p["ilp"] == 0 and p["map"] != 3, (s, p)
        if T > 1:
            assert p["fused"] == 1 and p["live"] == 0 and p["early"] == 0 and p["sp"] != 2 and p["map"] != 3, (s, p)
        else:
            assert p["fused"] == 0, (s, p)
        assert p["raw_blocks"] >= 1 and p["grid_blocks"] >= p["raw_blocks"], (s, p)
        if p["map"] == 0:
            assert p["waves"] == (1 if E <= ONE_WAVE_MAX else 4) and p["xcd"] == 0 and p["live"] == 0, (s, p)
    # the sweep reaches every kind of build: each mapping, both workgroup sizes, fused, all store policies, live, record, early, both units
    for col, values in enumerate([(0, 1, 2, 3), (1, 4), (0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1)]):
        assert {v[col] for v in seen} == set(values), col


def test_grids_block_order_flags_and_sub_ranges_by_hand(planner):
    """Workgroups, launched grid and the XCD mode byte, worked out by hand from the geometry (envs per wave: pairs 64 / pow2(N x lanes
    per agent), agents 64 / pow2(N), two lanes per agent 4, lane per env 64) and the block-order rule (< 64 workgroups: plain order,
    mode 0; <= 256: eighths, mode = ceil(blocks / 8), grid = 8 x mode; above: tiles of 256, mode 63, grid rounded up to 256).  The
    grid and the write-through / two-lane gates count the envs of the launch (EN - E0); waves per workgroup and the translation
    unit count the waves of the whole array (E)."""
    cases = [
        # (shape, map, waves, raw, grid, xcd, sp, early, ilp)
        (_shape(4, 4096), 1, 4, 256, 256, 32, 0, 0, 1),                         # 4 envs per wave, 1024 waves: 16 envs per workgroup
        (_shape(4, 4096, E0=1000, EN=3001), 1, 4, 126, 128, 16, 0, 0, 1),       # 2001 envs of the same array: still 4 waves
        (_shape(2, 1000), 1, 1, 32, 32, 0, 0, 0, 1),                            # 32 envs per wave, 32 waves
        (_shape(2, 8160), 1, 1, 255, 256, 32, 0, 0, 1),                         # 255 waves: the last single-wave size
        (_shape(2, 8161), 1, 4, 64, 64, 8, 0, 0, 1),                            # 256 waves: 128 envs per workgroup
        (_shape(8, 8192), 3, 4, 512, 512, 63, 2, 1, 1),                         # two lanes per agent: 16 envs per workgroup; 7.3 MB: wt, early
        (_shape(8, 100, forced="agent"), 3, 1, 25, 25, 0, 0, 0, 1),             # 13 waves of 8 envs: one wave, 4 envs per workgroup
        (_shape(8, 40009), 2, 4, 1251, 1280, 63, 2, 0, 1),                      # 8 envs per wave, 32 per workgroup; 5002 waves: max-ILP
        (_shape(8, 40009, EN=30000), 3, 4, 1875, 2048, 63, 2, 0, 1),            # 30 000 envs of it: two lanes per agent, above the early gate
        (_shape(8, 150001), 2, 4, 4688, 4864, 63, 2, 0, 0),                     # 18 751 waves: the default unit
        (_shape(4, 200003), 0, 4, 782, 782, 0, 2, 0, 0),                        # lane per env, 256 envs per workgroup, no block order
        (_shape(2, 300000, forced="env", E0=100000, EN=100065), 0, 4, 1, 1, 0, 0, 0, 0),
        (_shape(4, 20011, forced="env"), 0, 1, 313, 313, 0, 2, 0, 0),           # 20 011 x 192 B = 3.84 MB of rows: write-through
        (_shape(4, 20011, forced="env", EN=10000), 0, 1, 157, 157, 0, 0, 0, 0),  # 1.92 MB of them in this launch: plain
        (_shape(4, 20011, forced="env", copy=1), 0, 1, 313, 313, 0, 0, 0, 0),   # lane per env: no write-through beside a slot copy
        (_shape(6, 9000, copy=1), 2, 4, 282, 512, 63, 2, 0, 1),                 # lane per agent: the slot copy does not stop it
    ]
    got = planner([c[0] for c in cases])
    for (shape, *want), p in zip(cases, got):
        have = [p[k] for k in ("map", "waves", "raw_blocks", "grid_blocks", "xcd", "sp", "early", "ilp")]
        assert p["refused"] == 0 and have == want, (shape, have, want)


def test_which_shapes_take_a_live_record_also_beyond_4_gib(planner):
    """cm3_particle_live_record_applies for shapes with a slot copy and a record: float32, 2..4 agents, per-tick, in-kernel
    actions, records below 4 GiB (E < 2^25), and the launch goes to the lane-per-pair kernel.  A forced pair mapping whose
    obs_others reaches 4 GiB (N = 4: E >= 22 369 622) still takes the record -- the launch then names the limit -- but only
    where every record condition holds."""
    big = 23000000                      # N = 4: 4.4 GB of obs_others, 2.9 GB of records
    assert big * 4 * 3 * 16 >= 1 << 32 and big * 128 < 1 << 32
    rec = dict(copy=1, record=1)
    cases = [
        (_shape(4, 12288, flags=FLAG_GEN_ACTIONS, **rec), 1), (_shape(4, 12289, flags=FLAG_GEN_ACTIONS, **rec), 0),
        (_shape(4, 12289, flags=FLAG_GEN_ACTIONS, forced="pair", **rec), 1),
        (_shape(4, big, flags=FLAG_GEN_ACTIONS, forced="pair", **rec), 1),
        (_shape(4, big, flags=FLAG_GEN_ACTIONS, **rec), 0),                                  # not forced: lane per env at that size
        (_shape(4, big, flags=0, forced="pair", **rec), 0),                                  # no in-kernel actions
        (_shape(4, big, flags=FLAG_GEN_ACTIONS, forced="pair", n_ticks=2, **rec), 0),        # the tick loop
        (_shape(4, big, flags=FLAG_GEN_ACTIONS, forced="pair", real_bytes=8, **rec), 0),     # float64
        (_shape(8, big, flags=FLAG_GEN_ACTIONS, forced="pair", **rec), 0), (_shape(5, big, flags=FLAG_GEN_ACTIONS, forced="pair", **rec), 0),
        (_shape(4, 34000000, flags=FLAG_GEN_ACTIONS, forced="pair", **rec), 0),              # 128 B x E >= 4 GiB
        (_shape(3, 100000000, flags=FLAG_GEN_ACTIONS, forced="pair", **rec), 0),
        (_shape(4, big, flags=FLAG_GEN_ACTIONS, forced="agent", **rec), 0),
    ]
    got = planner([c[0] for c in cases])
    for (shape, want), p in zip(cases, got):
        assert p["takes_record"] == want, (shape, p)
        assert (p["refused"] == 0) == (want == 1 and shape[2] < 22369622), (shape, p)        # beyond 4 GiB the launch itself is refused
