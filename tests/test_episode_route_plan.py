"""CPU: the routing plan of DeviceDualReplayBuffer.add_rollout (csrc/episode_route.h), checked without a GPU.

The plan's arithmetic -- the per-env walks, the rank -> ring row rule, the skip rule -- is plain C++17 in one header that the kernels
of csrc/episode_route.hip include.  A small program with its own main(), written here and compiled with the host compiler under
AddressSanitizer and UBSan, runs the header's sequential route_plan_host() on the chunks it reads; sel / row / flush_row / counts /
pend_len are compared with the host model of tests/dual_ref.py, which walks `for t: for e:` with per-env episode lists and drives two
RingIndex objects add by add.

Cases: E = 70, T = 7, three chained chunks, with P = 5 and with P = 12.  An episode that spans TWO chunk boundaries is at least T + 2
= 9 ticks long and has 8 of them pending before its last chunk: it cannot occur with a pending store of 5 rows (episodes are at most
P ticks long), so that situation is asserted at P = 12 and every other one at both depths.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.dual_ref import DualModel, crafted_chunks, crafted_sync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cm3_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "episode_route.h"
// reads chunks: T E P sync has_valid idx0 size0 idx1 size1, then done [T E], collisions [T E], valid [T E] (if any), pend_in [E];
// the arrays are given odd tick strides; every output array is allocated at its exact size (ASan sees any write past it)
int main() {
  cm3::RouteShape s;
  int has_valid;
  long long i0, m0, i1, m1;
  while (scanf("%d %d %d %d %d %lld %lld %lld %lld", &s.T, &s.E, &s.P, &s.sync, &has_valid, &i0, &m0, &i1, &m1) == 9) {
    if (!cm3::route_shape_fits(s.T, s.E, s.P)) { printf("refused\n"); continue; }
    s.idx[0] = i0; s.maxsize[0] = m0; s.idx[1] = i1; s.maxsize[1] = m1;
    const size_t cells = (size_t)s.T * s.E;
    s.st_done = s.E + 3; s.st_coll = (size_t)(s.E + 1) * 4; s.st_valid = s.E + 5;
    std::vector<uint8_t> done(s.st_done * s.T), valid(s.st_valid * s.T);
    std::vector<int32_t> coll((s.E + 1) * (size_t)s.T), pend(s.E), pend_out(s.E);
    int v;
    for (int t = 0; t < s.T; ++t) for (int e = 0; e < s.E; ++e) { if (scanf("%d", &v) != 1) return 2; done[t * s.st_done + e] = (uint8_t)v; }
    for (int t = 0; t < s.T; ++t) for (int e = 0; e < s.E; ++e) { if (scanf("%d", &v) != 1) return 2; coll[(size_t)t * (s.E + 1) + e] = v; }
    if (has_valid) for (int t = 0; t < s.T; ++t) for (int e = 0; e < s.E; ++e) { if (scanf("%d", &v) != 1) return 2; valid[t * s.st_valid + e] = (uint8_t)v; }
    for (int e = 0; e < s.E; ++e) if (scanf("%d", &pend[e]) != 1) return 2;
    s.done = done.data(); s.coll = coll.data(); s.valid = has_valid ? valid.data() : nullptr;
    std::vector<uint8_t> sel(cells);
    std::vector<int64_t> row(cells), flush(2 * (size_t)s.P * s.E), counts(2);
    std::vector<uint64_t> scratch(cm3::route_scratch_words(cells));
    cm3::route_plan_host(s, pend.data(), pend_out.data(), sel.data(), row.data(), flush.data(), counts.data(), scratch.data());
    for (size_t b = 0; b < cells; ++b) printf("%d ", (int)sel[b]);
    printf("\n");
    for (size_t b = 0; b < cells; ++b) printf("%lld ", (long long)row[b]);
    printf("\n");
    for (size_t b = 0; b < flush.size(); ++b) printf("%lld ", (long long)flush[b]);
    printf("\n%lld %lld\n", (long long)counts[0], (long long)counts[1]);
    for (int e = 0; e < s.E; ++e) printf("%d ", s.sync ? 0 : pend_out[e]);
    printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """plan(T, E, P, sync, idx, sizes, done, coll, valid, pend_in) -> dict of the header's outputs, or None where it refuses"""
    tmp = tmp_path_factory.mktemp("route_plan")
    src, exe = tmp / "plan.cpp", tmp / "plan"
    src.write_text(PROGRAM)
    san = ["-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe)]
    if shutil.which("g++"):
        subprocess.check_call(["g++"] + san + [str(src)])
    elif os.path.exists(HIPCC):
        subprocess.check_call([HIPCC, "-x", "c++"] + san + [str(src)])      # host only: the header holds no device code
    else:
        pytest.skip("no host C++ compiler")

    def plan(T, E, P, sync, idx, sizes, done=None, coll=None, valid=None, pend_in=None):
        head = [T, E, P, int(sync), int(valid is not None), idx[0], sizes[0], idx[1], sizes[1]]
        parts = [head] + [np.asarray(a).reshape(-1).tolist() for a in (done, coll, valid, pend_in) if a is not None]
        text = "\n".join(" ".join(str(int(v)) for v in p) for p in parts) + "\n"
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr          # (a sanitizer report ends the program with a non-zero status)
        lines = out.stdout.splitlines()
        if lines == ["refused"]:
            return None
        assert len(lines) == 5
        sel, row, flush, counts, pend = (np.array(line.split(), dtype=np.int64) for line in lines)
        return dict(sel=sel.astype(np.uint8), row=row, flush_row=flush.reshape(2, -1), counts=counts, pend_len=pend.astype(np.int32))
    return plan


def _same(got, want, P, what):
    for k in ("sel", "row", "counts", "pend_len"):
        assert np.array_equal(got[k], want[k]), (what, k)
    if P:
        assert np.array_equal(got["flush_row"], want["flush_row"]), (what, "flush_row")


SITUATIONS = {"several ends of both classes at one tick", "one boundary", "two ends in one chunk", "wrap", "more than a ring holds",
              "pending row overwritten by the call that flushes it"}


@pytest.mark.parametrize("P", [5, 12])
def test_three_chained_chunks_equal_the_host_model(planner, P):
    E, T, sizes = 70, 7, (37, 600)
    done, coll = crafted_chunks(E, T, P, 3, seed=P)
    model = DualModel(sizes, E, P)
    pend = np.zeros(E, np.int32)
    for c in range(3):
        sl = slice(c * T, (c + 1) * T)
        want = model.add_chunk(done[sl], coll[sl])
        got = planner(T, E, P, False, want["idx"], sizes, done[sl], coll[sl], None, pend)
        _same(got, want, P, "chunk %d" % c)
        pend = got["pend_len"]                               # chained: the next chunk starts from what the header itself wrote
        assert set(np.unique(got["sel"])) <= {0, 1, 2, 255}
    # the model itself met every situation the case is about (asserted, not skipped)
    assert {cls for cls, _ in model.episodes} == {0, 1}
    assert SITUATIONS <= model.seen, SITUATIONS - model.seen
    assert ("two boundaries" in model.seen) == (P == 12)
    assert model.pending == int(pend.sum()) > 0
    assert all(np.count_nonzero(m >= 0) == r.len for m, r in zip(model.mem, model.rings))


def test_synchronous_flag_with_a_valid_mask_and_envs_that_never_finish(planner):
    E, T, sizes = 70, 7, (50, 1000)
    done, coll, valid = crafted_sync(E, T, seed=3)
    assert not done[:, :5].any() and not valid[:, 5:8].any()
    model = DualModel(sizes, E, 0)
    model.rings[0].plan_add(45)                              # (the bad ring wraps)
    want = model.add_chunk(done, coll, valid, sync=True)
    got = planner(T, E, 0, True, want["idx"], sizes, done, coll, valid, np.zeros(E, np.int32))
    _same(got, want, 0, "sync")
    assert int(want["counts"].sum()) == int(valid.sum()) and not (got["sel"] == 2).any()
    never = [toks for cls, toks in model.episodes if toks[0] < 5]
    assert len(never) == 5 and all(len(toks) == T for toks in never)           # envs that never finish end at the last tick
    assert {cls for cls, _ in model.episodes} == {0, 1} and "wrap" in model.seen


def test_a_tail_that_outgrows_the_pending_store_saturates_and_stays_in_bounds(planner):
    """No done at all: every env's tail outgrows P.  pend_len saturates at P, the newest P transitions take rows P - 1 downwards, the
    older ones are dropped, no pending row >= P is named (the Python class refuses such a configuration: its pending store is
    max_steps deep)."""
    E, T, P = 5, 7, 3
    got = planner(T, E, P, False, (0, 0), (10, 10), np.zeros((T, E)), np.zeros((T, E)), None, np.ones(E))
    pend = got["sel"] == 2
    assert got["row"][pend].max() < P * E and got["row"][pend].min() >= 0 and (got["pend_len"] == P).all()
    assert (got["flush_row"] == -1).all() and (got["counts"] == 0).all()
    sel, row = got["sel"].reshape(T, E), got["row"].reshape(T, E)
    for t in range(T):                                   # ticks T - P .. T - 1 are kept, on rows 0 .. P - 1 in time order
        k = t - (T - P)
        assert (sel[t] == (2 if k >= 0 else 255)).all() and (row[t] == (k * E + np.arange(E) if k >= 0 else -1)).all()


def test_shapes_beyond_31_bits_are_refused(planner):
    assert planner(1 << 16, 1 << 15, 0, False, (0, 0), (1, 1)) is None
    assert planner(7, 1 << 20, 2041, False, (0, 0), (1, 1)) is None
