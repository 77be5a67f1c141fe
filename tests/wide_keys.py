"""TEST INFRASTRUCTURE ONLY -- the keys under which the device random streams are pinned at full width, and the keys a kernel that
lost bits would effectively use (shared by tests/test_wide_keys_oracle.py, tests/test_philox_header.py and
tests/test_gpu_wide_keys.py; no GPU here).

Every draw of the build is one Philox4x32-10 block (csrc/philox.h): key words (uint32)seed and (uint32)(seed >> 32), counter words 0
and 1 the low and high half of a 64-bit id -- env_id_base + local env for the env, policy and exploration streams, row_id_base + row
for the rows streams.  The constants put live bits into every one of those words:

  SEEDS[0] = 0x9E3779B97F4A7C15   both key words non-zero and different, bit 63 set (a seed kept in a signed or 32-bit field shows)
  SEEDS[1] = 1 << 32              the low key word is ZERO: a kernel that keeps only the low word draws the seed-0 stream
  BASE     = (5 << 32) - 19       local env / row 0..18 have id high word 4 and low words 0xFFFFFFED..0xFFFFFFFF; local 19 is the first
                                  whose id carried out of the low word (high word 5, low word 0)
  E        = 37                   a partial wave with both sides of the carry in it: 19 entries before, 18 after
  CARRY    = 19                   the first local index past the carry; BASE + CARRY = 5 << 32 is also the base of the shard
                                  [19, 37), a base whose LOW word is zero
  ROWS_BASE_HIGH = 2^63 + 11      a row id base with bit 63 set, for the entry point whose ABI field is unsigned
  DRAW_LAST = 0xFFFFFFFF          the last value of the 32-bit draw counter of the rows streams

corruptions() yields, for a key (seed, ids), the three keys a broken kernel, wrapper or record would draw under, each with the mask of
the entries it changes: "seed_lo" (the seed's low word only; every entry), "id_lo" (the id's low word only; every entry), "no_carry"
(the low word wraps inside the batch and the high word does not move; the entries past the carry).  The CPU file proves that the
oracle's output differs under each of them in at least MIN_DIFFERENT of the affected entries at every point the GPU file compares,
which is what makes the GPU file's equalities able to fail.
"""
import numpy as np

from oracle import actor_oracle as AO
from oracle import philox
from tests import actor_rows_ref as RR
from tests import qmix_ref as QR

MASK32 = 0xFFFFFFFF
SEEDS = (0x9E3779B97F4A7C15, 1 << 32)
BASE = (5 << 32) - 19
E = 37
CARRY = 19
SHARD_BASE = BASE + CARRY
ROWS_BASE_HIGH = (1 << 63) + 11
DRAW_LAST = 0xFFFFFFFF
MIN_DIFFERENT = 0.25


def ids(base=BASE, n=E):
    """uint64 [n]: the global ids base .. base + n - 1 (mod 2^64)."""
    return np.arange(n, dtype=np.uint64) + np.uint64(int(base) & 0xFFFFFFFFFFFFFFFF)


def corruptions(seed, id_array):
    """(name, seed', ids', affected bool [n]) for the three ways of losing bits; a corruption that changes nothing of this key
    (no carry inside the batch) is left out."""
    id_array = np.asarray(id_array, dtype=np.uint64)
    everything = np.ones(id_array.shape[0], bool)
    lo = id_array & np.uint64(MASK32)
    stuck = (id_array[0] >> np.uint64(32) << np.uint64(32)) | lo
    yield "seed_lo", int(seed) & MASK32, id_array, everything
    yield "id_lo", int(seed), lo, everything
    if (stuck != id_array).any():
        yield "no_carry", int(seed), stuck, stuck != id_array


# ---- the points at which the GPU file compares a stream with the oracle (tests/test_gpu_wide_keys.py draws its cases from here) ----
MAX_STEPS, TICKS = 3, 8                      # particle cases A / B / D / E: every env restarts at steps == 3, so 8 ticks reach episode 3
PARTICLE_N = (2, 4, 5)
CHECKERS_N = (2, 5)
EPISODES = (1, 2, 3)
STEPS = (0, 1, 2)
GOAL_EPISODES = (2, 3, 4)                    # Checkers N = 1: reset() takes the first goal, the same-launch restarts draw these
ROWS_DRAWS = (0, 7, 0xFFFFFFFE, DRAW_LAST)   # explicit draws, and the device counter from 0xFFFFFFFE: FFFFFFFE, FFFFFFFF, 0
ROWS_BASES = (BASE, ROWS_BASE_HIGH)
RESET_CFG = {2: "particle_stage2_merge.json", 4: "particle_merge8.json", 5: "particle_merge8.json"}
P_RANDOM = 0.2


def _reset_rows(seed, id_array, n_agents, episode):
    from tests.helpers import load_cfg
    pos, lm, _ = philox.expected_reset(seed, id_array, episode, load_cfg(RESET_CFG[n_agents]), n_agents, P_RANDOM)
    return np.concatenate([pos.reshape(len(id_array), -1), lm.reshape(len(id_array), -1)], axis=1)


def oracle_points():
    """(label, base, fn) with fn(seed, ids) -> array [n, ...]: the oracle's output of one stream at one point the GPU file compares."""
    pts = []
    for n in sorted(set(PARTICLE_N) | set(CHECKERS_N)):
        for ep in EPISODES:
            for st in STEPS:
                pts.append(("actions N=%d ep=%d step=%d" % (n, ep, st), BASE,
                            lambda s, i, n=n, ep=ep, st=st: philox.expected_actions(s, i, ep, st, n)))
                pts.append(("policy N=%d ep=%d step=%d" % (n, ep, st), BASE,
                            lambda s, i, n=n, ep=ep, st=st: AO.policy_uniforms(s, i, ep, st, n)))
                pts.append(("explore N=%d ep=%d step=%d" % (n, ep, st), BASE,
                            lambda s, i, n=n, ep=ep, st=st: np.stack(QR.explore_words(s, i, ep, st, n), -1).reshape(len(i), -1)))
    for n in PARTICLE_N:
        for ep in EPISODES:
            pts.append(("reset N=%d ep=%d" % (n, ep), BASE, lambda s, i, n=n, ep=ep: _reset_rows(s, i, n, ep)))
    for ep in GOAL_EPISODES:
        pts.append(("goal ep=%d" % ep, BASE, lambda s, i, ep=ep: philox.reset_words(s, i, ep, 0)[0] & np.uint32(1)))
    for base in ROWS_BASES:
        for draw in ROWS_DRAWS:
            pts.append(("rows base=%#x draw=%#x" % (base, draw), base, lambda s, i, draw=draw: RR.rows_words(s, i, draw)))
    return pts


def different_fraction(a, b, affected):
    """Share of the ELEMENTS of the affected entries (leading axis) at which the two outputs differ -- for real outputs (the reset
    positions) by more than 1e-6, twice the widest bound the GPU file compares them under."""
    a, b = np.asarray(a), np.asarray(b)
    d = (np.abs(a - b) > 1e-6) if a.dtype == np.float64 else (a != b)
    return float(d[affected].mean())
