"""TEST INFRASTRUCTURE ONLY -- the host model of DeviceDualReplayBuffer.add_rollout and of cm3_episode_route_plan.

The model is the reference's feeding of replay_buffer_dual.Replay_Buffer (alg/train_onpolicy.py:300-356) done by a host that walks a
vectorised collection `for t: for e:`: every env keeps the list of its running episode's transitions; where a done byte is met the
whole list goes, oldest first, into the ring its collision count names, ONE RingIndex.plan_add(1) per transition.  Transitions are
TOKENS (chunk number * T * E + t * E + e), so a test can look up what a ring row must hold.  From the same walk the model derives what
the routing plan must say: sel / row of the chunk's transitions, flush_row of the pending rows, counts and pend_len.
"""
import numpy as np

from cm3_amd.replay import RingIndex

BAD, GOOD, PENDING, SKIP = 0, 1, 2, 255


class DualModel(object):
    def __init__(self, sizes, E, P):
        self.rings = [RingIndex(sizes[0]), RingIndex(sizes[1])]
        self.mem = [np.full(sizes[0], -1, np.int64), np.full(sizes[1], -1, np.int64)]      # ring row -> token
        self.E, self.P = int(E), int(P)
        self.running = [[] for _ in range(self.E)]          # tokens of every env's running episode (continuous collection)
        self.pend = np.full((max(self.P, 1), self.E), -1, np.int64)                         # pending row (k, e) -> token last written
        self.pend_pos = {}                                  # token -> (k, e)
        self.n_tokens = 0
        self.episodes = []                                  # (class, tokens) in the order they were added
        self.seen = set()                                   # which of the situations a test wants to have occurred did

    @property
    def pending(self):
        return sum(len(r) for r in self.running)

    def add_chunk(self, done, coll, valid=None, sync=False):
        """-> the plan this chunk must get: dict(sel, row, flush_row, counts, pend_len, idx) (idx: both rings' idx BEFORE the chunk)"""
        done, coll = np.asarray(done).astype(bool), np.asarray(coll)
        T, E, P = done.shape[0], self.E, self.P
        assert done.shape == (T, E) == coll.shape
        base = self.n_tokens
        self.n_tokens += T * E
        idx = [r.idx for r in self.rings]
        run = [[] for _ in range(E)] if sync else self.running
        where, counts = {}, [0, 0]
        ends_in_chunk = np.zeros(E, int)
        for t in range(T):
            ends_here = [0, 0]
            for e in range(E):
                v = valid is None or bool(valid[t, e])
                if v:
                    run[e].append(base + t * E + e)
                end = v and done[t, e]
                if sync and t == T - 1 and run[e]:
                    end = True                              # still open at the last tick: ends there with its count so far
                if not end:
                    continue
                cls = BAD if coll[t, e] != 0 else GOOD
                for tok in run[e]:
                    skip, start, kept = self.rings[cls].plan_add(1)
                    assert (skip, kept) == (0, 1)
                    if start == 0 and self.rings[cls].len > 1:
                        self.seen.add("wrap")                # (back at row 0 and not the ring's first add)
                    self.mem[cls][start] = tok
                    where[tok] = (cls, start)
                    counts[cls] += 1
                chunks = {tok // (T * E) for tok in run[e]}
                if len(chunks) >= 3:
                    self.seen.add("two boundaries")
                if len(chunks) >= 2:
                    self.seen.add("one boundary")
                self.episodes.append((cls, list(run[e])))
                run[e] = []
                ends_here[cls] += 1
                ends_in_chunk[e] += 1
            if ends_here[0] > 1 and ends_here[1] > 1:
                self.seen.add("several ends of both classes at one tick")
        if ends_in_chunk.max() >= 2:
            self.seen.add("two ends in one chunk")
        for c in (0, 1):
            if counts[c] > self.rings[c].maxsize:
                self.seen.add("more than a ring holds")
        sel, row = np.full(T * E, SKIP, np.uint8), np.full(T * E, -1, np.int64)
        flush = np.full((2, max(P, 1) * E), -1, np.int64)
        for tok, (cls, r) in where.items():
            if self.mem[cls][r] != tok:
                continue                                    # this very call overwrote it
            if tok >= base:
                sel[tok - base], row[tok - base] = cls, r
            else:
                k, e = self.pend_pos[tok]
                flush[cls, k * E + e] = r
        if not sync:
            for e in range(E):
                for k, tok in enumerate(run[e]):
                    if tok < base:
                        continue
                    assert k < P, "the model's episodes must fit the pending store"
                    if self.pend[k, e] >= 0 and self.pend[k, e] in where and k < P:
                        self.seen.add("pending row overwritten by the call that flushes it")
                    sel[tok - base], row[tok - base] = PENDING, k * E + e
                    self.pend[k, e] = tok
                    self.pend_pos[tok] = (k, e)
        pend_len = np.array([0 if sync else len(r) for r in run], np.int32)
        return dict(sel=sel, row=row, flush_row=flush, counts=np.array(counts, np.int64), pend_len=pend_len, idx=idx)


def crafted_chunks(E, T, P, n_chunks, seed):
    """done uint8 / collisions int32 [n_chunks * T, E] of a continuous collection whose episodes are at most P ticks long: random
    lengths, a few envs forced -- env 0 ends twice in its first chunk, env 1 runs one episode across as many chunk boundaries as P
    allows, envs 2 .. 9 all end at tick 2 (several ends of both classes at one tick)."""
    rng = np.random.RandomState(seed)
    TT = n_chunks * T
    done, coll = np.zeros((TT, E), np.uint8), rng.randint(-2, 3, size=(TT, E)).astype(np.int32)
    for e in range(E):
        forced = {0: [2, 3], 1: [T - 2, min(P, T + 4)]}.get(e, [3] if 2 <= e <= 9 else [])
        t = 0
        while True:
            n = forced.pop(0) if forced else int(rng.randint(1, P + 1))
            t += n
            if t > TT:
                break
            done[t - 1, e] = 1
            coll[t - 1, e] = 0 if rng.rand() < 0.55 else int(rng.randint(1, 4))
    coll[2, 2:6], coll[2, 6:10] = 0, 3
    return done, coll


def crafted_sync(E, T, seed):
    """done / collisions / valid [T, E] of an episode-synchronous collection: valid up to each env's first done, envs 0 .. 4 never
    finish, envs 5 .. 7 had finished before the collection (no valid transition at all)."""
    rng = np.random.RandomState(seed)
    done = (rng.rand(T, E) < 0.25).astype(np.uint8)
    done[:, :5] = 0
    coll = rng.randint(0, 3, size=(T, E)).astype(np.int32)
    before = np.cumsum(done, 0) - done
    valid = (before == 0).astype(np.uint8)
    valid[:, 5:8] = 0
    return done, coll, valid
