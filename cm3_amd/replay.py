"""Device-side replay buffers and the reference's CSV log rows.

  replay_buffer.Replay_Buffer        alg/replay_buffer.py:1-37     ring of transitions, uniform sample_batch
  replay_buffer_dual.Replay_Buffer   alg/replay_buffer_dual.py:1-63  two rings split by an "is_bad" flag
                                     (particle: scenario.collisions != 0, train_onpolicy.py:356)
  log.csv / log_century.csv columns  alg/train_onpolicy.py:200-221, :399-429
Transitions are the columns ParticleRollout / CheckersRollout export (numpy=False): each ring stores one tensor per
column; adding a whole vectorised rollout is ONE launch (cm3_rows_scatter, or the export kernels of csrc/batch.hip writing ring rows),
sampling is one gather launch.
"""
import ctypes

import torch

from . import _lib
from ._lib import Cm3Error
from .rollout import CHECKERS_ORDER, check_columns, compact_specs, sample_distinct


class RingIndex(object):
    """The bookkeeping of replay_buffer.Replay_Buffer (alg/replay_buffer.py:11-16) without the data: where the next transitions
    go and how many are stored.  Host logic (tests/test_replay.py replays the reference's recorded memory with it)."""

    def __init__(self, size):
        self.maxsize = int(size)
        self.idx = 0
        self.len = 0

    def plan_add(self, n):
        """n sequential adds -> (skip, start, kept): the first `skip` of them are overwritten again by the later ones of the same
        batch (n > maxsize), the other `kept` land at ring positions start, start + 1, ... (mod maxsize)."""
        n = int(n)
        skip = max(0, n - self.maxsize)
        start = (self.idx + skip) % self.maxsize
        kept = n - skip
        self.idx = (self.idx + n) % self.maxsize
        self.len = min(self.len + n, self.maxsize)
        return skip, start, kept


def dual_take(n1, n2, size):
    """How many transitions replay_buffer_dual.Replay_Buffer.sample_batch(size) takes from memory_1 (bad) and memory_2 (good)
    holding n1 / n2 transitions (alg/replay_buffer_dual.py:40-63) -> (k1, all1, k2, all2): k sampled without replacement, or
    everything in storage order when the flag is set."""
    half = int(size / 2.0)
    if half <= n1 and half > n2:
        return min(n1, size - n2), False, n2, True
    if half > n1 and half <= n2:
        return n1, True, min(n2, size - n1), False
    if n1 < half and n2 < half:
        return n1, True, n2, True
    return half, False, half, False


class _Ring(object):
    """What the replay rings share: the ring index with its maxsize / idx / len surface, the stream, and the draw of sample_batch
    (replay_buffer.py:28-37)."""

    def __init__(self, size=int(1e6), device="cuda:0"):
        self.device = _lib.require_gpu(device)
        self.ring = RingIndex(size)
        self.cols = None

    maxsize = property(lambda self: self.ring.maxsize)
    idx = property(lambda self: self.ring.idx)
    len = property(lambda self: self.ring.len)

    def __len__(self):
        return self.ring.len

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _draw(self, n, generator, everything=False):
        """int64 [min(n, len)] distinct stored rows, uniformly at random; everything=True (sample_batch): None where len <= n --
        all of them, in storage order."""
        if everything and self.len <= n:
            return None
        return sample_distinct(self.len, min(int(n), self.len), 1, generator, self.device)[0].to(torch.int64).contiguous()


class DeviceReplayBuffer(_Ring):
    """replay_buffer.Replay_Buffer on the device: capacity `size` transitions, overwrite oldest when full
    (replay_buffer.py:11-16), sample_batch(size) = everything if len <= size else `size` distinct uniformly
    (:28-37).  One tensor per column; `add` is ONE launch for all columns (cm3_rows_scatter onto the ring positions),
    sampling ONE launch (cm3_rows_gather).  There is no host path: the buffer lives on an AMD GPU."""

    def _alloc(self, cols):
        if self.cols is None:
            self.cols = {k: torch.zeros((self.maxsize,) + tuple(v.shape[1:]), dtype=v.dtype, device=self.device) for k, v in cols.items()}
        elif set(cols) != set(self.cols):
            raise Cm3Error("replay columns changed: %s vs %s" % (sorted(cols), sorted(self.cols)))

    @staticmethod
    def _src(v, device):
        return v.to(device).contiguous()

    def add(self, cols):
        """cols: dict of tensors with a common leading batch dim (B transitions, in order)."""
        B = next(iter(cols.values())).shape[0]
        if B == 0:
            return
        self._alloc(cols)
        skip, start, kept = self.ring.plan_add(B)
        pairs = [(self.cols[k], self._src(v, self.device)[skip:]) for k, v in cols.items()]
        _lib.rows_scatter(pairs, kept, self._stream(), ring_start=start, ring_size=self.maxsize)

    def add_rollout(self, rollout):
        """All transitions of a continuous collection, straight from the trajectory into the ring: ONE launch (the export kernel with
        ring positions as its output rows) instead of an export followed by an add, and no intermediate copy of the phase.
        ParticleRollout (float32): cm3_transitions_gather_f32.  The reference stores the same array as v_global and v_local
        (train_onpolicy.py:338): so does the ring (one tensor under both names, rollout.ALIASES).
        CheckersRollout: cm3_checkers_transitions_gather; the ring holds the 16 columns of as_reference_batch(numpy=False) with their
        dtypes, so it is interchangeable with one that add() allocated."""
        B = rollout.T * rollout.env.E
        if B > self.maxsize:                                   # (more than the ring holds: the newest survive, as sequential adds leave)
            return self.add(rollout.as_reference_batch(numpy=False))
        cols = rollout.empty_columns(self.maxsize, zero=True) if self.cols is None else self.cols
        if not rollout.aliases_hold(cols):
            return self.add(rollout.as_reference_batch(numpy=False))      # (a ring that add() allocated: separate v_local storage)
        # (validate and launch FIRST, keep the ring and advance it after: an export that raises must not leave idx / len pointing at
        # rows that were never written -- ADVICE r5)
        rollout.export_into(cols, self.ring.idx, self.maxsize)
        self.cols = cols
        self.ring.plan_add(B)

    def add_at(self, cols, dst_row, n_added):
        """Rows b with dst_row[b] >= 0 go to ring position dst_row[b] (int64 on the device; computed by the caller, e.g. the dual
        buffer's split); the ring advances by n_added sequential adds."""
        self._alloc(cols)
        B = next(iter(cols.values())).shape[0]
        pairs = [(self.cols[k], self._src(v, self.device)) for k, v in cols.items()]
        _lib.rows_scatter(pairs, B, self._stream(), dst_row=dst_row)
        self.ring.plan_add(n_added)

    def _take(self, index):
        index = index.to(torch.int64).contiguous()
        n = index.numel()
        out = {k: torch.empty((n,) + tuple(v.shape[1:]), dtype=v.dtype, device=self.device) for k, v in self.cols.items()}
        if n:
            _lib.rows_gather([(out[k], self.cols[k]) for k in self.cols], n, index, self._stream())
        return out

    def all(self):
        """Everything stored, in storage order: VIEWS of the ring (no copy; the next add() overwrites them in place -- internal use,
        sample_batch() copies)."""
        return {k: v[:self.len] for k, v in self.cols.items()}

    def sample_batch(self, size, generator=None):
        index = self._draw(size, generator, everything=True)
        if index is None:
            # a COPY: all() hands out views of the ring, which the next add() overwrites in place -- the reference's
            # np.array(self.memory) is a copy, and a learner may still hold the batch when the next chunk is added
            return {k: v.clone() for k, v in self.all().items()}
        return self._take(index)

    def sample_n(self, n, generator=None):
        return self._take(self._draw(n, generator))


class CompactCheckersReplayBuffer(_Ring):
    """replay_buffer.Replay_Buffer for Checkers transitions with NARROW storage: the ring keeps every column with the dtype the
    trajectory keeps (grid / obs_self_t int8, vec int32, goals the uint8 goal index: 707 B per transition at the reference geometry
    where DeviceReplayBuffer's float64 columns take 3657 B) and only the rows a learner samples are widened.  The surface and the
    draws are DeviceReplayBuffer's, and sample_batch() returns exactly its 16 float64 / int32 / bool / int64 columns
    (CheckersRollout.ORDER), bit for bit: int8 -> float64 and int32 -> float64 are exact.
      add_rollout  ONE launch of cm3_checkers_transitions_pack (csrc/batch.hip), nothing converted;
      sampling     the draws of DeviceReplayBuffer, then ONE launch of cm3_checkers_ring_expand;
      add          the wide reference columns, narrowed with torch casts (a cold path; values that do not survive are refused).
    all() and sample_batch() below `size` return COPIES (expanded rows), never views of the ring.  `self.cols` are the compact
    columns."""

    def __init__(self, size=int(1e6), device="cuda:0"):
        super().__init__(size, device)
        self._wide = None        # name -> (row shape, dtype) of the columns sample_batch returns
        self._desc = None

    def _layout(self, wide):
        """wide: name -> (row shape, dtype) of the reference columns.  Fixes the geometry on first use; later it must agree."""
        wide = {k: (tuple(shape), dt) for k, (shape, dt) in wide.items()}
        if self._wide is not None:
            if wide != self._wide:
                raise Cm3Error("replay columns changed: %s vs %s" % (wide, self._wide))
            return
        if tuple(wide) != CHECKERS_ORDER:
            raise Cm3Error("a compact Checkers ring takes the 16 columns of CheckersRollout.ORDER, got %s" % (sorted(wide),))
        grid, obst = wide["grid"][0], wide["obs_self_t"][0]
        if len(grid) != 3 or grid[2] != 2 or len(obst) != 4 or obst[1] != obst[2] or obst[3] != 3 or obst[1] % 2 != 1:
            raise Cm3Error("grid must be [B, R, C + 1, 2] and obs_self_t [B, N, K, K, 3] with odd K: %s, %s" % (grid, obst))
        d = _lib.CheckersDesc()
        d.n_envs, d.n_agents, d.n_rows, d.n_columns, d.n_obs = 1, obst[0], grid[0], grid[1] - 1, (obst[1] - 1) // 2
        self._wide, self._desc = wide, d

    def _ring(self):
        if self.cols is None:
            return {k: torch.zeros((self.maxsize,) + shape, dtype=dt, device=self.device) for k, (shape, dt) in compact_specs(self._wide).items()}
        return self.cols

    def add_rollout(self, rollout):
        """All transitions of a continuous Checkers collection, straight from the trajectory into the compact ring: ONE launch
        (CheckersRollout.pack_into).  A chunk larger than the ring goes through add(): the newest transitions survive, as
        sequential adds leave them."""
        if not hasattr(rollout, "pack_into"):
            raise Cm3Error("a compact Checkers ring takes a CheckersRollout")
        B = rollout.T * rollout.env.E
        if B > self.maxsize:
            return self.add(rollout.as_reference_batch(numpy=False))
        self._layout(rollout.column_specs())
        cols = self._ring()
        # (validate and launch FIRST, keep the ring and advance it after, as DeviceReplayBuffer.add_rollout)
        rollout.pack_into(cols, self.ring.idx, self.maxsize)
        self.cols = cols
        self.ring.plan_add(B)

    def add(self, cols):
        """cols: the WIDE reference columns (what as_reference_batch(numpy=False) returns), B transitions in order.  They are narrowed
        here; a value that does not survive -- a grid / obs_self_t entry that is no int8, a vec entry that is no int32, goals that are
        not one-hot -- raises Cm3Error and leaves the ring as it was."""
        if set(cols) != set(CHECKERS_ORDER):
            raise Cm3Error("a compact Checkers ring takes the 16 columns of CheckersRollout.ORDER, got %s" % (sorted(cols),))
        wide = {k: cols[k].to(self.device) for k in CHECKERS_ORDER}
        B = wide["reward"].shape[0]
        if B == 0:
            return
        self._layout({k: (tuple(v.shape[1:]), torch.bool if k == "done" else v.dtype) for k, v in wide.items()})
        narrow = {}
        for name, (shape, dt) in compact_specs(self._wide).items():
            v = wide[name]
            if v.shape[0] != B:
                raise Cm3Error("column %s has %d rows, reward %d" % (name, v.shape[0], B))
            if name == "goals":
                if not bool(((v == 0) | (v == 1)).all()) or not bool((v.sum(-1) == 1).all()):
                    raise Cm3Error("goals must be one-hot pairs: the compact ring stores the goal index")
                c = v[..., 1].to(torch.uint8)
            elif name == "done":
                c = v.bool()
            else:
                c = v.to(dt)
                if dt != v.dtype and not torch.equal(c.to(v.dtype), v):
                    raise Cm3Error("column %s holds values that are no %s: the compact ring cannot store them" % (name, dt))
            narrow[name] = c
        ring = self._ring()
        # (launch FIRST, keep the ring and advance it after, as add_rollout: a scatter that raises leaves idx / len as they were)
        skip = max(0, B - self.maxsize)
        start, kept = (self.ring.idx + skip) % self.maxsize, B - skip
        _lib.rows_scatter([(ring[k], narrow[k][skip:].contiguous()) for k in ring], kept, self._stream(), ring_start=start,
                          ring_size=self.maxsize)
        self.cols = ring
        assert self.ring.plan_add(B) == (skip, start, kept)

    def _expand(self, index, out, what):
        """Rows index[b] (None: everything stored) of the ring as the 16 reference columns: ONE launch of cm3_checkers_ring_expand."""
        n = self.len if index is None else index.numel()
        if self.cols is None:
            raise Cm3Error("%s: the replay buffer is empty" % what)
        if out is None:
            out = {k: torch.empty((n,) + shape, dtype=dt, device=self.device) for k, (shape, dt) in self._wide.items()}
        else:
            check_columns(self._wide, out, n, self.device, "%s(out=...): pass the dict an earlier call returned for %d transitions" % (what, n))
            out = {k: out[k] for k in self._wide}
        if n:
            src = _lib.fill_checkers_cols(_lib.CheckersCompactCols(), self.cols, 0, self.maxsize)
            dst = _lib.fill_checkers_cols(_lib.CheckersTransitionCols(), out)
            _lib.check(_lib.lib().cm3_checkers_ring_expand(ctypes.byref(self._desc), ctypes.byref(src), _lib.ptr(index), int(n),
                                                           ctypes.byref(dst), self._stream()))
        return out

    def all(self):
        """Everything stored, in storage order, as the reference columns: a COPY by nature (the rows are widened) -- unlike
        DeviceReplayBuffer.all(), whose views the next add overwrites."""
        return self._expand(None, None, "all")

    def sample_batch(self, size, generator=None, out=None):
        """DeviceReplayBuffer.sample_batch: everything in storage order if len <= size, else `size` distinct rows uniformly (the
        same draws for the same len and generator state).  Fresh tensors, or with out= (a dict an earlier call returned for the same
        row count) those tensors written again: the persistent addresses a captured graph of the consumer needs."""
        index = self._draw(size, generator, everything=True)
        return self._expand(index, out, "sample_batch" if index is None else "sample_n")

    def sample_n(self, n, generator=None, out=None):
        return self._expand(self._draw(n, generator), out, "sample_n")


def _cat(a, b):
    if a is None:
        return b
    if b is None:
        return a
    return {k: torch.cat([a[k], b[k]], dim=0) for k in a}


class DeviceDualReplayBuffer(object):
    """replay_buffer_dual.Replay_Buffer: memory_1 holds transitions of "bad" episodes, memory_2 the others; a batch
    takes half from each when both have enough, else everything from the smaller one and the remainder from the larger
    (replay_buffer_dual.py:40-63).  `add` splits a whole batch by its flag column on the device: ranks by a prefix sum, ring
    positions for both memories, one scatter launch per memory -- one host read (the number of bad transitions).
    `add_rollout` is the reference's own feeding (train_onpolicy.py:300-356): WHOLE episodes, each contiguous and in time order, into
    the memory its flag at the episode's end names; the tail of an episode that is still running waits in a pending store."""

    def __init__(self, size=int(5e4), device="cuda:0"):
        self.mem1 = DeviceReplayBuffer(size, device)
        self.mem2 = DeviceReplayBuffer(size, device)
        self._carry = None       # continuous add_rollout: the env batch, its pending store (P rows per env) and pend_len [2][E]
        self._work = {}          # (T, E, P) -> the plan's device buffers

    def add(self, cols, is_bad):
        """is_bad: bool [B] per transition (all transitions of an episode carry the episode's flag; particle:
        scenario.collisions != 0, train_onpolicy.py:356)."""
        dev = self.mem1.device
        bad = torch.as_tensor(is_bad, device=dev).bool()
        B = bad.numel()
        # (before anything is launched or advanced: flags that do not match the rows would be ranked against other rows' positions)
        rows = {k: int(v.shape[0]) for k, v in cols.items()}
        if any(n != B for n in rows.values()):
            raise Cm3Error("add: %d flags for columns of %s rows (one flag per transition, in the columns' order)"
                           % (B, sorted(set(rows.values()))))
        if B == 0:
            return
        n1 = int(bad.sum())            # the one host read
        for mem, flag, n in ((self.mem1, bad, n1), (self.mem2, ~bad, B - n1)):
            if n == 0:
                continue
            rank = torch.cumsum(flag, 0) - 1                                   # order among the transitions of this memory
            keep = flag & (rank >= n - mem.maxsize)                             # (the earlier ones would be overwritten by this very batch)
            pos = torch.where(keep, (rank + mem.ring.idx) % mem.maxsize, torch.full_like(rank, -1))
            mem.add_at(cols, pos.contiguous(), n)

    # ---- whole episodes, straight from the trajectory (csrc/episode_route.hip, k_transitions_gather<RouteParams>) ----------------
    @property
    def pending(self):
        """Transitions add_rollout holds back: those of episodes that were still running at the end of the last chunk (a host read)."""
        return 0 if self._carry is None or self._carry["zero"] else int(self._carry["pend_len"][0].sum())

    def drop_pending(self):
        """Forgets the held-back transitions: for a caller that resets the envs between two chunks (their episodes never end), or
        that goes on with another env batch."""
        self._carry = None

    def _route_buffers(self, T, E, P):
        key = (T, E, P)
        if key not in self._work:
            dev = self.mem1.device
            nbytes = int(_lib.lib().cm3_episode_route_scratch_bytes(T, E))
            if nbytes == 0:
                raise Cm3Error("add_rollout: %d ticks x %d envs are more than one routing plan takes" % (T, E))
            self._work = {key: dict(sel=torch.empty(T * E, dtype=torch.uint8, device=dev), row=torch.empty(T * E, dtype=torch.int64, device=dev),
                                    flush=torch.empty(2, max(P, 1) * E, dtype=torch.int64, device=dev),
                                    counts=torch.zeros(2, dtype=torch.int64, device=dev),
                                    scratch=torch.empty(nbytes // 8, dtype=torch.int64, device=dev))}
        return self._work[key]

    def add_rollout(self, rollout):
        """All transitions of a ParticleRollout collection (float32, record_collisions=True), as replay_buffer_dual.Replay_Buffer
        receives them from the reference's trainers: whole episodes.  Episodes are taken in the order (end tick, env index) -- the
        order in which a host walking `for t: for e:` meets the done bytes; the episode that ends at (t, e) goes, oldest transition
        first and contiguously, to memory_1 when collisions[t][e] != 0, else to memory_2, each transition one sequential add (wrap at
        maxsize; when one call adds more than a ring holds the newest survive).
        Continuous collection: the transitions of an episode still running at the chunk's last tick enter neither ring.  They wait in
        a PENDING STORE (max_steps rows per env) and are added, in front of the rest of their episode, by the later call in which the
        episode ends -- so successive calls must collect from the same env batch (checked: the env object and its size);
        drop_pending() forgets them.  Episode-synchronous collection: only valid transitions exist, an env that has not finished by
        the last tick counts as ending there with its collision count so far (ParticleRollout.episode_is_bad), nothing pends.
        Device side: the routing plan (cm3_episode_route_plan: 5 launches), two cm3_rows_scatter that flush pending rows, ONE routed
        export launch that reads every transition once (no dense copy of the chunk), then ONE host read (the two counts)."""
        if not (hasattr(rollout, "route_into") and hasattr(rollout, "episode_is_bad")):
            raise Cm3Error("a dual replay buffer splits by the episodes' flag (scenario.collisions != 0, train_onpolicy.py:356): that is a "
                           "ParticleRollout's")
        if not rollout.kernel_export:
            raise Cm3Error("add_rollout needs a float32 trajectory (the export kernel); use add() with as_reference_batch()")
        if rollout.collisions is None:
            raise Cm3Error("the dual buffer's flag needs the per-tick collision counts (record_collisions=True)")
        if not rollout.collected:
            raise Cm3Error("add_rollout: nothing collected yet")
        env, T, dev = rollout.env, rollout.T, self.mem1.device
        if torch.device(env.device) != dev:
            raise Cm3Error("add_rollout: the buffer lives on %s, the rollout's envs on %s" % (dev, env.device))
        E, sync = env.E, not rollout.auto_reset
        rings = []
        for mem in (self.mem1, self.mem2):
            cols = rollout.empty_columns(mem.maxsize, zero=True) if mem.cols is None else mem.cols
            rollout._check_columns(cols, mem.maxsize, "add_rollout: a ring that add() allocated keeps separate v_local storage; the rings")
            rings.append(cols)
        carry = self._carry
        if sync:
            P, pend_in, pend_out, sets = 0, None, None, [(rings[0], self.mem1.maxsize), (rings[1], self.mem2.maxsize)]
            valid = rollout.valid.to(torch.uint8).contiguous()
        else:
            if carry is None:
                # (the pending store is as deep as the longest episode: pend_len[e] + the ticks to env e's next done never exceed it)
                P = int(env.max_steps)
                carry = dict(env=env, E=E, P=P, zero=True, store=rollout.empty_columns(P * E, zero=True),
                             pend_len=[torch.zeros(E, dtype=torch.int32, device=dev), torch.zeros(E, dtype=torch.int32, device=dev)])
            elif carry["env"] is not env or carry["E"] != E or int(env.max_steps) > carry["P"]:
                raise Cm3Error("add_rollout: pending transitions belong to another env batch (successive chunks must come from the same "
                               "envs: %d envs, max_steps <= %d); drop_pending() forgets them" % (carry["E"], carry["P"]))
            P, valid = carry["P"], None
            rollout._check_columns(carry["store"], P * E, "add_rollout: the pending store")
            pend_in, pend_out = carry["pend_len"]
            sets = [(rings[0], self.mem1.maxsize), (rings[1], self.mem2.maxsize), (carry["store"], P * E)]
        if (T + P) * E >= 1 << 31:
            raise Cm3Error("add_rollout: %d ticks and %d pending rows of %d envs are more than one routing plan takes" % (T, P, E))
        w = self._route_buffers(T, E, P)
        d = _lib.EpisodeRouteDesc()
        d.done, d.done_stride = rollout.done.data_ptr(), E
        d.collisions, d.collisions_stride = rollout.collisions.data_ptr(), E * 4
        d.valid, d.valid_stride = _lib.ptr(valid), E
        d.n_ticks, d.n_envs, d.pending_depth, d.synchronous = T, E, P, int(sync)
        d.ring_idx[0], d.ring_idx[1], d.ring_size[0], d.ring_size[1] = self.mem1.idx, self.mem2.idx, self.mem1.maxsize, self.mem2.maxsize
        stream = env._stream()
        # (launch FIRST, keep the rings and advance after, as DeviceReplayBuffer.add_rollout: whatever raises leaves idx / len and the
        # current pend_len as they were -- the plan writes the new pend_len into the spare array)
        _lib.check(_lib.lib().cm3_episode_route_plan(ctypes.byref(d), _lib.ptr(pend_in), _lib.ptr(pend_out), w["sel"].data_ptr(),
                                                     w["row"].data_ptr(), w["flush"].data_ptr(), w["counts"].data_ptr(),
                                                     w["scratch"].data_ptr(), w["scratch"].numel() * 8, stream))
        if not sync and not carry["zero"]:
            # BEFORE the export: it may overwrite pending rows of an env whose next episode starts in this chunk
            for c in (0, 1):
                pairs = [(rings[c][k], carry["store"][k]) for k in rings[c] if k not in rollout.ALIASES]
                _lib.rows_scatter(pairs, P * E, stream, dst_row=w["flush"][c])
        rollout.route_into(sets, w["sel"], w["row"])
        n1, n2 = w["counts"].tolist()                     # the one host read
        self.mem1.cols, self.mem2.cols = rings
        self.mem1.ring.plan_add(n1)
        self.mem2.ring.plan_add(n2)
        if not sync:
            carry["pend_len"].reverse()
            carry["zero"] = False
            self._carry = carry
        return n1, n2

    def sample_batch(self, size, generator=None):
        n1, n2 = len(self.mem1), len(self.mem2)
        k1, all1, k2, all2 = dual_take(n1, n2, size)
        a = (self.mem1.all() if all1 else self.mem1.sample_n(k1, generator)) if n1 and k1 else None
        b = (self.mem2.all() if all2 else self.mem2.sample_n(k2, generator)) if n2 and k2 else None
        if a is None or b is None:          # (_cat would hand out the one side as is: ring views when it is "everything")
            one = a if b is None else b
            return None if one is None else {k: v.clone() for k, v in one.items()}
        return _cat(a, b)


def off_policy_batches(rollout, buffer, n_chunks, batch_size=128, generator=None, whole_episodes=False, **collect_kwargs):
    """The off-policy cadence of alg/train_offpolicy.py:309-356 (the trainer the reference's README routes Checkers to): every
    transition goes into a PERSISTENT replay buffer (:337-346), and every `steps_per_train` env steps (:348) a batch is sampled
    from it (:350) for a training step.  Vectorised: `rollout` (a ParticleRollout / CheckersRollout in continuous mode with
    n_ticks = steps_per_train) collects one chunk of ticks for all its envs, all transitions of the chunk are added to `buffer`
    (DeviceReplayBuffer, or for Checkers a CompactCheckersReplayBuffer -- a fifth of the memory, the same batches: ONE launch) and
    one batch is sampled -- yielded as device columns; `collect_kwargs` go to
    rollout.collect() (policy=..., epsilon=..., goals=... for Checkers; policy= a ParticleQmixAgent / CheckersQmixAgent is the
    QMIX baseline's collection, train_offpolicy.py:319 / :317 with use_qmix = 1).  The buffer outlives the chunks: old transitions are
    overwritten only when it is full (replay_buffer.py:11-16).
    whole_episodes=True (a DeviceDualReplayBuffer): the chunk goes in through buffer.add_rollout -- whole episodes in the order
    (end tick, env), each in the memory its flag at its END names, unfinished tails carried to the next chunk: what the reference's
    class holds.  The default splits every chunk at once by the flag so far (head and tail of an episode may part)."""
    dual = isinstance(buffer, DeviceDualReplayBuffer)
    if whole_episodes and not dual:
        raise Cm3Error("whole_episodes=True is the dual replay buffer's feeding (DeviceDualReplayBuffer.add_rollout)")
    if dual and not hasattr(rollout, "episode_is_bad"):
        raise Cm3Error("a dual replay buffer splits by the episodes' flag (scenario.collisions != 0, train_onpolicy.py:356): that is a "
                       "ParticleRollout's; use a DeviceReplayBuffer here")
    for _ in range(int(n_chunks)):
        rollout.collect(**collect_kwargs)
        if dual and whole_episodes:
            buffer.add_rollout(rollout)
        elif dual:
            # every transition carries the flag of the episode it belongs to: the flag is known at the tick that ENDS the episode
            # (ParticleRollout.episode_is_bad); transitions of episodes still running at the chunk's end take the flag so far.
            # One flag per EXPORTED row, in the export's order (an episode-synchronous export holds the valid transitions only)
            cols = rollout.as_reference_batch(numpy=False)
            buffer.add({k: v.contiguous() for k, v in cols.items()}, _transition_flags(rollout))
        elif rollout.auto_reset and rollout.kernel_export and hasattr(buffer, "add_rollout"):
            buffer.add_rollout(rollout)                                   # export + add in one launch
        else:
            cols = rollout.as_reference_batch(numpy=False)
            buffer.add({k: v.contiguous() for k, v in cols.items()})
        yield buffer.sample_batch(batch_size, generator=generator)


def _transition_flags(rollout):
    """One bool per row of as_reference_batch(), in its order (time-major).  Continuous collection: [T * E], transition (t, e) is
    "bad" when the episode it belongs to has collided by its end inside this chunk -- or by the chunk's last tick, for an episode that
    runs on.  Episode-synchronous collection: one per VALID transition (valid_indices()), the flag of its env's one episode
    (episode_is_bad(): at the tick that ends it, or the count so far for an env still running at the last tick) -- the rule of
    DeviceDualReplayBuffer.add_rollout's synchronous mode."""
    coll = rollout.collisions                       # int32 [T, E]: scenario.collisions after every tick (before a same-launch reset)
    if coll is None:
        raise Cm3Error("the dual buffer's flag needs the per-tick collision counts (record_collisions=True)")
    if not rollout.auto_reset:
        _, ee = rollout.valid_indices()
        return rollout.episode_is_bad()[ee]
    done = rollout.done.bool()
    T = coll.shape[0]
    bad_at_end = (coll != 0)
    flag = torch.empty_like(done)
    run = bad_at_end[T - 1].clone()                 # episodes still running at the end of the chunk: their count so far
    for t in range(T - 1, -1, -1):
        run = torch.where(done[t], bad_at_end[t], run)
        flag[t] = run
    return flag.reshape(-1)


class CsvLog(object):
    """The reference's two CSV logs with identical headers and row formats (train_onpolicy.py:200-221, :399-429)."""

    def __init__(self, log_path, century_path, n_agents):
        self.log_path, self.century_path, self.n = log_path, century_path, int(n_agents)
        header = "Step,Episode,r_global" + "".join(",r_%d" % i for i in range(self.n)) + "\n"
        header_c = ("Step,Century,r_global_avg" + "".join(",r_avg_%d" % i for i in range(self.n)) + ",r_global_eval"
                    + "".join(",r_eval_%d" % i for i in range(self.n)) + ",r_eval_local,t_env (s),t_train(s)\n")
        with open(self.log_path, "w") as f:
            f.write(header)
        with open(self.century_path, "w") as f:
            f.write(header_c)

    @staticmethod
    def episode_row(step, idx_episode, reward_global, reward_local):
        return "%d,%d,%.2f," % (step, idx_episode, reward_global) + ",".join("{:.2f}".format(v) for v in reward_local) + "\n"

    @staticmethod
    def century_row(step, idx_episode, r_global_avg, r_local_avg, r_global_eval, r_local_eval, t_env, t_train):
        s = "%d,%d,%.2f," % (step, idx_episode, r_global_avg)
        s += ",".join("{:.2f}".format(v) for v in r_local_avg)
        s += ",%.2f," % r_global_eval
        s += ",".join("{:.2f}".format(v) for v in r_local_eval)
        s += ",%.2f,%d,%d\n" % (float(sum(r_local_eval)), int(t_env), int(t_train))
        return s

    def log_episode(self, *a):
        with open(self.log_path, "a") as f:
            f.write(self.episode_row(*a))

    def log_century(self, *a):
        with open(self.century_path, "a") as f:
            f.write(self.century_row(*a))
