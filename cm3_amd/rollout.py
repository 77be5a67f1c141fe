"""Trajectory collection -- the `while not done` loop of alg/train_onpolicy.py:281-350 for E envs.

The reference appends one object-array row per tick to a Python list (replay_buffer.py:11-16):
  particle (11 columns, train_onpolicy.py:338)
    [global_state, obs_others, obs_self, actions, reward, local_rewards,
     next_global_state, next_obs_others, next_obs_self, done, goals]
  Checkers (16 columns, train_onpolicy.py:336)
    [grid, vec, obs_others, obs_self_t, obs_self_v, actions_prev, actions, reward, local_rewards,
     next_grid, next_vec, next_obs_others, next_obs_self_t, next_obs_self_v, done, goals]
Here the trajectory lives on the device, time-major and de-duplicated: slot t of the state /
observation arrays is "before tick t", slot t+1 is "after tick t", so `next_*` of transition t is
slot t+1 (or the captured terminal state when the env was re-initialised in the same launch).  The
step kernel writes slot t+1 directly (zero-copy, cm3_particle_rollout_*).  ``as_reference_batch``
gathers any set of (tick, env) pairs into exactly what ``np.stack(batch[:, k])`` yields in
alg_credit.process_batch (alg_credit.py:458-470) / alg_credit_checkers.process_batch
(alg_credit_checkers.py:427-444), and ``as_reference_rows`` rebuilds the reference's object rows so
the real ``process_batch`` consumes them unchanged.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import FLAG_AUTO_RESET, FLAG_GEN_ACTIONS, Cm3Error


def rows_from_columns(cols, order):
    """Object ndarray [B, len(order)]: row b = the reference's per-tick np.array([...fields...]) of
    train_onpolicy.py:336/:338 (dtype=object, which NumPy >= 1.24 requires for ragged rows), so that
    ``np.stack(rows[:, k])`` in the reference's process_batch returns cols[order[k]]."""
    B = len(cols[order[0]])
    rows = np.empty((B, len(order)), dtype=object)
    for k, name in enumerate(order):
        col = cols[name]
        for b in range(B):
            rows[b, k] = col[b]
    return rows


def _to_numpy(cols):
    return {k: v.detach().cpu().numpy() for k, v in cols.items()}


def _is_device_policy(policy):
    """An on-device agent (cm3_amd.actor / cm3_amd.qmix: enqueue() launches it on a stream) rather than a host callable."""
    return hasattr(policy, "enqueue") and hasattr(policy, "act")


PARTICLE_ORDER = ("v_global", "obs_others", "v_local", "actions", "reward", "reward_local", "v_global_next",
                  "obs_others_next", "v_local_next", "done", "goals")
CHECKERS_ORDER = _lib.CHECKERS_COLUMNS
# Checkers record -> (wide dtype: the reference's columns, trajectory dtype: what the trajectory and a compact ring keep); the goals
# record is the uint8 goal index, its wide form the one-hot int64 pair (one more dimension of 2)
_F64, _I32 = (torch.float64,) * 2, (torch.int32,) * 2
CHECKERS_DTYPES = dict(grid=(torch.float64, torch.int8), vec=(torch.float64, torch.int32), obs_others=_F64, obs_self_t=(torch.float64, torch.int8),
                       obs_self_v=_F64, actions=_I32, reward=_F64, local_rewards=_F64, done=(torch.bool,) * 2, goals=(torch.int64, torch.uint8))


def _valid_from_done(done_u8, finished0=None):
    """valid[t, e] = env e had not finished before tick t (episode-synchronous collection: an env that
    finishes early stops producing transitions, like the reference's `while not done`).  finished0 (bool [E]):
    envs whose episode had already ended when this collection started (the collector carries that across
    collect(reset=False) calls on an env without auto-reset) produce no valid transition at all."""
    d = done_u8.to(torch.int32)
    finished_before = torch.cumsum(d, dim=0) - d
    valid = finished_before == 0
    if finished0 is not None:
        valid = valid & ~finished0.unsqueeze(0)
    return valid


def _pairs_aligned(pairs):
    return all((d.numel() * d.element_size()) % 16 == 0 and d.data_ptr() % 16 == 0 and s_.data_ptr() % 16 == 0
               and d.is_contiguous() and s_.is_contiguous() and d.numel() * d.element_size() == s_.numel() * s_.element_size()
               for d, s_ in pairs)


def _copy_pairs(pairs, stream):
    """(dst, src) tensor pairs ON `stream`: ONE cm3_copy_list launch per 8 regions when every region is 16-byte sized /
    aligned, torch copies otherwise -- issued on `stream` too (an ExternalStream context), so that they are ordered with the
    launches around them and, while `stream` is being captured into a hipGraph, become nodes of that graph instead of
    running once, unordered, at capture time."""
    ok = _pairs_aligned(pairs)
    if ok:
        for k in range(0, len(pairs), 8):
            _lib.copy_list(pairs[k:k + 8], stream)
    else:
        dev = pairs[0][0].device
        # (handle 0 = the legacy default stream: torch.cuda.ExternalStream(0) would hand out a fresh POOL stream instead)
        ts = torch.cuda.ExternalStream(int(stream), device=dev) if stream else torch.cuda.default_stream(dev)
        with torch.cuda.stream(ts):
            for d, s_ in pairs:
                d.copy_(s_)


def _one_launch_hooks(policy):
    """(applies(env), enqueue(...)) of the whole-rollout Checkers kernel that runs `policy`, or None.  CheckersActor's pair
    (fused_rollout_ok / enqueue_rollout) is what policy_mode "auto" looks for; CheckersQmixAgent's (episode_ok /
    enqueue_episode) runs under policy_mode "episode" only."""
    if hasattr(policy, "enqueue_rollout"):
        return policy.fused_rollout_ok, policy.enqueue_rollout
    if hasattr(policy, "enqueue_episode"):
        return policy.episode_ok, policy.enqueue_episode
    return None


def _one_launch_refusal(policy, env):
    """Why the whole-rollout Checkers kernel does not run `policy` on `env`: the first failed condition, in words."""
    who = type(policy).__name__
    if _one_launch_hooks(policy) is None:
        return "%s has no one-launch rollout kernel" % who
    if getattr(policy, "precision", None) != "f16x3":
        return ("precision: the one-launch rollout kernel runs the split-float16 network (precision='f16x3'); this %s has "
                "precision=%r, which runs as launch pairs (policy_mode='tick')" % (who, getattr(policy, "precision", None)))
    if env.n != policy.n or env.n not in (1, 2):
        return ("agent count: the one-launch rollout kernel covers one or two agents, the env's and the policy's alike; env has %d, "
                "%s %d -- other counts run as launch pairs (policy_mode='tick')" % (env.n, who, policy.n))
    if hasattr(policy, "stage") and (policy.stage > 1) != (env.n > 1):
        return "agent count: a stage-%d %s does not match an env with %d agent(s)" % (policy.stage, who, env.n)
    if (policy.seed & 0xFFFFFFFFFFFFFFFF) != int(env._desc.seed) or policy.env_id_base != int(env._desc.env_id_base):
        return ("seed / env_id_base: the one-launch rollout kernel draws for policy and env under one Philox key; %s has seed %d, "
                "env_id_base %d, the env seed %d, env_id_base %d" % (who, policy.seed, policy.env_id_base, int(env._desc.seed),
                                                                      int(env._desc.env_id_base)))
    return "geometry: the one-launch rollout kernel needs the 3 x 8 band, n_obs 2 and 4-byte padded records"


_Mode = collections.namedtuple("_Mode", "kind live sparse")

# ParticleRollout(partial_tiles=True), policy_mode="auto": per agent count with padded tiles, the largest batch (envs) up to which the
# one-launch rollout was measured faster than the launch pairs -- "auto" takes the one launch up to there and the pairs beyond (see
# ParticleRollout._mode; 0 would mean never).  Measured at f16x3 on one MI355X, profiles/r21_policy_partial_tiles.txt.
#   3, 5, 6, 7 agents: faster at 1024, 4096, 16384 and 65536 envs (the largest measured; 33.5 / 46.7, 64.4 / 84.6, 96.6 / 105.1,
#                       99.5 / 118.5 us per tick there: the one launch's slowest round / the pairs' fastest round)
#   9 agents:           faster at 1024, 4096 (18.4 / 26.0) and 8192 (35.8 / 40.5), NOT at 16384 (69.9 against 69.3)
#   10 agents:          faster at 1024 and 4096 (21.9 / 27.6); 8192 is a tie (42.9 / 43.0, inside the arm-to-arm spread) and 16384 a
#                       loss (84.0 against 79.9): the bound stays at 4096
PARTIAL_TILES_AUTO = {3: 65536, 5: 65536, 6: 65536, 7: 65536, 9: 8192, 10: 4096}


def partial_tiles_auto(n_agents, n_envs):
    """Does policy_mode="auto" of ParticleRollout(partial_tiles=True) take the one launch at this padded-tile shape?"""
    return n_envs <= PARTIAL_TILES_AUTO.get(n_agents, 0)


def _policy_rollout_entry(lib, dtype):
    """cm3_policy_rollout_f32 / _f64 (the one-launch policy kernel) by the env's real."""
    return lib.cm3_policy_rollout_f64 if dtype == torch.float64 else lib.cm3_policy_rollout_f32


class _CapturedGraph(object):
    """Owner of ONE executable hipGraph: captured on the first launch() after construction or destroy(), replayed by every
    launch(), destroyed only after the device has drained."""

    def __init__(self, device):
        self.device = device
        self.graph = None
        self._lib = _lib.lib()

    def launch(self, capture, stream):
        if self.graph is None:
            self.graph = _lib.capture_graph(self.device, capture)
        _lib.check(self._lib.cm3_graph_launch(self.graph, stream))

    def destroy(self):
        if self.graph is not None:
            torch.cuda.synchronize(self.device)     # a previous replay may still be in flight
            self._lib.cm3_graph_destroy(self.graph)
            self.graph = None


class _ActorGraphCache(_CapturedGraph):
    """One captured (actor launch, step launch) x T graph per rollout object.  The key is the policy OBJECT (a strong
    reference: `id()` of a collected actor can be reused); epsilon is not part of it -- the actor launches read it from
    a device float that collect() refreshes, so the annealing of train_onpolicy.py:369 never triggers a re-capture."""

    def __init__(self, device):
        super().__init__(device)
        self.policy = self.key = None
        self.eps = torch.zeros(1, dtype=torch.float32, device=device)

    def launch(self, policy, epsilon, capture, stream, key=None):
        """key: anything else the captured launches bake in (the per-tick fused policy kernel takes epsilon by value)."""
        self.eps.fill_(float(epsilon))          # ordered before the replay on the same stream
        if self.policy is not policy or self.key != key:
            self.destroy()
            self.policy, self.key = policy, key
        super().launch(capture, stream)

    def destroy(self):
        super().destroy()
        self.policy = None


def check_columns(specs, columns, rows, device, what):
    """Every column of `specs` (name -> (row shape, dtype)) present in `columns` as a contiguous tensor [rows, ...] on `device` with
    that row shape and dtype (done: bool or uint8): what a kernel that writes through the raw pointers relies on."""
    for name, (shape, dt) in specs.items():
        t = columns.get(name) if hasattr(columns, "get") else None
        ok_dt = (torch.bool, torch.uint8) if name == "done" else (dt,)
        if (not torch.is_tensor(t) or not t.is_cuda or t.device != device or not t.is_contiguous() or t.dim() != 1 + len(shape)
                or t.shape[0] != rows or tuple(t.shape[1:]) != shape or t.dtype not in ok_dt):
            raise Cm3Error("%s: column %s must be a contiguous tensor [%d%s] of %s on %s" %
                           (what, name, rows, "".join(", %d" % d for d in shape), dt, device))


def compact_specs(specs):
    """The compact form of the Checkers column specs (name -> (row shape, dtype)): every column with the dtype the trajectory keeps --
    grid / obs_self_t int8, vec int32, goals the uint8 goal index instead of the one-hot int64 pair -- the others as they are."""
    record = dict(_lib.CHECKERS_COLUMN_RECORDS)
    out = {}
    for name, (shape, dt) in specs.items():
        wide, kept = CHECKERS_DTYPES[record[name]]
        out[name] = (shape[:-1] if record[name] == "goals" else shape, dt if wide == kept else kept)
    return out


class _Transitions(object):
    """What ParticleRollout and CheckersRollout share once a trajectory is collected: which transitions are valid, their export as the
    reference's columns (one launch, into fresh tensors, the caller's, or ring rows), draws over them, the one-launch export of a whole
    phase of minibatches -- and the ownership of the captured graphs.  The class supplies T, env, auto_reset, done, ORDER,
    column_specs(), _gather(tt, ee, B, columns, ring_start, ring_size), as_reference_batch_torch(tt, ee, numpy) and `_graphs`."""

    last_sample_positions = None
    ALIASES = {}                # column -> the column whose tensor it shares (the reference stores one array under both names)
    kernel_export = True        # the export kernel (_gather) applies to this trajectory; else as_reference_batch_torch does the work
    _finished0 = None

    def _drop_graphs(self):
        for g in self._graphs:
            g.destroy()

    def close(self):
        self._drop_graphs()

    @property
    def valid(self):
        """bool [T, E]"""
        if self.auto_reset:
            return torch.ones(self.T, self.env.E, dtype=torch.bool, device=self.env.device)
        return _valid_from_done(self.done, self._finished0)

    def valid_indices(self):
        """(tt, ee) int64 tensors of all valid transitions, time-major."""
        idx = self.valid.nonzero(as_tuple=False)
        return idx[:, 0], idx[:, 1]

    def empty_columns(self, rows, zero=False):
        """The columns of ORDER with `rows` rows each (what as_reference_batch(numpy=False) returns; a replay ring when zero=True);
        aliased names share one tensor."""
        make = torch.zeros if zero else torch.empty
        cols = {}
        for name, (shape, dt) in self.column_specs().items():
            cols[name] = (cols[self.ALIASES[name]] if name in self.ALIASES
                          else make((int(rows),) + shape, dtype=dt, device=self.env.device))
        return cols

    def aliases_hold(self, columns):
        """Every aliased name of `columns` is the tensor of the column it stands for (the kernel writes each distinct column once)."""
        return all(a in columns and b in columns and columns[a].data_ptr() == columns[b].data_ptr() for a, b in self.ALIASES.items())

    def _check_columns(self, columns, rows, what, specs=None):
        """Every column a contiguous device tensor [rows, ...] of the right row shape and dtype: the kernel writes rows * row bytes
        through each pointer, a wrong layout would be an out-of-bounds device write."""
        check_columns(self.column_specs() if specs is None else specs, columns, rows, self.done.device, what)
        if not self.aliases_hold(columns):
            raise Cm3Error("%s: %s must be the tensors of %s" % (what, ", ".join(self.ALIASES), ", ".join(self.ALIASES.values())))

    def as_reference_batch(self, tt=None, ee=None, numpy=True, out=None):
        """Columns of the reference's transition batch for the (tick, env) pairs (tt, ee) (default: all valid ones), each equal to
        np.stack(batch[:, k]) in the reference's process_batch.  ONE launch of the class's export kernel (_gather) fills all of them;
        where it does not apply (kernel_export) the torch composition as_reference_batch_torch does: same values.
        out: a dict this call returned earlier for the same number of transitions (numpy=False): the columns are written into those
        tensors again (persistent addresses: what a captured hipGraph of the consumer needs)."""
        dev = self.env.device
        everything = tt is None and self.auto_reset and self.kernel_export    # (all T x E transitions are valid: b = t E + e, no index arrays)
        if tt is None and not everything:
            tt, ee = self.valid_indices()
        if not everything:
            tt = torch.as_tensor(tt, device=dev, dtype=torch.long).contiguous()
            ee = torch.as_tensor(ee, device=dev, dtype=torch.long).contiguous()
        if not self.kernel_export:
            return self.as_reference_batch_torch(tt, ee, numpy)
        if not everything and tt.shape != ee.shape:
            raise Cm3Error("as_reference_batch: tt and ee must have the same shape")
        B = self.T * self.env.E if everything else tt.numel()
        if out is not None:
            if numpy:
                raise Cm3Error("as_reference_batch(out=...) returns the device tensors of `out`: pass numpy=False")
            self._check_columns(out, B, "as_reference_batch(out=...): pass the dict an earlier call returned for %d transitions" % B)
            cols = {name: out[name] for name in self.ORDER}
        else:
            cols = self.empty_columns(B)
        self._gather(None if everything else tt, None if everything else ee, B, cols)
        return _to_numpy(cols) if numpy else cols

    def _ring_chunk(self, what, columns, ring_start, ring_size, specs=None):
        """What export_into and CheckersRollout.pack_into (`what`: the one called) check before their launch: a continuous collection,
        a ring that takes its T * E transitions, every column.  Returns the number of transitions."""
        if not (self.auto_reset and self.kernel_export):
            raise Cm3Error("%s needs a continuous collection (every transition valid) that the export kernel reads" % what)
        B, ring_start, ring_size = self.T * self.env.E, int(ring_start), int(ring_size)
        if not (0 <= ring_start < ring_size and B <= ring_size):
            raise Cm3Error("%s: ring of %d rows from row %d does not take %d transitions" % (what, ring_size, ring_start, B))
        self._check_columns(columns, ring_size, what, specs)
        return B

    def export_into(self, columns, ring_start, ring_size):
        """Every transition of the trajectory (continuous collection the export kernel applies to) written straight into the rows
        (ring_start + b) mod ring_size of `columns` -- a dict with the tensors of as_reference_batch(numpy=False), each with ring_size
        rows: export and replay add in ONE launch (DeviceReplayBuffer.add_rollout).  Every column is checked before the launch.
        Returns the number of transitions."""
        B = self._ring_chunk("export_into", columns, ring_start, ring_size)
        self._gather(None, None, B, columns, ring_start, ring_size)
        return B

    def as_reference_rows(self, tt=None, ee=None):
        """Object ndarray [B, len(ORDER)]: row b is the reference's np.array([...fields...]) of train_onpolicy.py:336 / :338
        (dtype=object, as NumPy >= 1.24 requires for ragged rows)."""
        return rows_from_columns(self.as_reference_batch(tt, ee), self.ORDER)

    def _sample_positions(self, size, rows, generator):
        """int64 [rows, k] positions into the valid transitions (time-major), each row `size` distinct ones uniformly at random
        (random.sample, replay_buffer.py:34), or all of them when there are <= size -- and the (tt, ee) of all valid transitions,
        None when every transition is valid (continuous collection: position b = t E + e, nothing to enumerate)."""
        if self.auto_reset:
            n, tt, ee = self.T * self.env.E, None, None
        else:
            tt, ee = self.valid_indices()
            n = tt.numel()
        if n <= size:
            return torch.arange(n, device=self.env.device).unsqueeze(0).expand(rows, n), tt, ee
        return sample_distinct(n, size, rows, generator, self.env.device), tt, ee

    def sample_batch(self, size, generator=None, numpy=True):
        """replay_buffer.sample_batch (replay_buffer.py:28-37): all transitions if there are <= size of them,
        else `size` distinct ones uniformly at random."""
        pos, tt, ee = self._sample_positions(size, 1, generator)
        pos = pos[0]
        if tt is None:
            E = self.env.E
            if pos.numel() == self.T * E:
                return self.as_reference_batch(numpy=numpy)
            return self.as_reference_batch(torch.div(pos, E, rounding_mode="floor"), pos % E, numpy=numpy)
        return self.as_reference_batch(tt[pos], ee[pos], numpy=numpy)

    def on_policy_minibatches(self, epochs=24, batch_size=128, generator=None, numpy=False):
        """The on-policy cadence of train_onpolicy.py:359-377: after a collection phase, `epochs` minibatches of
        `batch_size` transitions are sampled from the freshly collected buffer, which is then discarded (the next
        collect() overwrites the trajectory).  The reference collects episodes_per_train = 10 episodes (<= 330
        transitions) per phase; a vectorised phase holds n_envs episodes.
        All minibatches of the phase are drawn together and exported by ONE launch (round 5: 24 separate samples cost 24 permutations
        of the phase's 1.35 M transitions, 7 ms against the 0.8 ms of collecting them); each yielded dict holds views of that export."""
        cols, k = self._phase_export(epochs, batch_size, generator)
        for m in range(int(epochs)):
            mb = {name: v[m * k:(m + 1) * k] for name, v in cols.items()}
            yield (_to_numpy(mb) if numpy else mb)

    def _phase_export(self, epochs, batch_size, generator, out=None):
        """-> (columns of all `epochs` minibatches back to back [epochs * k, ...], k = transitions per minibatch): one draw, one launch"""
        epochs = int(epochs)
        pos, tt, ee = self._sample_positions(batch_size, epochs, generator)
        self.last_sample_positions = pos          # (tests: which transitions the minibatches hold)
        k = pos.shape[1]
        flat = pos.reshape(-1)
        if tt is None:
            E = self.env.E
            cols = self.as_reference_batch(torch.div(flat, E, rounding_mode="floor"), flat % E, numpy=False, out=out)
        else:
            cols = self.as_reference_batch(tt[flat], ee[flat], numpy=False, out=out)
        return cols, k


class ParticleRollout(_Transitions):
    """T-tick trajectory over a VecParticleEnv.

    env.auto_reset False: episode-synchronous -- reset all envs, run T = max_steps ticks, transitions of
        an env after its `done` are flagged invalid (mirrors one reference episode per env).
    env.auto_reset True: continuous -- finished envs restart inside the launch; the true terminal
        next-state/obs are captured per tick, goals are recorded per slot; every transition is valid.
    """

    def __init__(self, env, n_ticks=None, use_graph=True, fused=False, record_collisions=True,
                 fused_policy_tick=False, live_state=None, policy_mode="auto", sparse_goals=None, partial_tiles=False):
        self.env = env
        self.T = int(n_ticks or env.max_steps)
        self.use_graph = bool(use_graph)
        # fused: the random-action branch runs all T ticks in ONE launch (CM3_FLAG_FUSED_TICKS; state in
        # registers, identical results).  Policy-driven collection always launches once per tick.
        self.fused = bool(fused)
        # fused_policy_tick: policy-driven collection with ONE launch per tick -- actor forward pass, sampling and env step of
        # a tick in one cm3_policy_rollout_f32 launch (n_ticks = 1) instead of an actor launch followed by a step launch;
        # bit-identical to both other policy modes (float32 envs: any n_agents; float64 envs: n_agents in {1, 2, 4, 8})
        self.fused_policy_tick = bool(fused_policy_tick)
        # policy_mode: how collect(policy=<device actor>) launches (all three are bit-identical, tests/test_gpu_actor.py):
        #   "episode"  the whole policy-driven episode in ONE launch (csrc/policy.hip) -- the fastest (C2: 5.6 vs 10.6 us per tick);
        #   "tick"     an actor launch and a step launch per tick inside one hipGraph;
        #   "auto"     (default, round 3) "episode" whenever the fused kernel applies -- n_agents in {1, 2, 4, 8} (float64 envs: 1, 2, 4),
        #              actor.seed == env.seed (one Philox key) -- else "tick".  fused=True / fused_policy_tick=True
        #              still force their modes.
        # A ParticleQmixAgent runs as launch pairs in every mode unless it was built with episode_kernel=True: then "episode" and,
        # where eligible, "auto" run ITS one-launch rollout (kind qmix_episode in _mode); fused / fused_policy_tick stay refused.
        if policy_mode not in ("auto", "episode", "tick"):
            raise Cm3Error("policy_mode must be 'auto', 'episode' or 'tick'")
        self.policy_mode = policy_mode
        # partial_tiles (opt-in): policy_mode "episode" and "auto" also consider the one-launch kernel at n_agents 3, 5, 6, 7, 9, 10
        # -- 16-row wave tiles that hold 16 // n_agents whole envs and pad rows (csrc/policy_tiles.h); CM3 actor, float32 envs,
        # actor.seed == env.seed; the same bits as the launch pairs (tests/test_gpu_policy_partial_tiles.py).  "episode" then runs
        # it at every such n_agents, "auto" where PARTIAL_TILES_AUTO says it was measured faster.  Without the keyword those agent
        # counts run as launch pairs and "episode" refuses them, as ever.  (fused=True / fused_policy_tick=True call the same
        # entry and need no keyword.)
        self.partial_tiles = bool(partial_tiles)
        # live_state: None = by size (see collect); True / False force stepping in place on the env's buffers with slot copies /
        # chaining the ticks through the slots.  Identical trajectories either way (tests/test_gpu_rollout.py).
        self.live_state = live_state
        # sparse_goals: random-action collection at streaming sizes writes a goals slot only where an env restarts (landmarks move
        # only at an episode start; cm3_particle_traj.goals_live alone) instead of all of them every tick -- 7 % of the bytes of a
        # tick that runs at the chip's copy rate (profiles/r04_trajectory_stream.txt).  None = by size (see collect), True / False
        # force it.  `goals` (and as_reference_batch) look the same either way: the dense array is filled in on first access.
        self.sparse_goals = sparse_goals
        self._goals_sparse = False
        self._graph_mode = None          # the _Mode the captured graphs were built with (+ the env's buffer parity when live)
        self.n_captures = 0              # hipGraph captures of the random-action collection so far (tests)
        self._goal_src = None
        self._goal_src32 = self._goal_src32_of = None
        E, N, L, T, dev, dt = env.E, env.n, env.L, self.T, env.device, env.dtype
        z = lambda *s, d=dt: torch.zeros(*s, dtype=d, device=dev)  # noqa: E731
        self.state = z(T + 1, N, E, 4)
        self.obs_others = z(T + 1, E, N, L)
        self.actions = z(T, E, N, d=torch.int32)
        self.reward = z(T, E)
        self.reward_n = z(T, E, N)
        self.done = z(T, E, d=torch.uint8)
        self.auto_reset = env.auto_reset
        if self.auto_reset:
            self._goals_buf = z(T + 1, N, E, 2)
            self.term_state = z(T, N, E, 4)
            self.term_obs_others = z(T, E, N, L)
        else:
            self._goals_buf = None
            self.term_state = self.term_obs_others = None
        # scenario.collisions after every tick, before any same-launch reset: the per-episode value the reference reads
        # at train_onpolicy.py:356 sits at the tick that ends the episode
        # (record_collisions=False drops the slot: episode_is_bad() is then unavailable)
        self.collisions = z(T, E, d=torch.int32) if record_collisions else None
        # the captured graphs: collect()'s random-action rollout, collect_normalized()'s whole step, the actor / step launch pairs
        self._graph, self._norm_graph, self._actor_graph = _CapturedGraph(dev), _CapturedGraph(dev), _ActorGraphCache(dev)
        self._graphs = (self._norm_graph, self._graph, self._actor_graph)
        self._norm = self._norm_key = None       # collect_normalized's ReturnsNormalizer and the arguments it was built for
        self._live, self._live_cur = False, env._cur
        # packed live records (cm3_particle_traj.live_record): one 128-byte line per env that the per-tick random-action live-state
        # launches of the pair kernel step on (float32, 2..4 agents); allocated once, its address is part of the graphs' key
        self._record = (torch.zeros(E, 32, dtype=torch.int32, device=dev)
                        if env.dtype == torch.float32 and 2 <= N <= 4 and self._goals_buf is not None else None)
        # episode-synchronous mode: which envs' episodes have ended since their last reset (carried across collects)
        self._finished = torch.zeros(E, dtype=torch.bool, device=dev)
        self._finished0 = None
        self._lib = _lib.lib()
        self.collected = False
        if hasattr(env, "_rollouts"):
            env._rollouts.add(self)          # env.reset() / env.set_state() outside the collector clear `_finished` (mark_reset)

    def mark_reset(self, mask=None):
        """Envs (bool / uint8 [E] mask; None = all) were re-seeded outside this collector -- env.reset(mask), env.set_state():
        their next episode is fresh, so transitions collected with reset=False are valid again.  VecParticleEnv calls this
        itself; call it by hand only for an env object that does not."""
        if mask is None:
            self._finished.zero_()
        else:
            m = torch.as_tensor(mask, device=self.env.device).bool().reshape(-1)
            self._finished &= ~m

    # ---- plumbing ------------------------------------------------------------------------------------
    def _record_for(self, flags, live):
        """The record tensor when the launches of `flags` step on packed live records, else None: live state, and a descriptor the
        library takes them for (float32, in-kernel actions, a launch per tick, 2..4 agents, the pair kernel steps this batch)."""
        if not live or self._record is None:
            return None
        env = self.env
        env._desc.flags = flags
        ok = self._lib.cm3_particle_live_record_applies(ctypes.byref(env._desc), self.state.element_size())
        return self._record if ok else None

    def _traj(self, t0=0, live=False, sparse_goals=False, record=None):
        """live: per-tick launches step IN PLACE on the env's own state / goals buffers and write every tick's state / goals
        to its slot as a copy (cm3_particle_traj.state_live): a tick then loads lines its predecessor read and overwrote
        instead of a fresh slot that was only ever written -- 0.19 us of 2.83 per tick at C2 (tools/trajectory_gap.py)."""
        env, es = self.env, self.state.element_size()
        E, N, L = env.E, env.n, env.L
        t = _lib.ParticleTraj()
        if live:
            t.state_live = env._state[env._cur].data_ptr()
            t.goals_live = env._goals.data_ptr()
            if record is not None:
                t.live_record = record.data_ptr()
        t.state = self.state[t0].data_ptr()
        t.state_stride = N * E * 4 * es
        if self._goals_buf is not None:
            t.goals = self._goals_buf[t0].data_ptr()
            t.goals_stride = N * E * 2 * es
            if sparse_goals:
                t.goals_live = env._goals.data_ptr()
        else:
            t.goals = env._goals.data_ptr()
            t.goals_stride = 0
        t.obs_others = self.obs_others[t0].data_ptr()
        t.obs_others_stride = E * N * L * es
        t.actions = self.actions[t0].data_ptr()
        t.actions_stride = E * N * 4
        t.reward_n = self.reward_n[t0].data_ptr()
        t.reward_n_stride = E * N * es
        t.reward = self.reward[t0].data_ptr()
        t.reward_stride = E * es
        t.done = self.done[t0].data_ptr()
        t.done_stride = E
        t.meta = env._meta.data_ptr()
        t.episode = env._episode.data_ptr()
        if self.term_state is not None:
            t.term_state = self.term_state[t0].data_ptr()
            t.term_state_stride = N * E * 4 * es
            t.term_obs_others = self.term_obs_others[t0].data_ptr()
            t.term_obs_others_stride = E * N * L * es
        if self.collisions is not None:
            t.collisions = self.collisions[t0].data_ptr()
            t.collisions_stride = E * 4
        return t

    def _enqueue(self, t0, n, flags, stream=None, live=False, sparse_goals=False, record=None):
        env = self.env
        env._desc.flags = flags
        traj = self._traj(t0, live, sparse_goals, record)
        stream = env._stream() if stream is None else stream
        fn = getattr(self._lib, "cm3_particle_rollout_" + env._suffix)
        _lib.check(fn(ctypes.byref(env._desc), ctypes.byref(traj), int(n), stream))

    def _enqueue_tick0_from_env(self, flags, stream):
        """Tick 0 as a plain step launch that READS the env's own state / goals buffers (not slot 0) and writes slot 1 and the
        per-tick slots 0: the copy that records slot 0 then no longer stands between the caller and the first step launch
        (collect_normalized runs it on a parallel branch of its graph).  Values are those of `_enqueue(0, 1, ...)`."""
        env = self.env
        b = _lib.ParticleBufs()
        b.state_in = env._state[env._cur].data_ptr()
        b.state_out = self.state[1].data_ptr()
        b.goals_in = env._goals.data_ptr()
        b.goals_out = self._goals_buf[1].data_ptr() if self._goals_buf is not None else env._goals.data_ptr()
        b.meta_in = b.meta_out = env._meta.data_ptr()
        b.episode = env._episode.data_ptr()
        b.actions = self.actions[0].data_ptr()
        b.obs_others = self.obs_others[1].data_ptr()
        b.reward_n = self.reward_n[0].data_ptr()
        b.reward = self.reward[0].data_ptr()
        b.done = self.done[0].data_ptr()
        if self.term_state is not None:
            b.term_state = self.term_state[0].data_ptr()
            b.term_obs_others = self.term_obs_others[0].data_ptr()
        if self.collisions is not None:
            b.collisions_tick = self.collisions[0].data_ptr()
        env._desc.flags = flags
        fn = getattr(self._lib, "cm3_particle_step_" + env._suffix)
        _lib.check(fn(ctypes.byref(env._desc), ctypes.byref(b), stream))

    def _copy(self, pairs):
        """(dst, src) tensor pairs: one cm3_copy_list launch when every region is 16-byte sized / aligned."""
        _copy_pairs(pairs, self.env._stream())

    def _slot0_pairs(self):
        """(dst, src): slot 0 <- the env's current buffers."""
        env = self.env
        pairs = [(self.state[0], env._state[env._cur]), (self.obs_others[0], env._obs_others[env._cur])]
        if self._goals_buf is not None:
            pairs.append((self._goals_buf[0], env._goals))
        return pairs

    def _store_back_pairs(self, live):
        """(dst, src): the env's current buffers <- slot T."""
        env = self.env
        pairs = [(env._obs_others[env._cur], self.obs_others[self.T])]
        if not live:    # (live: the env's state / goals buffers ARE the final state)
            pairs.append((env._state[env._cur], self.state[self.T]))
            if self._goals_buf is not None and not self._goals_sparse:     # (sparse goal slots: the live goals array is current)
                pairs.append((env._goals, self._goals_buf[self.T]))
        return pairs

    def _load_slot0(self):
        self._copy(self._slot0_pairs())

    def _store_back(self, live=False):
        self._copy(self._store_back_pairs(live))

    # ---- collection ------------------------------------------------------------------------------------
    def _enqueue_actor_rollout(self, actor, epsilon, base_flags, stream):
        """T x (actor launch, step launch) on `stream`: the policy reads slot t, writes actions[t]; the step kernel
        consumes them and writes slot t+1 (train_onpolicy.py:311-323 without leaving the device)."""
        env = self.env
        live = self._live
        for t in range(self.T):
            goals = self._goals_buf[t] if (self._goals_buf is not None and not live) else env._goals   # (live: goals in place)
            actor.enqueue(env.E, self.obs_others[t], self.state[t], goals, env._meta, env._episode, self.actions[t],
                          epsilon, stream=stream, env_id_base=env.env_id_base, dtype=env.dtype)
            self._enqueue(t, 1, base_flags, stream, live=live)

    def _enqueue_fused_policy_ticks(self, actor, epsilon, base_flags, stream):
        """T launches of the fused policy kernel, one tick each (slot t -> slot t+1)."""
        env = self.env
        env._desc.flags = base_flags & FLAG_AUTO_RESET
        ad = actor._desc(env.E, epsilon, env.env_id_base)
        fn = _policy_rollout_entry(self._lib, env.dtype)
        for t in range(self.T):
            traj = self._traj(t)
            _lib.check(fn(ctypes.byref(env._desc), ctypes.byref(traj), ctypes.byref(ad), ctypes.byref(actor._wt), None, 0, 1, stream))

    def _streaming(self):
        """The trajectory is streaming-size: >= 128 MB of observation slots (see _mode)."""
        env = self.env
        return env.E * env.n * env.L * self.state.element_size() * self.T >= (128 << 20)

    def _wants_live_state(self):
        """The live-state size rule of _mode -- a tick's state <= 1 MiB and a streaming-size trajectory -- unless live_state forces it."""
        if self.live_state is not None:
            return bool(self.live_state)
        return self.env.n * self.env.E * 4 * self.state.element_size() <= (1 << 20) and self._streaming()

    def _mode(self, policy):
        """How this collect() launches -- the one place that decides it.  -> _Mode(kind, live, sparse):
          kind    random_fused | random            the reference's random-action branch, all ticks in one launch / a launch per tick
                  policy_episode                   on-device actor, the whole episode in ONE launch (csrc/policy.hip)
                  policy_fused_tick | policy_tick  on-device actor, one fused launch / an actor + a step launch per tick
                                                   (a policy with fused_kernels = False, the QMIX agent: policy_tick only ...
                  qmix_episode                     ... unless it was built with episode_kernel=True: the QMIX agent's whole rollout
                                                   in ONE launch (csrc/policy.hip, QMIX mode).  policy_mode="episode" runs it or
                                                   raises with the first failed condition (float32 env, n_agents in {1, 2, 4, 8},
                                                   policy.n == env.n, policy.seed == env.seed); "auto" runs it where eligible (it
                                                   was faster at every measured size), launch pairs otherwise; "tick" is launch
                                                   pairs; fused=True / fused_policy_tick=True are refused as for the default agent)
                  host_policy                      a Python callable per tick
          live    per-tick step launches step IN PLACE on the env's buffers and copy every tick's state to its slot -- only while a
                  tick's state is small (<= 1 MiB: the slot copy is extra write traffic, the gain is load latency: C2 2.87 -> 2.74 us)
                  and the trajectory is streaming-size (>= 128 MB of observation slots: a small trajectory collected over and over stays
                  cache-resident and the copies only cost); measured in profiles/r02_trajectory_gap_live_state.txt,
                  r03_live_state_crossover.txt.  live_state = True / False forces it.
          sparse  goal slots are written only where an env restarts: always with live state (the goals live in place), and for the
                  random-action branch at streaming sizes (sparse_goals = True / False forces that)."""
        env = self.env
        dev_policy = _is_device_policy(policy)
        if dev_policy and env.dtype not in (torch.float32, torch.float64):
            raise Cm3Error("the device actor reads float32 or float64 env buffers")
        same_key = dev_policy and getattr(policy, "seed", None) == env.seed
        if policy is None:
            kind = "random_fused" if self.fused else "random"
        elif not dev_policy:
            kind = "host_policy"
        elif not getattr(policy, "fused_kernels", True):
            # an agent the CM3 actor's one-launch kernels do not run (ParticleQmixAgent): launch pairs, unless the agent opted in to
            # its own one-launch rollout (episode_kernel=True: cm3_policy_rollout_qmix_f32, the same bits as the pairs)
            opted = bool(getattr(policy, "episode_kernel", False))
            if self.fused or self.fused_policy_tick or (self.policy_mode == "episode" and not opted):
                raise Cm3Error("%s runs as an agent launch plus a step launch per tick: policy_mode='episode', fused=True and "
                               "fused_policy_tick=True run the CM3 actor" % type(policy).__name__)
            kind = "policy_tick"
            if opted and self.policy_mode != "tick":
                # "auto" takes the one launch wherever it is eligible: at every measured size its slowest round beat the pairs'
                # fastest round of the same run -- C2 3.55 against 8.00 us per tick, C5 12.75 against 17.06, 65 536 x 4 36.7 against
                # 40.6 (profiles/r18_qmix_particle_episode.txt) -- so there is no size rule, unlike the f64 N = 8 case below
                why = policy.episode_refusal(env)
                if why is None:
                    kind = "qmix_episode"
                elif self.policy_mode == "episode":
                    raise Cm3Error("policy_mode='episode': " + why)
        else:
            dense = env.n in (1, 2, 4, 8)
            # partial_tiles=True: the padded-tile builds of the kernel -- float32 envs only (no float64 build of them exists)
            padded = self.partial_tiles and not dense and env.dtype == torch.float32 and 1 <= env.n <= 10
            episode_ok = (dense or padded) and same_key and not self.fused_policy_tick
            # "auto" leaves float64 envs of eight agents to the launch pairs: measured at C5 (8192 x 8, f16x3) the f64 one-launch
            # episode runs 40.8 us per tick against 33.5 (its 64-row build needs 83.7 KB of LDS: one workgroup per CU;
            # profiles/r07_policy_f64.txt).  policy_mode="episode" still runs it.
            auto_ok = episode_ok and not (env.dtype == torch.float64 and env.n == 8)
            # ... and a padded-tile agent count goes to the one launch only where PARTIAL_TILES_AUTO holds it (the criterion of
            # profiles/r18_qmix_particle_episode.txt: its slowest round beat the pairs' fastest round of the same run;
            # profiles/r21_policy_partial_tiles.txt).  policy_mode="episode" runs the kernel at every such count.
            auto_ok = auto_ok and (dense or partial_tiles_auto(env.n, env.E))
            if self.fused or (self.policy_mode == "episode" and episode_ok) or (self.policy_mode == "auto" and auto_ok):
                kind = "policy_episode"
            elif self.policy_mode == "episode" and self.partial_tiles:
                raise Cm3Error("policy_mode='episode' with partial_tiles=True needs a float32 env where n_agents is outside "
                               "{1, 2, 4, 8} (the padded-tile builds are float32 only), n_agents <= 10 and actor.seed == env.seed")
            elif self.policy_mode == "episode":
                raise Cm3Error("policy_mode='episode' needs n_agents in {1, 2, 4, 8} and actor.seed == env.seed")
            else:
                kind = "policy_fused_tick" if self.fused_policy_tick else "policy_tick"
            if kind in ("policy_episode", "policy_fused_tick") and not same_key:
                raise Cm3Error("fused policy launches need actor.seed == env.seed (one Philox key)")
        stream_size, small = self._streaming(), self._wants_live_state()
        per_tick_steps = kind in ("random", "policy_tick", "host_policy") and not self.fused
        live = bool(self._goals_buf is not None and small and per_tick_steps)
        sparse = bool(self._goals_buf is not None and kind != "random_fused" and (
            live or (kind == "random" and bool(stream_size if self.sparse_goals is None else self.sparse_goals))))
        return _Mode(kind, live, sparse)

    def collect(self, policy=None, reset=None, epsilon=0.0):
        """Runs T ticks.  policy None = the reference's random-action branch (train_onpolicy.py:305-307,
        drawn in-kernel; the whole rollout is one hipGraph replay); otherwise ``policy(obs_others [E,N,L],
        obs_self [E,N,4], goals [E,N,2]) -> int actions [E,N]`` is called every tick (:311-313).
        reset: None -> reset at the start iff the env does not auto-reset."""
        env = self.env
        if reset is None:
            reset = not self.auto_reset
        if reset:
            env.reset()
            self._finished.zero_()
        # envs whose episode already ended in an earlier collect (no auto-reset, reset=False) stay invalid
        self._finished0 = None if self.auto_reset else self._finished.clone()
        self._load_slot0()
        base = (FLAG_AUTO_RESET if self.auto_reset else 0) | env.kernel_flags
        mode = self._mode(policy)
        live, sparse = mode.live, mode.sparse
        self._live = live
        # packed live records: the per-tick random-action launches only (every other mode reads the env's buffers between ticks)
        record = self._record_for(base | FLAG_GEN_ACTIONS, live) if mode.kind == "random" else None
        # ONE key for every captured graph of this object: the mode, plus the env's buffer parity where the launches hold the
        # addresses of the env's current buffers (live state; env.step() flips them) and the record's address where they hold that
        key = (mode, env._cur if live else None, record.data_ptr() if record is not None else None)
        if self._graph_mode is not None and self._graph_mode != key:
            self._drop_graphs()
        self._graph_mode = key
        if self._live_cur != env._cur:
            self._drop_norm_graph()       # (collect_normalized's graph reads the env's current buffers in every mode)
            self._live_cur = env._cur
        # `_goals_sparse` only says whether the goal slots of the LAST collection still need completing (the `goals` getter clears it)
        self._goals_sparse, self._goal_src = sparse, None
        stream = env._stream()
        if mode.kind == "random_fused":
            self._enqueue(0, self.T, base | FLAG_GEN_ACTIONS | _lib.FLAG_FUSED_TICKS)
        elif mode.kind == "random":
            flags = base | FLAG_GEN_ACTIONS
            if self.use_graph:
                self.n_captures += int(self._graph.graph is None)
                self._graph.launch(lambda s: self._enqueue(0, self.T, flags, s, live=live, sparse_goals=sparse, record=record), stream)
            else:
                self._enqueue(0, self.T, flags, live=live, sparse_goals=sparse, record=record)
        elif mode.kind == "policy_episode":
            # the whole policy-driven episode in ONE launch (csrc/policy.hip): weights, observation tile and env state stay in
            # LDS / registers for all T ticks; bit-identical to alternating actor / step launches
            env._desc.flags = base & FLAG_AUTO_RESET
            traj = self._traj(0)
            ad = policy._desc(env.E, epsilon, env.env_id_base)
            fn = _policy_rollout_entry(self._lib, env.dtype)
            _lib.check(fn(ctypes.byref(env._desc), ctypes.byref(traj), ctypes.byref(ad), ctypes.byref(policy._wt), None, 0, self.T,
                          stream))
        elif mode.kind == "qmix_episode":
            # the QMIX agent's whole rollout in ONE launch (csrc/policy.hip, QMIX mode; no graph): bit-identical to alternating
            # agent / step launches.  epsilon: a float or a 0-dim float32 device tensor, read by the launch
            env._desc.flags = base & FLAG_AUTO_RESET
            policy.enqueue_episode(env._desc, self._traj(0), env.E, self.T, epsilon, stream=stream)
        elif mode.kind == "policy_fused_tick":
            if self.use_graph:      # epsilon is a by-value argument of these launches: part of the graph's key
                self._actor_graph.launch(policy, epsilon, lambda s: self._enqueue_fused_policy_ticks(policy, epsilon, base, s),
                                         stream, key=("fused_tick", float(epsilon)))
            else:
                self._enqueue_fused_policy_ticks(policy, epsilon, base, stream)
        elif mode.kind == "policy_tick":
            if self.use_graph:
                cache = self._actor_graph
                cache.launch(policy, epsilon, lambda s: self._enqueue_actor_rollout(policy, cache.eps, base, s), stream)
            else:
                self._enqueue_actor_rollout(policy, epsilon, base, stream)
        else:                       # a host policy: one call and one step launch per tick
            for t in range(self.T):
                goals = (self._goals_buf[t] if (self._goals_buf is not None and not live) else env._goals).permute(1, 0, 2)
                a = policy(self.obs_others[t], self.state[t].permute(1, 0, 2), goals)
                self.actions[t].copy_(torch.as_tensor(a, device=env.device).reshape(env.E, env.n))
                self._enqueue(t, 1, base, live=live)
        self._store_back(live)
        if not self.auto_reset:
            self._finished |= self.done.bool().any(0)
        self.collected = True
        return self

    def collect_normalized(self, gamma=0.99, eps=1e-8, normalize=True, group=None, time_collective=False, segments=1):
        """Random-action collection (continuous mode) FOLLOWED by the advantage-normalisation step over reward_n -- BASELINE
        configs[3]: discounted returns + this rank's float64 moments, ONE 24-byte all-gather over the ranks, normalisation
        with the global statistics (cm3_amd.shard).  With one rank the collective is the identity and the whole step --
        slot copy in, T step launches, slot copy out, returns + moments, normalise -- is ONE hipGraph replay; with several
        ranks the graph ends at the moments, the all-gather and the normalise launch follow eagerly (RCCL / gloo).
        Returns (normalised returns [T,E,N], (mean, std, count) device scalars); with time_collective=True also the seconds
        the host spent in the all-gather call (0.0 for one rank).
        segments = K > 1 (round 4): the T ticks are K consecutive rollouts of T / K ticks -- one collection phase
        (train_onpolicy.py:359: episodes_per_train rollouts between two training steps) -- each with its own returns and its own
        normalisation statistics ((mean, std, count) become [K] tensors); the K advantage steps are the same two launches at the
        end of ONE chain of T step launches, the whole phase one hipGraph replay, and with several ranks the K moment triples
        travel in ONE all-gather.  Values per rollout are bit-identical to K calls with segments = 1 on a T / K-tick collector."""
        import time
        from .shard import ReturnsNormalizer, gather_moments
        import torch.distributed as dist
        env = self.env
        if not self.auto_reset or self.fused:
            raise Cm3Error("collect_normalized runs the continuous, one-launch-per-tick random-action collection")
        world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
        key = (float(gamma), float(eps), bool(normalize), world > 1, int(segments))
        if self._norm_key != key:
            self._drop_norm_graph()
            self._norm = ReturnsNormalizer(self.reward_n, self.done, gamma, eps, normalize, segments=segments)
            self._norm_key = key
        self._finished0 = None
        live = self._live = self._wants_live_state()
        flags = FLAG_AUTO_RESET | env.kernel_flags | FLAG_GEN_ACTIONS
        record = self._record_for(flags, live)      # (the live branch steps on packed live records where they apply, as collect does)
        key_mode = (live, live, record.data_ptr() if record is not None else None)
        if self._graph_mode is not None and self._graph_mode != key_mode:
            self._drop_graphs()
        self._graph_mode = key_mode
        self._goals_sparse, self._goal_src = live, None      # (the live-state launches write a goals slot only where an env restarts)
        # The captured graph bakes in the addresses of env._state[env._cur] / env._obs_others[env._cur] (tick 0 reads them, the
        # slot bookkeeping writes them) -- live or not -- and VecParticleEnv.step() flips env._cur: re-capture after a flip.
        if self._live_cur != env._cur:
            self._drop_graphs()
            self._live_cur = env._cur

        def enqueue(s):
            pairs, back = self._slot0_pairs(), self._store_back_pairs(live)      # (what _load_slot0 / _store_back copy)
            if not live and world == 1 and _pairs_aligned(pairs + back):
                # one rank, one graph: tick 0 reads the env's buffers directly (not slot 0), and the launch that computes the
                # returns and their partial moments also records slot 0 from the env's buffers and then leaves slot T in them --
                # the chain of dependent launches is T step launches + 2, not T + 4
                self._enqueue_tick0_from_env(flags, s)
                if self.T > 1:
                    self._enqueue(1, self.T - 1, flags, s, live=False)
                self._norm.enqueue_fused(s, [(self.state[0], env._state[env._cur], self.state[self.T]),
                                             (self.obs_others[0], env._obs_others[env._cur], self.obs_others[self.T]),
                                             (self._goals_buf[0], env._goals, self._goals_buf[self.T])])
                return
            _copy_pairs(pairs, s)
            self._enqueue(0, self.T, flags, s, live=live, record=record)
            _copy_pairs(back, s)
            if world == 1:
                self._norm.enqueue_fused(s)        # (= enqueue_moments + enqueue_normalize on the own moments, bit for bit)
            else:
                self._norm.enqueue_moments(s)

        stream = env._stream()
        if self.use_graph:
            self._norm_graph.launch(enqueue, stream)
        else:
            enqueue(stream)
        t_coll = 0.0
        if world > 1:
            t0 = time.perf_counter()
            parts, n_parts = gather_moments(self._norm.moments, group)
            t_coll = time.perf_counter() - t0
            self._norm.enqueue_normalize(stream, parts, n_parts)
        self.collected = True
        st = self._norm.stats
        res = (self._norm.out, (st[0], st[1], st[2]) if st.dim() == 1 else (st[:, 0], st[:, 1], st[:, 2]))
        return res + (t_coll,) if time_collective else res

    def _drop_norm_graph(self):
        self._norm_graph.destroy()

    # ---- views --------------------------------------------------------------------------------------------
    @property
    def goals(self):
        """[T + 1, N, E, 2] landmark positions per slot (None for an episode-synchronous collector: they do not change).  After a
        collection with sparse goal slots the array is completed here, once, on first access."""
        if self._goals_sparse:
            idx = self._goal_source_slots().view(self.T + 1, 1, self.env.E, 1).expand_as(self._goals_buf)
            self._goals_buf.copy_(self._goals_buf.gather(0, idx))
            self._goals_sparse = False
        return self._goals_buf

    @goals.setter
    def goals(self, value):
        self._goals_buf, self._goals_sparse = value, False

    def _goal_source_slots(self):
        """int64 [T + 1, E]: the slot that holds the goals in effect at slot t of env e -- the last slot <= t that was written
        (slot 0, or slot k + 1 of a tick k that ended an episode)."""
        if self._goal_src is None:
            T, E = self.T, self.env.E
            src = torch.zeros(T + 1, E, dtype=torch.int64, device=self.env.device)
            ticks = torch.arange(1, T + 1, device=self.env.device, dtype=torch.int64).view(T, 1)
            src[1:] = torch.where(self.done.bool(), ticks, torch.zeros_like(ticks))
            self._goal_src = torch.cummax(src, dim=0).values
        return self._goal_src

    def episode_is_bad(self):
        """The reference's dual-buffer flag `scenario.collisions != 0` per finished episode (train_onpolicy.py:356), read
        from the per-tick collision counts of the trajectory at the tick that ENDS the episode -- collisions of an env
        that is stepped on after its `done` (episode-synchronous mode) do not count, as in the reference, whose loop
        stops there (:302).
        Episode-synchronous mode: bool [E]; an env still running at the end of this trajectory reports its count so far.
        Continuous mode: bool [T, E], set only where ``done`` is set (the count of the episode that ended at that tick,
        captured before the same-launch reset zeroes the live counter)."""
        if self.collisions is None:
            raise Cm3Error("episode_is_bad() needs ParticleRollout(record_collisions=True)")
        d = self.done.bool()
        if self.auto_reset:
            return (self.collisions != 0) & d
        T = self.T
        first = torch.where(d.any(0), d.to(torch.uint8).argmax(0), torch.full_like(d[0], T - 1, dtype=torch.long))
        return self.collisions.gather(0, first.unsqueeze(0)).squeeze(0) != 0

    def episode_returns(self):
        """(reward_global [E], reward_local [E,N]) accumulated over each env's episode
        (train_onpolicy.py:349-350); episode-synchronous mode."""
        v = self.valid.to(self.reward.dtype)
        return (self.reward * v).sum(0), (self.reward_n * v.unsqueeze(2)).sum(0)

    def _next(self, name, tt, ee):
        """next_* of transitions (tt, ee): slot t+1, or the captured terminal values where the env restarted."""
        if name == "state":
            nxt = self.state[tt + 1, :, ee]                    # [B, N, 4]
            if self.term_state is not None:
                term = self.term_state[tt, :, ee]
                d = self.done[tt, ee].bool().view(-1, 1, 1)
                nxt = torch.where(d, term, nxt)
            return nxt
        nxt = self.obs_others[tt + 1, ee]
        if self.term_obs_others is not None:
            term = self.term_obs_others[tt, ee]
            d = self.done[tt, ee].bool().view(-1, 1, 1)
            nxt = torch.where(d, term, nxt)
        return nxt

    ORDER = PARTICLE_ORDER
    ALIASES = {"v_local": "v_global", "v_local_next": "v_global_next"}      # (one array under both names, train_onpolicy.py:338)
    _COLS_FIELDS = (("state", "v_global"), ("obs_others", "obs_others"), ("actions", "actions"), ("reward", "reward"),
                    ("reward_n", "reward_local"), ("next_state", "v_global_next"), ("next_obs_others", "obs_others_next"),
                    ("done", "done"), ("goals", "goals"))                   # cm3_transition_cols field <- column
    kernel_export = property(lambda self: self.state.dtype == torch.float32)

    def column_specs(self):
        """name -> (row shape, dtype) of the 11 columns of as_reference_batch(numpy=False) of a float32 trajectory, in ORDER."""
        N, L, f32 = self.env.n, self.env.L, torch.float32
        specs = dict(v_global=((N, 4), f32), obs_others=((N, L), f32), actions=((N,), torch.int32), reward=((), f32),
                     reward_local=((N,), f32), v_global_next=((N, 4), f32), obs_others_next=((N, L), f32), done=((), torch.bool),
                     goals=((N, 2), f32))
        specs.update({alias: specs[name] for alias, name in self.ALIASES.items()})
        return {name: specs[name] for name in self.ORDER}

    def _goal_slots32(self):
        """The sparse-goal argument of the export kernel: _goal_source_slots() as int32 [T + 1, E], converted once per collection;
        None while the goal slots are dense."""
        if self._goals_buf is None or not self._goals_sparse:
            return None
        if self._goal_src32 is None or self._goal_src32_of is not self._goal_source_slots():
            self._goal_src32_of = self._goal_source_slots()
            self._goal_src32 = self._goal_src32_of.to(torch.int32)
        return self._goal_src32

    def _gather(self, tt, ee, B, columns, ring_start=0, ring_size=0):
        """ONE launch of cm3_transitions_gather_f32 (csrc/batch.hip) fills all of `columns` (checked by the caller); float32
        trajectories only -- the float64 parity instantiation goes through the torch composition below (as_reference_batch_torch: same
        values, ~25 launches)."""
        env = self.env
        traj = self._traj(0)
        goal_slot = self._goal_slots32()
        out = _lib.TransitionCols()
        for field, name in self._COLS_FIELDS:
            setattr(out, field, columns[name].data_ptr())
        out.ring_start, out.ring_size = int(ring_start), int(ring_size)
        _lib.check(self._lib.cm3_transitions_gather_f32(ctypes.byref(env._desc), ctypes.byref(traj), _lib.ptr(goal_slot),
                                                        0 if goal_slot is None else env.E * 4, _lib.ptr(tt), _lib.ptr(ee), int(B),
                                                        ctypes.byref(out), env._stream()))

    def route_into(self, sets, sel, row):
        """Every transition of the trajectory written to row row[b] of the column set sets[sel[b]] (b = t E + e; sel[b] >= len(sets):
        nowhere) in ONE launch of cm3_transitions_route_f32 -- the routed form of export_into, which DeviceDualReplayBuffer.add_rollout
        feeds with the plan of cm3_episode_route_plan: the two rings and the pending store.  sets: 1..3 (columns, rows) pairs, each
        `columns` a dict with the tensors of as_reference_batch(numpy=False) with `rows` rows (checked before the launch); sel uint8
        and row int64 [T * E] on the device.  row is NOT bounds-checked: derive it from sizes you own.  Works for both collection
        modes (an episode-synchronous trajectory has no terminal capture: next_* is slot t + 1)."""
        if not self.kernel_export:
            raise Cm3Error("route_into needs a float32 trajectory (the export kernel)")
        env, B = self.env, self.T * self.env.E
        dev = self.done.device
        if not 1 <= len(sets) <= 3:
            raise Cm3Error("route_into: 1..3 column sets")
        for t, dt, name in ((sel, torch.uint8, "sel"), (row, torch.int64, "row")):
            if not (torch.is_tensor(t) and t.dtype == dt and t.device == dev and t.is_contiguous() and t.numel() == B):
                raise Cm3Error("route_into: %s must be a contiguous %s tensor of %d elements on %s" % (name, dt, B, dev))
        out = (_lib.TransitionCols * len(sets))()
        for k, (columns, rows) in enumerate(sets):
            self._check_columns(columns, int(rows), "route_into: column set %d" % k)
            for field, name in self._COLS_FIELDS:
                setattr(out[k], field, columns[name].data_ptr())
        traj = self._traj(0)
        goal_slot = self._goal_slots32()
        _lib.check(self._lib.cm3_transitions_route_f32(ctypes.byref(env._desc), ctypes.byref(traj), _lib.ptr(goal_slot),
                                                       0 if goal_slot is None else env.E * 4, int(B), sel.data_ptr(), row.data_ptr(),
                                                       out, len(sets), env._stream()))
        return B

    def as_reference_batch_torch(self, tt, ee, numpy=True):
        """The same columns as a composition of torch indexing operations (any dtype; what the kernel path is tested against)."""
        tt = torch.as_tensor(tt, device=self.env.device, dtype=torch.long)
        ee = torch.as_tensor(ee, device=self.env.device, dtype=torch.long)
        state = self.state[tt, :, ee]                                   # [B, N, 4]
        nxt_state = self._next("state", tt, ee)
        if self._goals_buf is None:
            goals = self.env._goals[:, ee].permute(1, 0, 2)             # [B, N, 2]
        elif self._goals_sparse:                                        # (gathered from the last written slot: nothing is filled in)
            goals = self._goals_buf[self._goal_source_slots()[tt, ee], :, ee]
        else:
            goals = self._goals_buf[tt, :, ee]
        cols = dict(
            v_global=state, obs_others=self.obs_others[tt, ee], v_local=state,
            actions=self.actions[tt, ee], reward=self.reward[tt, ee], reward_local=self.reward_n[tt, ee],
            v_global_next=nxt_state, obs_others_next=self._next("obs_others", tt, ee), v_local_next=nxt_state,
            done=self.done[tt, ee].bool(), goals=goals)
        return _to_numpy(cols) if numpy else cols

    def on_policy_phase(self, epochs=24, batch_size=128, generator=None, l_action=5):
        """The minibatches of on_policy_minibatches() TOGETHER WITH the static feeds of the reference's train_step for each of them
        (cm3_amd.batch.phase_static_feeds: process_actions / process_global_state, the n x n credit repeats, the n x n x l_action
        counterfactual tiling of alg_credit.py:406-557, :614-658, :730-751) -- for the whole phase one export launch and one pair of
        tiling launches; a list of (columns, static) pairs of views, static None where the tiling kernel does not apply (N = 1, float64).
        Feed them to cm3_amd.batch.train_step_feeds(columns, run, gamma, epsilon, static=static)."""
        from . import batch as B
        cols, k = self._phase_export(epochs, batch_size, generator)
        vg = cols["v_global"]
        if vg.is_cuda and vg.dtype == torch.float32 and vg.shape[1] > 1:
            statics = B.phase_static_feeds(cols, int(epochs), l_action)
        else:
            statics = [None] * int(epochs)
        return [({name: v[m * k:(m + 1) * k] for name, v in cols.items()}, statics[m]) for m in range(int(epochs))]


def sample_distinct(n, size, rows, generator, device):
    """int64 [rows, size]: every row `size` DISTINCT integers of range(n), uniformly at random over the size-subsets and their orders
    (the reference's random.sample).  n small: a permutation per row.  n >> size (a phase holds 10^6 transitions, a minibatch 128):
    2 size draws with replacement per row and the first `size` distinct values in draw order -- sequential drawing with rejection of
    repeats is exactly sampling without replacement -- found with a stable sort, no host synchronisation: O(size log size) work instead
    of a permutation of all n.  (Fewer than `size` distinct values among 2 size draws from n >= 64 size needs more than `size`
    collisions: probability below 1e-100; the positions such a row would leave unset hold 0 .. size - 1.)"""
    if n < 64 * size:
        return torch.stack([torch.randperm(n, generator=generator, device=device)[:size] for _ in range(rows)])
    m = 2 * size
    x = torch.randint(0, n, (rows, m), generator=generator, device=device)
    sx, order = torch.sort(x, dim=1, stable=True)
    first_sorted = torch.ones_like(sx, dtype=torch.bool)
    first_sorted[:, 1:] = sx[:, 1:] != sx[:, :-1]                    # first of each run of equal values = its earliest draw (stable)
    first = torch.zeros_like(first_sorted).scatter_(1, order, first_sorted)      # ... in draw order
    rank = torch.cumsum(first, dim=1) - 1
    dst = torch.where(first & (rank < size), rank, torch.full_like(rank, size))
    out = torch.arange(size + 1, device=device).repeat(rows, 1)
    out.scatter_(1, dst, x)
    return out[:, :size].contiguous()


class CheckersRollout(_Transitions):
    """T-tick trajectory over a VecCheckersEnv (16-column transitions, train_onpolicy.py:336).

    env.auto_reset False: episode-synchronous -- the env is reset at the start of every collect(); transitions of an
        env after its `done` are flagged invalid (one reference episode per env).
    env.auto_reset True: continuous -- finished envs restart inside the launch (CM3_FLAG_AUTO_RESET); slot t+1 then
        holds the FRESH episode's observation, the true terminal next_* of the transition are captured per tick
        (term_*; the reference stores them before it resets, train_onpolicy.py:336-347), the goals in effect are
        recorded per slot (they change when a single-agent env restarts, :288-291), and `actions_prev` of the first
        transition of an episode is zeros (:295).  Every transition is valid; collect() continues where the previous
        one stopped.
    """

    def __init__(self, env, n_ticks=None, use_graph=True, fused=False, policy_mode="auto", record_probs=False):
        """policy_mode (collect(policy=<CheckersActor>)): "auto" = the whole rollout in ONE launch (cm3_policy_rollout_checkers)
        wherever that kernel applies (CheckersActor.fused_rollout_ok), else -- and with "tick" -- an actor launch and a step
        launch per tick inside one hipGraph; the two produce the same bits.  A CheckersQmixAgent runs as launch pairs under
        "auto" and "tick".  "episode" = the one-launch kernel or an error, for either device policy: cm3_policy_rollout_checkers
        for the actor, cm3_policy_rollout_checkers_qmix for the QMIX agent (CheckersQmixAgent.episode_ok), same bits as its
        launch pairs; collect() raises Cm3Error naming the condition that fails (precision, agent count, seed / env_id_base).
        A host callable or policy=None behaves under "episode" as under "auto".  record_probs: keep the mixed probabilities
        the actions were drawn from -- the QMIX agent's Q values -- float32 [T, E, N, 5] (self.probs)."""
        self.env = env
        self.T = int(n_ticks or env.max_steps)
        self.use_graph = bool(use_graph)
        self.fused = bool(fused)      # random-action branch in ONE launch (CM3_FLAG_FUSED_TICKS; fast kernel only)
        if policy_mode not in ("auto", "episode", "tick"):
            raise Cm3Error("policy_mode must be 'auto', 'episode' or 'tick'")
        self.policy_mode = policy_mode
        self.auto_reset = bool(env.auto_reset)
        E, N, T, dev = env.E, env.n, self.T, env.device
        z = lambda *s, d: torch.zeros(*s, dtype=d, device=dev)  # noqa: E731
        self._grid_raw = z(T + 1, E, env.grid_stride, d=torch.int8)
        self._obst_raw = z(T + 1, E, env.obst_stride, d=torch.int8)
        self.grid = env.grid_view(self._grid_raw)              # [T+1, E, R, C+1, 2] view (padding hidden)
        self.vec = z(T + 1, E, N, 4, d=torch.int32)
        self.obs_others = z(T + 1, E, N, env.Lo, d=torch.float64)
        self.obs_self_t = env.obst_view(self._obst_raw)        # [T+1, E, N, K, K, 3] view
        self.obs_self_v = z(T + 1, E, N, 4, d=torch.float64)
        self.actions = z(T, E, N, d=torch.int32)
        self.local_rewards = z(T, E, N, d=torch.float64)
        self.reward = z(T, E, d=torch.float64)
        self.done = z(T, E, d=torch.uint8)
        self._prev_bufs = (z(E, N, d=torch.int32), z(E, N, d=torch.int32), z(E, N, d=torch.int32))
        self.prev0 = self._prev_bufs[1]                        # actions_prev of slot 0 (zeros at an episode start)
        self._rolled = None
        self.probs = z(T, E, N, 5, d=torch.float32) if record_probs else None
        if self.auto_reset:
            self._term_grid_raw = z(T, E, env.grid_stride, d=torch.int8)
            self._term_obst_raw = z(T, E, env.obst_stride, d=torch.int8)
            self.term_grid = env.grid_view(self._term_grid_raw)
            self.term_obs_self_t = env.obst_view(self._term_obst_raw)
            self.term_vec = z(T, E, N, 4, d=torch.int32)
            self.term_obs_others = z(T, E, N, env.Lo, d=torch.float64)
            self.term_obs_self_v = z(T, E, N, 4, d=torch.float64)
            self.goal_slots = z(T + 1, E, N, d=torch.uint8)
        else:
            self.goal_slots = None
        self._started = False
        self._goals_onehot = None
        self._traj_cache = None               # (the ctypes structs of the one-launch rollout: the buffers never move)
        self._gather_traj = None              # (... and of the transition export)
        # the captured graphs: the random-action rollout, the actor / step launch pairs
        self._graph, self._actor_graph = _CapturedGraph(dev), _ActorGraphCache(dev)
        self._graphs = (self._graph, self._actor_graph)
        self._lib = _lib.lib()

    def _bufs(self, t):
        env = self.env
        b = _lib.CheckersBufs()
        b.mask, b.agents, b.steps = env._mask.data_ptr(), env._agents.data_ptr(), env._steps.data_ptr()
        b.episode, b.goals = env._episode.data_ptr(), env._goals.data_ptr()
        b.actions = self.actions[t].data_ptr()
        b.grid, b.vec = self._grid_raw[t + 1].data_ptr(), self.vec[t + 1].data_ptr()
        b.obs_others = self.obs_others[t + 1].data_ptr()
        b.obs_self_t, b.obs_self_v = self._obst_raw[t + 1].data_ptr(), self.obs_self_v[t + 1].data_ptr()
        b.local_rewards, b.reward, b.done = (self.local_rewards[t].data_ptr(), self.reward[t].data_ptr(),
                                             self.done[t].data_ptr())
        if self.auto_reset:
            b.term_grid, b.term_vec = self._term_grid_raw[t].data_ptr(), self.term_vec[t].data_ptr()
            b.term_obs_others = self.term_obs_others[t].data_ptr()
            b.term_obs_self_t, b.term_obs_self_v = self._term_obst_raw[t].data_ptr(), self.term_obs_self_v[t].data_ptr()
            b.goals_next = self.goal_slots[t + 1].data_ptr()
        return b

    def _traj(self):
        env = self.env
        t = _lib.CheckersTraj()
        t.mask, t.agents, t.steps = env._mask.data_ptr(), env._agents.data_ptr(), env._steps.data_ptr()
        t.episode, t.goals = env._episode.data_ptr(), env._goals.data_ptr()
        t.action_block = env._action_block.data_ptr()
        def slot(x):
            return x.data_ptr(), x[0].numel() * x.element_size()
        t.actions, t.actions_stride = slot(self.actions)
        t.grid, t.grid_slot_stride = slot(self._grid_raw)
        t.vec, t.vec_stride = slot(self.vec)
        t.obs_others, t.obs_others_stride = slot(self.obs_others)
        t.obs_self_t, t.obs_self_t_slot_stride = slot(self._obst_raw)
        t.obs_self_v, t.obs_self_v_stride = slot(self.obs_self_v)
        t.local_rewards, t.local_rewards_stride = slot(self.local_rewards)
        t.reward, t.reward_stride = slot(self.reward)
        t.done, t.done_stride = slot(self.done)
        if self.auto_reset:
            t.term_grid, t.term_grid_slot_stride = slot(self._term_grid_raw)
            t.term_vec, t.term_vec_stride = slot(self.term_vec)
            t.term_obs_others, t.term_obs_others_stride = slot(self.term_obs_others)
            t.term_obs_self_t, t.term_obs_self_t_slot_stride = slot(self._term_obst_raw)
            t.term_obs_self_v, t.term_obs_self_v_stride = slot(self.term_obs_self_v)
            t.goals_slots, t.goals_slots_stride = slot(self.goal_slots)
        return t

    def _base_flags(self):
        return FLAG_AUTO_RESET if self.auto_reset else 0

    def _enqueue_random(self, stream, fused):
        env = self.env
        env._desc.flags = self._base_flags() | FLAG_GEN_ACTIONS | (_lib.FLAG_FUSED_TICKS if fused else 0)
        traj = self._traj()
        _lib.check(self._lib.cm3_checkers_rollout(ctypes.byref(env._desc), ctypes.byref(traj), self.T, stream))
        env._desc.flags = 0

    def _enqueue_step(self, t, stream):
        """One cm3_checkers_step launch: consumes actions[t], writes slot t + 1 (the caller clears env._desc.flags after its last)."""
        env = self.env
        env._desc.flags = self._base_flags()
        b = self._bufs(t)
        _lib.check(self._lib.cm3_checkers_step(ctypes.byref(env._desc), ctypes.byref(b), stream))

    def _enqueue_actor_rollout(self, actor, epsilon, stream):
        """T x (actor launch, step launch) on `stream`: the policy reads trajectory slot t (+ actions[t-1] as
        actions_prev -- prev0 at t = 0, zeros where the previous tick ended an episode: train_onpolicy.py:295,345) and
        writes actions[t]; the step kernel consumes them and writes slot t+1 (train_onpolicy.py:309-321 without leaving
        the device)."""
        env = self.env
        for t in range(self.T):
            goals = self.goal_slots[t] if self.auto_reset else env._goals
            actor.enqueue(env.E, self._obst_raw[t], env.obst_stride, self.obs_self_v[t], self.obs_others[t], goals,
                          self.actions[t - 1] if t > 0 else self.prev0, env._steps, env._episode, self.actions[t], epsilon,
                          probs=None if self.probs is None else self.probs[t], stream=stream, env_id_base=env._desc.env_id_base,
                          prev_done=self.done[t - 1] if (t > 0 and self.auto_reset) else None)
            self._enqueue_step(t, stream)
        env._desc.flags = 0

    def _enqueue_policy_rollout(self, actor, epsilon, stream, prev0_next=None):
        """The same T ticks as _enqueue_actor_rollout in ONE launch (csrc/policy_checkers.hip), slot 0 and the env's
        current-observation buffers (what _load_slot0 / _store_back copy for the other modes) included."""
        env = self.env
        env._desc.flags = self._base_flags()
        if self._traj_cache is None or self._traj_cache[0] != env._cur:
            self._traj_cache = (env._cur, self._traj(), env._bufs(env._cur))
        _, traj, final = self._traj_cache
        _, enqueue = _one_launch_hooks(actor)
        enqueue(env._desc, traj, env.E, env.obst_stride, self.T, epsilon, prev0=self.prev0, probs=self.probs, stream=stream,
                final_obs=final, prev0_next=prev0_next)
        env._desc.flags = 0

    def _load_slot0(self):
        """slot 0 <- the env's current observation (after a reset, or where the previous collect() stopped)."""
        env = self.env
        s = env._slots[env._cur]
        pairs = [(self._grid_raw[0], s["grid_raw"]), (self._obst_raw[0], s["obs_self_t_raw"]), (self.vec[0], s["vec"]),
                 (self.obs_others[0], s["obs_others"]), (self.obs_self_v[0], s["obs_self_v"])]
        if self.goal_slots is not None:
            pairs.append((self.goal_slots[0], env._goals))
        _copy_pairs(pairs, env._stream())

    def _store_back(self):
        """the env's current-observation buffers <- slot T, so that get_obs() / CheckersActor.act(env) / the next
        collect() see the state the rollout left (the compact live state is advanced in place by the launches)."""
        env, T = self.env, self.T
        s = env._slots[env._cur]
        _copy_pairs([(s["grid_raw"], self._grid_raw[T]), (s["obs_self_t_raw"], self._obst_raw[T]), (s["vec"], self.vec[T]),
                     (s["obs_others"], self.obs_others[T]), (s["obs_self_v"], self.obs_self_v[T]),
                     (s["actions"], self.actions[T - 1])], env._stream())

    def collect(self, goals=None, policy=None, epsilon=0.0, reset=None):
        """goals: one-hot [N,2] / [E,N,2] (train_onpolicy.py:287-293); needed whenever the env is reset.
        policy None = uniform random actions drawn in-kernel; a cm3_amd.actor.CheckersActor or cm3_amd.qmix.CheckersQmixAgent = the
        on-device policy (the whole rollout in one launch, or policy and step launches alternating inside one hipGraph: policy_mode);
        else policy(actions_prev, obs_others, obs_self_t, obs_self_v, goals) -> [E,N] on the host.  reset: None -> always for an
        episode-synchronous env, only the first time for a continuous (auto-reset) one."""
        env = self.env
        one_launch = (policy is not None and hasattr(policy, "enqueue_rollout") and self.policy_mode == "auto"
                      and policy.fused_rollout_ok(env))
        if self.policy_mode == "episode" and _is_device_policy(policy):
            hooks = _one_launch_hooks(policy)
            if hooks is None or not hooks[0](env):     # (before the env is reset or anything is launched)
                raise Cm3Error("policy_mode='episode': " + _one_launch_refusal(policy, env))
            one_launch = True
        if reset is None:
            reset = (not self.auto_reset) or (not self._started)
        # actions_prev of tick 0 (self.prev0; train_onpolicy.py:295,345): zeros after a reset, else the previous rollout's last actions
        # (zeros where its last tick ended an episode).  Three buffers: one that holds zeros and is never written, two that take
        # turns -- the one-launch kernel writes the NEXT rollout's prev0 into the spare one, so nothing is launched for it here.
        pz, pa, pb = self._prev_bufs
        if reset:
            if goals is None:
                raise Cm3Error("collect() resets the env here and needs goals")
            env.reset(goals, quiet=True)
            if one_launch:
                self.prev0 = pz
            else:
                self.prev0 = pa
                self.prev0.zero_()
        elif self._started:
            if self._rolled is not None and one_launch:
                self.prev0 = self._rolled
            else:
                # (the launch-per-tick modes read prev0 from a CAPTURED graph: always the same buffer, pa)
                if self._rolled is not None:
                    nxt = self._rolled
                else:
                    keep = (self.done[self.T - 1] == 0).unsqueeze(1)
                    nxt = torch.where(keep, self.actions[self.T - 1], torch.zeros_like(self.actions[0]))
                self.prev0 = pa
                if nxt is not pa:
                    pa.copy_(nxt)
        self._rolled = None
        self._started = True
        self._goals_onehot = None             # (lazy: see goals_onehot)
        stream = env._stream()
        if one_launch:
            # cm3_policy_rollout_checkers writes slot 0 from the live state and hands the state it leaves to the env's own
            # current-observation buffers: no copies around the launch
            spare = pa if self.prev0 is not pa else pb
            self._enqueue_policy_rollout(policy, epsilon, stream, spare)
            self._rolled = spare
            return self
        self._load_slot0()
        if policy is None:
            # random-action branch (train_onpolicy.py:305-307): cm3_checkers_rollout -- one fused launch, or T step
            # launches bound to their trajectory slots and replayed as one hipGraph
            if self.fused:
                self._enqueue_random(stream, True)
            elif self.use_graph:
                self._graph.launch(lambda st: self._enqueue_random(st, False), stream)
            else:
                self._enqueue_random(stream, False)
        elif _is_device_policy(policy):                                          # on-device actor, a launch pair per tick
            if self.use_graph:
                cache = self._actor_graph
                cache.launch(policy, epsilon, lambda st: self._enqueue_actor_rollout(policy, cache.eps, st), stream)
            else:
                self._enqueue_actor_rollout(policy, epsilon, stream)
        else:
            for t in range(self.T):                                              # host policy: one call per tick
                a = policy(self.actions_prev_at(t), self.obs_others[t], self.obs_self_t[t], self.obs_self_v[t],
                           self.goals_at(t))
                self.actions[t].copy_(torch.as_tensor(a, device=env.device).reshape(env.E, env.n))
                self._enqueue_step(t, stream)
            env._desc.flags = 0
        self._store_back()
        return self

    @property
    def goals_onehot(self):
        """[E,N,2] one-hot goals of the rollout's episodes when no goal slots are recorded (episode-synchronous envs: the goals the
        env was reset with; they cannot change inside a collect()).  Built on first use: a collect() does not pay for it."""
        if self._goals_onehot is None:
            self._goals_onehot = self.env.goals.clone()
        return self._goals_onehot

    def actions_prev_at(self, t):
        """int32 [E,N]: the actions_prev fed at tick t (train_onpolicy.py:295,345)."""
        if t == 0:
            return self.prev0
        if not self.auto_reset:
            return self.actions[t - 1]
        return torch.where((self.done[t - 1] == 0).unsqueeze(1), self.actions[t - 1], torch.zeros_like(self.actions[0]))

    def goals_at(self, t):
        """one-hot [E,N,2] goals in effect at tick t."""
        if self.goal_slots is None:
            return self.goals_onehot
        return torch.nn.functional.one_hot(self.goal_slots[t].long(), 2)

    ORDER = CHECKERS_ORDER

    def _next(self, name, tt, ee):
        """next_<name> of transitions (tt, ee): slot t+1, or the captured terminal observation where the env restarted
        in the same launch (continuous mode)."""
        nxt = getattr(self, name)[tt + 1, ee]
        if self.auto_reset:
            term = getattr(self, "term_" + name)[tt, ee]
            d = self.done[tt, ee].bool().view(-1, *([1] * (nxt.dim() - 1)))
            nxt = torch.where(d, term, nxt)
        return nxt

    def column_specs(self):
        """name -> (row shape, dtype) of the 16 columns of as_reference_batch(numpy=False), in ORDER."""
        env = self.env
        N = env.n
        shapes = dict(grid=(env.R, env.C + 1, 2), vec=(N, 4), obs_others=(N, env.Lo), obs_self_t=(N, env.K, env.K, 3), obs_self_v=(N, 4),
                      actions=(N,), reward=(), local_rewards=(N,), done=(), goals=(N, 2))
        return {name: (shapes[rec], CHECKERS_DTYPES[rec][0]) for name, rec in _lib.CHECKERS_COLUMN_RECORDS}

    def compact_column_specs(self):
        """name -> (row shape, dtype) of the 16 columns of a compact replay ring (replay.CompactCheckersReplayBuffer), in ORDER: the
        columns of column_specs() with the dtypes the trajectory keeps (707 B per transition at the reference geometry, not 3657)."""
        return compact_specs(self.column_specs())

    def _export_args(self):
        if self._gather_traj is None:
            self._gather_traj = self._traj()           # (built once: the trajectory buffers never move)
        return ctypes.byref(self.env._desc), ctypes.byref(self._gather_traj), self.prev0.data_ptr()

    def _gather(self, tt, ee, B, columns, ring_start=0, ring_size=0):
        """ONE launch of cm3_checkers_transitions_gather (csrc/batch.hip) fills all of `columns` (checked by the caller); integer-valued
        columns are cast to the reference's float64 (alg_credit_checkers.py:427-444).  as_reference_batch_torch below is the same as a
        composition of torch operations, ~40 launches: what the kernel is tested against."""
        out = _lib.fill_checkers_cols(_lib.CheckersTransitionCols(), columns, ring_start, ring_size)
        _lib.check(self._lib.cm3_checkers_transitions_gather(*self._export_args(), _lib.ptr(tt), _lib.ptr(ee), int(B), ctypes.byref(out),
                                                             self.env._stream()))

    def pack_into(self, columns, ring_start, ring_size):
        """export_into for a compact ring: `columns` are those of compact_column_specs(), ring_size rows each.  ONE launch of
        cm3_checkers_transitions_pack, nothing converted; the same checks before it.  Returns the number of transitions."""
        B = self._ring_chunk("pack_into", columns, ring_start, ring_size, self.compact_column_specs())
        out = _lib.fill_checkers_cols(_lib.CheckersCompactCols(), columns, ring_start, ring_size)
        _lib.check(self._lib.cm3_checkers_transitions_pack(*self._export_args(), B, ctypes.byref(out), self.env._stream()))
        return B

    def as_reference_batch_torch(self, tt, ee, numpy=True):
        """The same columns as a composition of torch indexing operations (the specification of cm3_checkers_transitions_gather);
        tt None: all valid transitions."""
        dev = self.env.device
        if tt is None:
            tt, ee = self.valid_indices()
        tt =torch.as_tensor(tt, device=dev, dtype=torch.long)
        ee = torch.as_tensor(ee, device=dev, dtype=torch.long)
        f = lambda x: x.to(torch.float64)  # noqa: E731
        prev = self.actions[(tt - 1).clamp(min=0), ee]
        if self.auto_reset:                                            # a fresh episode starts from zeros (:295)
            fresh = self.done[(tt - 1).clamp(min=0), ee].bool().view(-1, 1)
            prev = torch.where(fresh, torch.zeros_like(prev), prev)
        prev = torch.where((tt > 0).view(-1, 1), prev, self.prev0[ee])
        goals = (self.goals_onehot[ee] if self.goal_slots is None
                 else torch.nn.functional.one_hot(self.goal_slots[tt, ee].long(), 2))
        cols = dict(
            grid=f(self.grid[tt, ee]), vec=f(self.vec[tt, ee]), obs_others=self.obs_others[tt, ee],
            obs_self_t=f(self.obs_self_t[tt, ee]), obs_self_v=self.obs_self_v[tt, ee],
            actions_prev=prev, actions=self.actions[tt, ee], reward=self.reward[tt, ee],
            local_rewards=self.local_rewards[tt, ee],
            next_grid=f(self._next("grid", tt, ee)), next_vec=f(self._next("vec", tt, ee)),
            next_obs_others=self._next("obs_others", tt, ee), next_obs_self_t=f(self._next("obs_self_t", tt, ee)),
            next_obs_self_v=self._next("obs_self_v", tt, ee), done=self.done[tt, ee].bool(),
            goals=goals)
        return _to_numpy(cols) if numpy else cols

    def on_policy_phase(self, epochs=24, batch_size=128, generator=None, l_action=5):
        """The minibatches of on_policy_minibatches() TOGETHER WITH the static feeds of alg_credit_checkers.train_step for each of them
        (cm3_amd.batch.phase_static_feeds(env="checkers"): process_batch / process_global_state, the n x n credit repeats, the
        n x n x l_action counterfactual tiling of alg_credit_checkers.py:414-535, :590-760) -- for the whole phase one export launch and
        three tiling launches; a list of (columns, static) pairs of views, static None where the tiling kernel does not apply (N = 1).
        Feed them to cm3_amd.batch.train_step_feeds(columns, run, gamma, epsilon, env="checkers", static=static)."""
        from . import batch as B
        cols, k = self._phase_export(epochs, batch_size, generator)
        if B.checkers_static_feeds_apply(cols):
            statics = B.phase_static_feeds(cols, int(epochs), l_action, env="checkers")
        else:
            statics = [None] * int(epochs)
        return [({name: v[m * k:(m + 1) * k] for name, v in cols.items()}, statics[m]) for m in range(int(epochs))]

    def episode_returns(self):
        v = self.valid.to(torch.float64)
        return (self.reward * v).sum(0), (self.local_rewards * v.unsqueeze(2)).sum(0)
