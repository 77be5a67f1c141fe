"""Batch reformatting on the device.

The reference reshapes every sampled batch on the host with NumPy before each of its 6-8 sess.run calls:
  alg_credit.Alg.process_actions       alg/alg_credit.py:406-443
  alg_credit.Alg.process_batch         alg/alg_credit.py:445-499
  alg_credit.Alg.process_goals         alg/alg_credit.py:501-526
  alg_credit.Alg.process_global_state  alg/alg_credit.py:528-557
  the n x n "credit" repeats of train_step   alg/alg_credit.py:614-658
Here the same arrays are produced from the device trajectory columns (ParticleRollout.as_reference_batch(...,
numpy=False)) with gathers / views, so a learner living on the GPU never pulls the batch through the host.
Pure data movement: outputs are bit-identical to the reference's (tests/test_batch.py pins them to arrays produced
by the REAL reference functions, tests/golden/batch_particle.npz).

Layout: _Tiler and the two TileSpec tables (particle_static_feed_specs / checkers_static_feed_specs) -- every feed of train_step
that does not depend on a network output, as "destination row r <- source row f(r)" outputs of cm3_rows_tile; the torch composition
of the same dict (_static_feeds_composed: the specification, and the path of the inputs the kernels do not take); train_step_feeds,
which reads either dict on one path, the envs differing in data only (_Particle / _Checkers); OnPolicyPhasePlan, which captures one
train_step_feeds per minibatch into a hipGraph and holds every tensor the captured launches touch; the QMIX feed builders.
"""
import collections

import torch

from ._net import _keep


def rep_rows(x, n):
    """every row of x repeated n times consecutively -- x.repeat_interleave(n, dim=0) as ONE copy launch (expand + reshape; torch's
    repeat_interleave builds a repeats tensor, a cumulative sum and an index_select: four launches, and train_step has a dozen)."""
    return x.unsqueeze(1).expand(x.shape[0], int(n), *x.shape[1:]).reshape(x.shape[0] * int(n), *x.shape[1:])


class _Tiler(object):
    """Collects "destination row r <- source row f(r)" outputs and builds them 16 per launch (cm3_rows_tile, csrc/batch.hip)."""

    def __init__(self, device):
        self.device, self.specs, self.keep = device, [], []

    def add(self, src, n_rows, epr, dtype, kind, terms=((1, 0, 1), (1, 0, 0)), others=None, shape=None, out=None):
        from . import _lib
        want = tuple((n_rows, epr) if shape is None else shape)
        if out is None:
            out = torch.empty(want, dtype=dtype, device=self.device)
        elif tuple(out.shape) != want or out.dtype != dtype or not out.is_contiguous():
            raise ValueError("persistent feed tensor has shape %s / %s, expected %s / %s" % (tuple(out.shape), out.dtype, want, dtype))
        c = _lib.TileCol()
        c.dst, c.src, c.n_rows, c.elems_per_row, c.kind = out.data_ptr(), (0 if src is None else src.data_ptr()), n_rows, epr, kind
        c.elem_bytes = src.element_size() if (src is not None and kind == _lib.TILE_COPY) else 0
        if others is not None:
            c.others_n, c.others_divq, c.others_divn = others
        else:
            for i, (d, m, mul) in enumerate(terms):
                c.div[i], c.mod[i], c.mul[i] = d, m, mul
        self.specs.append(c)
        self.keep.append(src)
        return out

    def run(self):
        from . import _lib
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for k in range(0, len(self.specs), 16):
            chunk = self.specs[k:k + 16]
            arr = (_lib.TileCol * len(chunk))(*chunk)
            _lib.check(_lib.lib().cm3_rows_tile(arr, len(chunk), stream))
        self.specs, self.keep = [], []


TileSpec = collections.namedtuple("TileSpec", "name src rows epr dtype kind terms others shape")
TileSpec.__doc__ = """One output of cm3_rows_tile: `name` [shape, default (rows, epr)] of `dtype`, destination row r <- row f(r) of column `src`
(None: no source), f from the two (divisor, modulus, multiplier) `terms` or, when given, the `others` triple (N, divq, divn) of the
reference's `np.arange(N) != n` selections (include/cm3_amd.h, cm3_tile_col); `kind` one of _lib.TILE_*."""
_IDENT = ((1, 0, 1), (1, 0, 0))


def _row_maps(N):
    """The row functions both spec tables use, for N agents: by_n / by_m (things the reference repeats "indexed by n" / "by m"), by_b
    (per time step) and the `others` triple."""
    by_n = lambda outer=1: ((outer * N * N, 0, N), (outer, N, 1))          # noqa: E731  rows (b, m, n[, a]) <- row b N + n
    by_m = lambda outer=1: ((outer * N, 0, 1), (1, 0, 0))                   # noqa: E731  rows (r, m[, a])    <- row r
    by_b = lambda per: ((per, 0, 1), (1, 0, 0))                             # noqa: E731  `per` rows per time step <- row b
    oth = lambda per, inner: (N, per * (N - 1), inner * (N - 1))            # noqa: E731  `per` rows per time step, n varies every `inner`
    return by_n, by_m, by_b, oth


def particle_static_feed_specs(shapes, dtypes, l_action=5):
    """The outputs of particle_static_feeds_device as a list of TileSpec, from shapes and dtypes alone (no device, no library): shapes
    maps v_global and goals to the shapes of those columns of ParticleRollout.as_reference_batch -- [B, N, l], [B, N, l_goal] -- and
    dtypes maps v_global, goals, reward and reward_local to theirs (the copies keep them; v_global_next is v_global's twin).  Source
    names are column names; "actions" stands for the flat int32 actions, "done" for its bytes.  The sixteen outputs of the first
    launch, then the six of the second: per agent row (B N rows; alg_credit.py:406-443, :528-557), the credit repeats (B N N;
    :614-658), the counterfactual tiling (B N N l_action; :730-751)."""
    from . import _lib
    COPY, WIDEN, ONE_I, ONE_F, EYE, NOT = (_lib.TILE_COPY, _lib.TILE_F32_TO_F64, _lib.TILE_ONEHOT_I64, _lib.TILE_ONEHOT_F64,
                                           _lib.TILE_EYE_F64, _lib.TILE_NOT_I64)
    B, N, l = (int(v) for v in shapes["v_global"])
    lg = int(shapes["goals"][2])
    A, R = int(l_action), B * N
    f64, i64, vt, gt = torch.float64, torch.int64, dtypes["v_global"], dtypes["goals"]
    by_n, by_m, by_b, oth = _row_maps(N)
    T = TileSpec
    return [
        T("a1", "actions", R, A, i64, ONE_I, _IDENT, None, None),
        T("ao", "actions", R * (N - 1), A, f64, ONE_F, None, oth(N, 1), (R, N - 1, A)),
        T("reward_rep", "reward", R, 1, dtypes["reward"], COPY, by_b(N), None, (R,)),
        T("done_rep", "done", R, 1, torch.bool, COPY, by_b(N), None, (R,)),
        T("not_done", "done", R, 1, i64, NOT, by_b(N), None, (R,)),
        T("others", "v_global", R * (N - 1), l, f64, WIDEN, None, oth(N, 1), (R, (N - 1) * l)),
        T("others_next", "v_global_next", R * (N - 1), l, f64, WIDEN, None, oth(N, 1), (R, (N - 1) * l)),
        T("goals_self_rep", "goals", R * N, lg, gt, COPY, by_n(), None, None),
        T("one_next_rep_n", "v_global_next", R * N, l, vt, COPY, by_n(), None, None),
        T("one_next_rep_m", "v_global_next", R * N, l, vt, COPY, by_m(), None, None),
        T("others_next_rep_n", "v_global_next", R * N * (N - 1), l, f64, WIDEN, None, oth(N * N, 1), (R * N, (N - 1) * l)),
        T("r_rep", "reward_local", R * N, 1, dtypes["reward_local"], COPY, by_n(), None, (R * N,)),
        T("nd_rep", "done", R * N, 1, i64, NOT, by_b(N * N), None, (R * N,)),
        T("s_n_rep", "v_global", R * N, l, vt, COPY, by_n(), None, None),
        T("s_m_rep", "v_global", R * N, l, vt, COPY, by_m(), None, None),
        T("s_others_rep", "v_global", R * N * (N - 1), l, f64, WIDEN, None, oth(N * N, 1), (R * N, (N - 1) * l)),
        # ---- second launch ----
        T("a1_rep_m", "actions", R * N, A, i64, ONE_I, by_m(), None, None),
        T("cf_s_n", "v_global", R * N * A, l, vt, COPY, by_n(A), None, None),
        T("cf_goals", "goals", R * N * A, lg, gt, COPY, by_n(A), None, None),
        T("cf_eye", None, R * N * A, A, f64, EYE, _IDENT, None, None),
        T("cf_s_m", "v_global", R * N * A, l, vt, COPY, by_m(A), None, None),
        T("cf_s_others", "v_global", R * N * A * (N - 1), l, f64, WIDEN, None, oth(N * N * A, A), (R * N * A, (N - 1) * l)),
    ]


def checkers_static_feed_specs(shapes, goals_dtype=torch.int64, l_action=5):
    """The outputs of checkers_static_feeds_device as a list of TileSpec, from the shapes alone (no device, no library): shapes maps
    grid, vec, obs_self_t, obs_self_v and goals to the shapes of those columns of CheckersRollout.as_reference_batch -- [B, R, C + 1, 2],
    [B, N, 4], [B, N, K, K, 3], [B, N, 4], [B, N, 2]; the next_* columns have the shapes of their twins.  Source names are column names;
    "actions" / "actions_prev" stand for the flat int32 actions, "done" for its bytes.  Three groups, in the order of train_step
    (alg_credit_checkers.py:536-780): per agent row (B N rows), the credit repeats (B N N), the counterfactual tiling (B N N l_action)."""
    from . import _lib
    COPY, ONE_I, ONE_F, EYE, NOT = _lib.TILE_COPY, _lib.TILE_ONEHOT_I64, _lib.TILE_ONEHOT_F64, _lib.TILE_EYE_F64, _lib.TILE_NOT_I64
    B, N, lv = (int(v) for v in shapes["vec"])
    g_sh, t_sh, v_sh = tuple(shapes["grid"][1:]), tuple(shapes["obs_self_t"][2:]), tuple(shapes["obs_self_v"][2:])
    count = lambda sh: int(torch.Size(sh).numel())                          # noqa: E731
    ne, nt, nv, lg = count(g_sh), count(t_sh), count(v_sh), int(shapes["goals"][2])
    A, R = int(l_action), B * N
    f64, i64 = torch.float64, torch.int64
    by_n, by_m, by_b, oth = _row_maps(N)
    T = TileSpec
    return [
        # ---- per agent row: process_batch (:414-482), process_global_state (:510-535), not_done (:560) ----
        T("state_env", "grid", R, ne, f64, COPY, by_b(N), None, (R,) + g_sh),
        T("state_env_next", "next_grid", R, ne, f64, COPY, by_b(N), None, (R,) + g_sh),
        T("a1", "actions", R, A, i64, ONE_I, _IDENT, None, None),
        T("ao", "actions", R * (N - 1), A, f64, ONE_F, None, oth(N, 1), (R, N - 1, A)),
        T("prev1", "actions_prev", R, A, i64, ONE_I, _IDENT, None, None),
        T("done_rep", "done", R, 1, torch.bool, COPY, by_b(N), None, (R,)),
        T("not_done", "done", R, 1, i64, NOT, by_b(N), None, (R,)),
        T("others", "vec", R * (N - 1), lv, f64, COPY, None, oth(N, 1), (R, (N - 1) * lv)),
        T("others_next", "next_vec", R * (N - 1), lv, f64, COPY, None, oth(N, 1), (R, (N - 1) * lv)),
        # ---- the n x n credit repeats (:590-660): things indexed by n repeat per block, things indexed by m row by row ----
        T("goals_self_rep", "goals", R * N, lg, goals_dtype, COPY, by_n(), None, None),
        T("one_next_rep_n", "next_vec", R * N, lv, f64, COPY, by_n(), None, None),
        T("one_next_rep_m", "next_vec", R * N, lv, f64, COPY, by_m(), None, None),
        T("others_next_rep_n", "next_vec", R * N * (N - 1), lv, f64, COPY, None, oth(N * N, 1), (R * N, (N - 1) * lv)),
        T("r_rep", "local_rewards", R * N, 1, f64, COPY, by_n(), None, (R * N,)),
        T("nd_rep", "done", R * N, 1, i64, NOT, by_b(N * N), None, (R * N,)),
        T("s_n_rep", "vec", R * N, lv, f64, COPY, by_n(), None, None),
        T("s_m_rep", "vec", R * N, lv, f64, COPY, by_m(), None, None),
        T("s_others_rep", "vec", R * N * (N - 1), lv, f64, COPY, None, oth(N * N, 1), (R * N, (N - 1) * lv)),
        T("a1_rep_m", "actions", R * N, A, i64, ONE_I, by_m(), None, None),
        T("env_next_rep", "next_grid", R * N, ne, f64, COPY, by_b(N * N), None, (R * N,) + g_sh),
        T("ot_next_rep", "next_obs_self_t", R * N, nt, f64, COPY, by_m(), None, (R * N,) + t_sh),
        T("ov_next_rep", "next_obs_self_v", R * N, nv, f64, COPY, by_m(), None, (R * N,) + v_sh),
        T("env_rep", "grid", R * N, ne, f64, COPY, by_b(N * N), None, (R * N,) + g_sh),
        T("ot_rep", "obs_self_t", R * N, nt, f64, COPY, by_m(), None, (R * N,) + t_sh),
        T("ov_rep", "obs_self_v", R * N, nv, f64, COPY, by_m(), None, (R * N,) + v_sh),
        # ---- the n x n x l_action counterfactual tiling (:700-760): each of the above repeated l_action times ----
        T("cf_s_n", "vec", R * N * A, lv, f64, COPY, by_n(A), None, None),
        T("cf_goals", "goals", R * N * A, lg, goals_dtype, COPY, by_n(A), None, None),
        T("cf_eye", None, R * N * A, A, f64, EYE, _IDENT, None, None),
        T("cf_s_m", "vec", R * N * A, lv, f64, COPY, by_m(A), None, None),
        T("cf_s_others", "vec", R * N * A * (N - 1), lv, f64, COPY, None, oth(N * N * A, A), (R * N * A, (N - 1) * lv)),
        T("cf_env", "grid", R * N * A, ne, f64, COPY, by_b(N * N * A), None, (R * N * A,) + g_sh),
        T("cf_ot", "obs_self_t", R * N * A, nt, f64, COPY, by_m(A), None, (R * N * A,) + t_sh),
        T("cf_ov", "obs_self_v", R * N * A, nv, f64, COPY, by_m(A), None, (R * N * A,) + v_sh),
    ]


_CHECKERS_WIDE = ("grid", "vec", "obs_others", "obs_self_t", "obs_self_v", "reward", "local_rewards", "next_grid", "next_vec",
                  "next_obs_others", "next_obs_self_t", "next_obs_self_v")


def checkers_static_feeds_apply(cols):
    """Whether checkers_static_feeds_device takes these columns: all on the GPU and contiguous, the wide ones float64, more than one
    agent, goals of a width the copy kernel moves (1, 4 or 8 bytes per element)."""
    vec = cols["vec"]
    return (vec.is_cuda and vec.dim() == 3 and vec.shape[1] > 1 and all(v.is_cuda and v.is_contiguous() for v in cols.values())
            and all(cols[n].dtype == torch.float64 for n in _CHECKERS_WIDE) and cols["goals"].element_size() in (1, 4, 8)
            and cols["done"].dtype in (torch.bool, torch.uint8) and not cols["actions"].dtype.is_floating_point
            and not cols["actions_prev"].dtype.is_floating_point)


def _particle_static_feeds_apply(cols):
    """Whether particle_static_feeds_device takes these columns: float32 on the GPU, more than one agent."""
    vg = cols["v_global"]
    return vg.is_cuda and vg.dtype == torch.float32 and vg.shape[1] > 1


def _static_feeds_device(cols, specs, out):
    """name -> device tensor for every TileSpec, 16 per launch of cm3_rows_tile, from the columns the specs name: action columns as
    flat int32, done as its bytes, the rest made contiguous.  out: the dict of an earlier call -- written into again."""
    src = {None: None}
    for name in (s.src for s in specs):
        if name in src:
            continue
        c = cols[name]
        if name in ("actions", "actions_prev"):
            src[name] = c.reshape(-1).to(torch.int32).contiguous()
        elif name == "done":
            c = c.contiguous()
            src[name] = c.view(torch.uint8) if c.dtype == torch.bool else c.to(torch.uint8)
        else:
            src[name] = c.contiguous()
    t = _Tiler(cols["goals"].device)
    S, O = {}, (out or {})
    for s in specs:
        S[s.name] = t.add(src[s.src], s.rows, s.epr, s.dtype, s.kind, terms=s.terms, others=s.others,
                          shape=s.shape, out=O.get(s.name))
    t.run()
    return S


def particle_static_feeds_device(cols, l_action=5, out=None):
    """Every feed of the reference's train_step that does not depend on a network output (particle env, N > 1, Q-credit variant), from
    the float32 columns of ParticleRollout.as_reference_batch(numpy=False) -- the 22 outputs of particle_static_feed_specs in TWO
    launches of cm3_rows_tile.  Values and dtypes are those of the torch composition (_static_feeds_composed; tests/test_batch.py
    compares the two and both with the arrays the REAL train_step fed).  out: the dict an earlier call returned for the same batch
    size -- the feeds are written into those tensors again (persistent addresses for a captured consumer)."""
    names = ("v_global", "goals", "reward", "reward_local")
    return _static_feeds_device(cols, particle_static_feed_specs({n: tuple(cols[n].shape) for n in names},
                                                                 {n: cols[n].dtype for n in names}, l_action), out)


def checkers_static_feeds_device(cols, l_action=5, out=None):
    """The Checkers twin of particle_static_feeds_device: every feed of alg_credit_checkers.train_step (:536-780; N > 1, Q-credit
    variant) that does not depend on a network output, from the 16 device columns of CheckersRollout.as_reference_batch(numpy=False)
    (wide columns float64, actions any integer type, goals as they come, done bool) -- the 33 outputs of checkers_static_feed_specs
    in THREE launches of cm3_rows_tile; the 432-byte grid rows and the 600-byte window rows take its row-granular path.  Values,
    shapes and dtypes are those of the torch composition in train_step_feeds (tests/test_gpu_checkers_static_feeds.py compares the
    two and both with the arrays the REAL train_step fed).  out: the dict an earlier call returned for the same batch size."""
    if not checkers_static_feeds_apply(cols):
        raise ValueError("checkers_static_feeds_device takes contiguous device columns, float64 wide ones, more than one agent "
                         "(checkers_static_feeds_apply); the torch composition of train_step_feeds covers the rest")
    return _static_feeds_device(cols, checkers_static_feed_specs({n: tuple(v.shape) for n, v in cols.items()}, cols["goals"].dtype,
                                                                 l_action), out)


def phase_static_feeds(cols_all, n_minibatches, l_action=5, env="particle"):
    """The static feeds of EVERY minibatch of an on-policy phase (train_onpolicy.py:359-377: 24 minibatches of 128) from the phase's
    one export (ParticleRollout.on_policy_phase: columns [n_minibatches * batch_size, ...]) -- ONE pair of cm3_rows_tile launches;
    returns a list of per-minibatch dicts of VIEWS (every feed is transition-major, so a minibatch is a contiguous block of rows).
    Round 5 built them per minibatch: 24 x 0.09 ms of launch latency for 0.13 ms of work.  env="checkers": the same over the export
    of CheckersRollout.on_policy_phase, from checkers_static_feeds_device (three launches)."""
    if env not in ("particle", "checkers"):
        raise ValueError("phase_static_feeds: env must be 'particle' or 'checkers', got %r" % (env,))
    S = _ENVS[env].static_device(cols_all, l_action)
    M = int(n_minibatches)
    out = []
    for k in range(M):
        d = {}
        for name, t in S.items():
            r = t.shape[0] // M
            d[name] = t[k * r:(k + 1) * r]
        out.append(d)
    return out


class OnPolicyPhasePlan(object):
    """One on-policy phase of the reference's loop (train_onpolicy.py:359-377: after a collection phase, 24 x (sample 128 transitions,
    train_step)) with PERSISTENT device tensors, so that the data movement of every train_step can be a hipGraph replay:

        plan = OnPolicyPhasePlan(rollout, run, gamma, epsilon)        # once
        rollout.collect(); plan.refresh(generator)                     # per phase: one export launch + one pair of tiling launches
        for k in range(plan.epochs): calls = plan.step(k)              # per minibatch: ONE graph replay

    refresh() draws the phase's minibatches and writes their columns and the static feeds of all of them INTO THE SAME tensors every
    phase; step(k) replays the graph captured from cm3_amd.batch.train_step_feeds(columns_k, run, gamma, epsilon, static=static_k) --
    every launch that function and `run` enqueue (the session's networks included, if `run` launches them on the current stream
    into tensors of its own that it keeps) -- and returns the same list of (ops, feed) with this phase's values in the same tensors.
    `run` is CALLED only while a graph is captured (the first step(k) of each k): it must not synchronise or allocate per call what
    it does not keep.  Without graphs (use_graph=False) step(k) simply calls train_step_feeds: the specification the replay is
    tested against (tests/test_batch.py::test_phase_plan_replays_equal_eager_feeds).

    rollout: a ParticleRollout (float32) or a CheckersRollout -- refresh() then tiles with checkers_static_feeds_device (three
    launches) and step(k) captures train_step_feeds(..., env="checkers", static=...); self.env names which.

    target_actor / actor: the device actors of train_step_feeds (ParticleActors or CheckersActors holding the Policy_target /
    Policy_main weights); their two rows launches are then part of the replayed graph and `run` is not called for
    ["action_samples_target"] / ["probs"].  A host-side draw counter would be frozen into the capture, so the plan samples through a
    cm3_amd.actor.RowsDrawCounter (draw_counter, or one of its own starting at 0; self.draw_counter): the captured launch reads the
    counter word from device memory and advances it itself, one draw per step(k) -- replayed or not.  The eager pass that precedes a
    capture consumes no draw (the counter is put back after it), so a graph plan and a use_graph=False plan that start from equal
    counters produce equal feeds and hold equal counters after any sequence of step(k).  The launches read the actors' persistent
    packed weights: ``target_actor.soft_update_from(actor, tau)`` between steps is seen by the next replay, as in eager mode.
    Every tensor the actors' calls allocate for a captured launch is held next to the step's calls (self._keep[k]) for as long as
    the graph lives.  Without actors nothing changes and no counter is made.

    q_global_target / q_credit_target / q_credit: the ParticleCritics (over a CheckersRollout: CheckersCritics) of train_step_feeds; their launches
    -- the three evaluations and the pack launch behind Q_credit_op -- become part of the replayed graph, and their tensors are held
    in self._keep[k] like the actors'.  `run` must write the Q_credit_main variables into q_credit.w[...] in place."""

    def __init__(self, rollout, run, gamma, epsilon, epochs=24, batch_size=128, l_action=5, use_graph=True, target_actor=None,
                 actor=None, draw_counter=None, q_global_target=None, q_credit_target=None, q_credit=None):
        self.ro, self.run, self.gamma, self.epsilon = rollout, run, float(gamma), float(epsilon)
        self.epochs, self.batch_size, self.l_action, self.use_graph = int(epochs), int(batch_size), int(l_action), bool(use_graph)
        self.cols = self.static = None
        self.k = 0
        self._graphs, self._calls, self._keep = {}, {}, {}
        self.target_actor, self.actor = target_actor, actor
        self.critics = {k: v for k, v in (("q_global_target", q_global_target), ("q_credit_target", q_credit_target),
                                          ("q_credit", q_credit)) if v is not None}
        self.draw_counter = draw_counter
        if self.draw_counter is None and target_actor is not None:
            from .actor import RowsDrawCounter
            self.draw_counter = RowsDrawCounter(target_actor.device)

    def refresh(self, generator=None):
        first = self.cols is None
        self.cols, self.k = self.ro._phase_export(self.epochs, self.batch_size, generator, out=self.cols)
        self.env = "checkers" if "vec" in self.cols else "particle"         # (a CheckersRollout exports the 16 Checkers columns)
        E = _ENVS[self.env]
        if not E.static_apply(self.cols):
            raise ValueError("OnPolicyPhasePlan covers %s with more than one agent (the tiling kernels' case)" % E.plan_covers)
        self.static = E.static_device(self.cols, self.l_action, out=self.static)
        if first:
            M, k = self.epochs, self.k
            self._mb = [({n: v[m * k:(m + 1) * k] for n, v in self.cols.items()},
                         {n: t[m * (t.shape[0] // M):(m + 1) * (t.shape[0] // M)] for n, t in self.static.items()}) for m in range(M)]
        return self

    def minibatch(self, k):
        """(columns, static feeds) of minibatch k: views of the persistent phase tensors"""
        return self._mb[k]

    def _feeds(self, k, keep):
        cols, static = self._mb[k]
        return train_step_feeds(cols, self.run, self.gamma, self.epsilon, l_action=self.l_action, static=static, env=self.env,
                                target_actor=self.target_actor, actor=self.actor,
                                draw=self.draw_counter if self.target_actor is not None else None, keep=keep, **self.critics)

    def step(self, k):
        from . import _lib
        cols, static = self._mb[k]
        if not self.use_graph:
            self._keep[k] = []
            return self._feeds(k, self._keep[k])
        dev = next(iter(cols.values())).device
        if k not in self._graphs:
            # once eagerly (the allocator then holds blocks of every size the capture will ask for), then captured; the tensors the
            # captured pass created are KEPT (self._calls, and self._keep for what the actors' launches touch): a replay writes to
            # their addresses.  The eager pass must not consume a draw: the counter goes back to what it was.
            draw0 = self.draw_counter.value() if self.target_actor is not None else None
            self._feeds(k, [])
            if draw0 is not None:
                self.draw_counter.set(draw0)
            torch.cuda.synchronize(dev)
            box = {"keep": []}

            def enqueue(stream):
                with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)):
                    box["calls"] = self._feeds(k, box["keep"])
            self._graphs[k] = _lib.capture_graph(dev, enqueue)
            self._calls[k], self._keep[k] = box["calls"], box["keep"]
        _lib.check(_lib.lib().cm3_graph_launch(self._graphs[k], torch.cuda.current_stream(dev).cuda_stream))
        return self._calls[k]

    def close(self):
        from . import _lib
        if self._graphs:
            torch.cuda.synchronize()
            for g in self._graphs.values():
                _lib.lib().cm3_graph_destroy(g)
        self._graphs, self._calls, self._keep = {}, {}, {}


def td_target(reward, q, multiplier, gamma):
    """reward + gamma * q * multiplier in NumPy's order (alg_credit.py:594, :640, :684), float64: one launch of cm3_td_target_f64 for
    device tensors (reward float32 / float64, multiplier int64), the torch composition otherwise -- the same bits."""
    q = q.reshape(-1)
    if (q.is_cuda and q.dtype == torch.float64 and q.is_contiguous() and multiplier.dtype == torch.int64 and multiplier.is_contiguous()
            and reward.dtype in (torch.float32, torch.float64) and reward.is_contiguous() and reward.numel() == q.numel()):
        from . import _lib
        out = torch.empty_like(q)
        _lib.check(_lib.lib().cm3_td_target_f64(reward.data_ptr(), 1 if reward.dtype == torch.float64 else 0, q.data_ptr(),
                                                multiplier.data_ptr(), float(gamma), out.data_ptr(), q.numel(),
                                                torch.cuda.current_stream(q.device).cuda_stream))
        return out
    return reward.to(torch.float64) + gamma * q * multiplier


def process_actions_device(acts, n_steps, n_agents, l_action=5, rep_m=False, keep=None):
    """process_actions(acts.reshape(n_steps, N)) -- and optionally the one-hot rows repeated N times (`rep_m`, alg_credit.py:628) -- in
    ONE cm3_rows_tile launch for a device tensor of sampled actions (any integer dtype).  keep: an optional list that receives the
    int32 form of the actions the launch reads (a temporary unless acts is flat int32) -- whoever captures the launch holds it."""
    from . import _lib
    N, A, R = n_agents, int(l_action), n_steps * n_agents
    a32 = acts.reshape(-1).to(torch.int32).contiguous()
    _keep(keep, a32)
    t = _Tiler(acts.device)
    one = t.add(a32, R, A, torch.int64, _lib.TILE_ONEHOT_I64)
    others = t.add(a32, R * (N - 1), A, torch.float64, _lib.TILE_ONEHOT_F64, others=(N, N * (N - 1), N - 1), shape=(R, N - 1, A))
    rep = t.add(a32, R * N, A, torch.int64, _lib.TILE_ONEHOT_I64, terms=((N, 0, 1), (1, 0, 0))) if rep_m else None
    t.run()
    return one, others, rep


def others_index(n_agents, device=None):
    """[N, N-1] long: row n lists the other agents in ascending order (np.arange(N) != n)."""
    idx = [[j for j in range(n_agents) if j != n] for n in range(n_agents)]
    return torch.tensor(idx, dtype=torch.long, device=device).reshape(n_agents, max(n_agents - 1, 0))


def gather_others(x):
    """x [B, N, d] -> [B*N, N-1, d]: row b*N+n holds x[b, m] for the agents m != n in ascending order
    (the reference's `out[n::N] = x[:, np.arange(N) != n]` interleave)."""
    B, N = x.shape[0], x.shape[1]
    idx = others_index(N, x.device)
    return x[:, idx].reshape(B * N, N - 1, *x.shape[2:])


def process_actions(actions, l_action=5):
    """actions int [B, N] -> (actions_1hot int64 [B*N, A], actions_others_1hot float64 [B*N, N-1, A])
    (alg_credit.py:406-443; dtypes as the reference: np.zeros(dtype=int) and np.zeros default float64)."""
    B, N = actions.shape
    one = torch.nn.functional.one_hot(actions.long(), l_action)            # [B, N, A] int64
    others = gather_others(one).to(torch.float64)
    return one.reshape(B * N, l_action), others


def process_goals(goals):
    """goals [B, N, l_goal] -> (goals_self [B*N, l_goal], goals_others [B*N, (N-1)*l_goal]) (alg_credit.py:501-526)."""
    B, N, lg = goals.shape
    return goals.reshape(B * N, lg), gather_others(goals).reshape(B * N, (N - 1) * lg).to(torch.float64)


def process_global_state(v_global):
    """v_global [B, N, l] -> (one_agent [B*N, l], others [B*N, (N-1)*l], state [B*N, N*l]) (alg_credit.py:528-557)."""
    B, N, l = v_global.shape
    one = v_global.reshape(B * N, l)
    others = gather_others(v_global).reshape(B * N, (N - 1) * l).to(torch.float64)
    state = rep_rows(v_global.reshape(B, N * l), N)
    return one, others, state


def process_batch(cols, l_action=5):
    """Columns of ParticleRollout.as_reference_batch(numpy=False) -> the 13-tuple of alg_credit.process_batch
    (alg_credit.py:445-499): per-agent rows, global quantities repeated N times."""
    v_global = cols["v_global"]
    B, N = v_global.shape[0], v_global.shape[1]
    a1, ao = process_actions(cols["actions"], l_action)
    return (B, v_global, cols["obs_others"].reshape(B * N, -1), cols["v_local"].reshape(B * N, -1), a1, ao,
            rep_rows(cols["reward"], N), cols["reward_local"].reshape(B * N),
            cols["v_global_next"], cols["obs_others_next"].reshape(B * N, -1), cols["v_local_next"].reshape(B * N, -1),
            rep_rows(cols["done"], N), cols["goals"])


def repeat_indexed_by_n(x, n_agents):
    """[B*N, d] -> [B*N*N, d]: each time step's block of N rows repeated N times (alg_credit.py:621-623, :648-649)."""
    d = x.shape[1:]
    return rep_rows(x.reshape(-1, n_agents, *d), n_agents).reshape(-1, *d)


def repeat_indexed_by_m(x, n_agents):
    """[B*N, d] -> [B*N*N, d]: every row repeated N times consecutively (alg_credit.py:628-629, :651-652)."""
    return rep_rows(x, n_agents)


# ---- Checkers (alg_credit_checkers.py:375-535) ---------------------------------------------------------------------------

def process_batch_checkers(cols, l_action=5):
    """Columns of CheckersRollout.as_reference_batch(numpy=False) -> the 18-tuple of
    alg_credit_checkers.Alg.process_batch (alg_credit_checkers.py:414-482): per-agent rows; grid and done repeated N
    times, `reward` left per time step (unlike the particle variant), both action columns one-hot."""
    vec = cols["vec"]
    B, N = vec.shape[0], vec.shape[1]
    rep = lambda x: rep_rows(x, N)                             # noqa: E731
    rows = lambda x: x.reshape(B * N, *x.shape[2:])            # noqa: E731
    a1, ao = process_actions(cols["actions"], l_action)
    prev1 = torch.nn.functional.one_hot(cols["actions_prev"].long(), l_action).reshape(B * N, l_action)
    return (B, rep(cols["grid"]), vec, rows(cols["obs_others"]), rows(cols["obs_self_t"]), rows(cols["obs_self_v"]),
            prev1, a1, ao, cols["reward"], cols["local_rewards"].reshape(B * N), rep(cols["next_grid"]),
            cols["next_vec"], rows(cols["next_obs_others"]), rows(cols["next_obs_self_t"]),
            rows(cols["next_obs_self_v"]), rep(cols["done"]), cols["goals"])


CHECKERS_BATCH_NAMES = ("n_steps", "state_env", "state_agents", "obs_others", "obs_self_t", "obs_self_v",
                        "actions_prev_1hot", "actions_1hot", "actions_others_1hot", "reward", "reward_local",
                        "state_env_next", "state_agents_next", "obs_others_next", "obs_self_t_next", "obs_self_v_next",
                        "done", "goals")
# process_goals / process_global_state of alg_credit_checkers.py:484-535 are the particle functions above, verbatim
# in behaviour (l_goal = 2, l_state_one_agent = 4): use process_goals(goals) and process_global_state(state_agents).


# ---- every feed_dict of train_step (alg_credit.py:558-800, alg_credit_checkers.py:536-780) -------------------------------

PARTICLE_BATCH_NAMES = ("n_steps", "v_global", "obs_others", "v_local", "actions_1hot", "actions_others_1hot", "reward", "reward_local",
                        "v_global_next", "obs_others_next", "v_local_next", "done", "goals")


class _Particle(object):
    """What train_step_feeds needs to know about the env -- column names, the feeds' keys, the static-feed builders -- as data."""
    next_fmt, state, reward_local = "%s_next", "v_global", "reward_local"
    actor_cols = ("obs_others", "v_local")                      # the actors' observation columns, in their rows methods' order
    feed_keys = ("obs_others", "v_obs")                         # ... and the placeholders they feed
    actions_prev = False                                        # the actors take no previous action
    critic_head, critic_tail = ("v_global",), ()                # the critics' columns before (goals, actions) and after them
    env_keys = ()                                               # placeholders of the env's own state: none
    static_apply, static_device = staticmethod(_particle_static_feeds_apply), staticmethod(particle_static_feeds_device)
    plan_covers = "float32 device rollouts"
    process_batch, batch_names = staticmethod(process_batch), PARTICLE_BATCH_NAMES
    # the composed static dict: entries taken from process_batch, entries repeated by m, entries repeated l_action times
    from_batch = (("a1", "actions_1hot"), ("ao", "actions_others_1hot"), ("reward_rep", "reward"), ("done_rep", "done"))
    env_rep_m, env_rep_a = (), ()


class _Checkers(object):
    next_fmt, state, reward_local = "next_%s", "vec", "local_rewards"
    actor_cols = feed_keys = ("obs_self_t", "obs_self_v", "obs_others")
    actions_prev = True                                         # ... and the previous action (one-hot in the feed, an index to an actor)
    critic_head, critic_tail = ("grid", "vec"), ("obs_self_t", "obs_self_v")
    env_keys = ("state_env", "obs_self_t", "obs_self_v")
    static_apply, static_device = staticmethod(checkers_static_feeds_apply), staticmethod(checkers_static_feeds_device)
    plan_covers = "Checkers device rollouts"
    process_batch, batch_names = staticmethod(process_batch_checkers), CHECKERS_BATCH_NAMES
    from_batch = (("state_env", "state_env"), ("state_env_next", "state_env_next"), ("a1", "actions_1hot"),
                  ("ao", "actions_others_1hot"), ("prev1", "actions_prev_1hot"), ("done_rep", "done"))
    env_rep_m = (("env_next_rep", "state_env_next"), ("ot_next_rep", "obs_self_t_next"), ("ov_next_rep", "obs_self_v_next"),
                 ("env_rep", "state_env"), ("ot_rep", "obs_self_t"), ("ov_rep", "obs_self_v"))
    env_rep_a = (("cf_env", "env_rep"), ("cf_ot", "ot_rep"), ("cf_ov", "ov_rep"))


_ENVS = {"particle": _Particle, "checkers": _Checkers}


class _Recorder(object):
    """Plays sess.run for the feed builders: call(ops, feed) records (ops, feed) in self.calls and returns run(ops, feed) -- or, with
    launch=False (a device network answers instead), None."""

    def __init__(self, run):
        self.run, self.calls = run, []

    def __call__(self, ops, feed, launch=True):
        self.calls.append((ops, feed))
        return self.run(ops, feed) if launch else None


def _static_feeds_composed(cols, E, l_action, credit):
    """The dict of particle_static_feeds_device / checkers_static_feeds_device -- the same names, shapes, dtypes and bits
    (tests/test_static_feeds_composed.py) -- from torch's own gathers and repeats, as the reference composes them: the specification
    the tiling kernels are tested against, and the path of the inputs they do not take (host tensors, float64 particle columns, one
    agent, device_tiling=False, the variants without Q-credit).  Per agent row always; the n x n credit repeats and the n x n x
    l_action counterfactual tiling only with `credit`."""
    T = dict(zip(E.batch_names, E.process_batch(cols, l_action)))
    S = {name: T[src] for name, src in E.from_batch}
    v_global, v_global_next, goals = cols[E.state], cols[E.next_fmt % E.state], cols["goals"]
    B, N = v_global.shape[0], v_global.shape[1]
    one, S["others"], _ = process_global_state(v_global)
    one_next, S["others_next"], _ = process_global_state(v_global_next)
    S["not_done"] = -(S["done_rep"].to(torch.int64) - 1)                            # if true, then 0, else 1 (:590)
    if not credit:
        return S
    rep_n = lambda x: repeat_indexed_by_n(x, N)                                     # noqa: E731  things indexed by n (:621-623)
    rep_m = lambda x: repeat_indexed_by_m(x, N)                                     # noqa: E731  things indexed by m (:628-629)
    rep_a = lambda x: rep_rows(x, l_action)                                         # noqa: E731
    S["goals_self_rep"] = rep_n(goals.reshape(-1, goals.shape[2]))
    S["one_next_rep_n"], S["one_next_rep_m"], S["others_next_rep_n"] = rep_n(one_next), rep_m(one_next), rep_n(S["others_next"])
    S["r_rep"] = rep_n(T["reward_local"].reshape(-1, 1)).reshape(-1)
    S["nd_rep"] = -(rep_n(S["done_rep"].reshape(-1, 1).to(torch.int64)).reshape(-1) - 1)
    S["s_n_rep"], S["s_others_rep"], S["s_m_rep"] = rep_n(one), rep_n(S["others"]), rep_m(one)
    S["a1_rep_m"] = rep_m(S["a1"])
    S.update((name, rep_m(T[src])) for name, src in E.env_rep_m)
    eye = torch.eye(l_action, dtype=torch.float64, device=one.device)               # self.actions = np.eye(l_action)
    S["cf_s_n"], S["cf_goals"], S["cf_eye"] = rep_a(S["s_n_rep"]), rep_a(S["goals_self_rep"]), eye.repeat(N * N * B, 1)
    S["cf_s_m"], S["cf_s_others"] = rep_a(S["s_m_rep"]), rep_a(S["s_others_rep"])
    S.update((name, rep_a(S[src])) for name, src in E.env_rep_a)
    return S


def train_step_feeds(cols, run, gamma, epsilon, env="particle", use_Q_credit=True, use_V=True, l_action=5, device_tiling=True,
                     static=None, target_actor=None, actor=None, draw=None, keep=None, q_global_target=None, q_credit_target=None,
                     q_credit=None):
    """The data movement of the reference's train_step on the device: builds, in the reference's order, the feed_dict of
    every sess.run -- TD targets, the n x n credit repeats (alg_credit.py:614-658) and the n x n x l_action counterfactual
    tiling (:730-751; Checkers twin alg_credit_checkers.py:590-760) -- from the columns of
    {Particle,Checkers}Rollout.as_reference_batch(numpy=False).

    ``run(ops, feed)`` plays sess.run: `ops` is a list of the reference's op attribute names (e.g. ["Q_global_op",
    "Q_global"]), `feed` a dict keyed by the reference's placeholder attribute names; it returns one tensor per op (None
    for optimiser ops).  Returns the list of (ops, feed) in call order.  Pure gathers / repeats plus the float64 TD
    arithmetic: bit-identical to the arrays the REAL train_step feeds (tests/golden/trainstep_*.npz, recorded by
    oracle/gen_golden_trainstep.py from the reference code itself under a recording session).
    static: this minibatch's entry of phase_static_feeds() -- the static feeds then cost no launch here.  Both envs: float32 particle
    columns (particle_static_feeds_device, two launches) and float64 Checkers columns (checkers_static_feeds_device, three) on the GPU
    take the tiling kernel by default; device_tiling=False, host tensors, N = 1 and the variants without Q-credit the composition.

    target_actor / actor (CUDA columns): device actors holding the Policy_target / Policy_main weights -- ParticleActors for the
    particle env, CheckersActors for env="checkers" (an actor of the other env's class is refused).  With target_actor, `run` is NOT
    called for ["action_samples_target"] (its (ops, feed) entry still appears in the list): the samples come in one launch from
    target_actor.sample_rows(obs_others_next, v_local_next, goals, epsilon), on Checkers from
    target_actor.sample_rows(next_obs_self_t, next_obs_self_v, next_obs_others, cols["actions"], goals, epsilon) (the reference
    feeds the action just taken as actions_prev there, alg_credit_checkers.py:551) -- the build's own rows stream, equal to
    tf.multinomial in law only -- and go on through the same one-hot paths.  With actor, the same holds for
    ["probs"], from actor.probs_rows(obs_others, v_local, goals, epsilon), on Checkers from
    actor.probs_rows(obs_self_t, obs_self_v, obs_others, cols["actions_prev"], goals, epsilon).  epsilon: a float, or the one-element
    float32 device tensor the actors accept.  The soft update of the target actor -- the actor half of list_update_target_ops -- is
    left to the caller: ``target_actor.soft_update_from(actor, tau)`` after this function returns.  With both None nothing changes.
    draw / keep go to the actors' calls as they are: draw is sample_rows' (None: the target actor's host counter; an integer; or a
    cm3_amd.actor.RowsDrawCounter, the device counter a captured launch advances itself), keep the list that receives every tensor
    sample_rows / probs_rows allocate for their launches (OnPolicyPhasePlan holds them while it replays the capture).

    q_global_target / q_credit_target / q_credit (CUDA columns): cm3_amd.critic.ParticleCritics -- for env="checkers" CheckersCritics;
    a critic of the other env's class is refused -- holding the Q_global_target / Q_credit_target / Q_credit_main weights, for the
    batch's agent count.  On Checkers the launches read next_grid / next_vec / next_obs_self_t / next_obs_self_v (the two targets,
    with local_rewards and done) and grid / vec / obs_self_t / obs_self_v (the counterfactual) next to goals and the actions; the
    window and obs_self_v of a pair row are agent m's, as the reference repeats them.  With one given, `run` is NOT called for
    its op (the (ops, feed) entry still appears in the list) and the evaluation is one launch on the batch's base columns:
      ["Q_global_target"]  q_global_target.q_rows(v_global_next, goals, a', reward_local, done, gamma); its "td" is the
                           Q_global_td_target feed (kind "global")
      ["Q_credit_target"]  q_credit_target.q_pairs(...), likewise; its "td" is the Q_credit_td_target feed (kind "credit")
      ["Q_credit"]         the counterfactual Q_cf = q_credit.q_counterfactual(v_global, goals) (kind "credit").  With ONE agent
                           (stage 1) the counterfactual op is ["Q_global"] on the Q_global_main weights: q_credit then takes a
                           kind "global" critic -- the same argument, no fourth one.
    The reference evaluates the counterfactual AFTER the optimiser step on the main critic (alg_credit.py:660, then :750; with one
    agent :601, then :726), so q_credit.repack() is launched right after call(["Q_credit_op"], ...) (one agent: after
    call(["Q_global_op", "Q_global"], ...)).  CONTRACT: `run` writes the updated variables INTO q_credit.w[...] in place (the
    tensors are persistent, the pack launch capturable).  The soft updates of the two target critics -- their part of
    list_update_target_ops -- are the caller's: ``q_global_target.soft_update_from(main, tau)`` after this function returns.  keep
    receives the tensors of these launches too.  With all three None nothing changes: not a launch, not a bit."""
    checkers = env == "checkers"
    E = _ENVS["checkers" if checkers else "particle"]
    critics = (("q_global_target", q_global_target), ("q_credit_target", q_credit_target), ("q_credit", q_credit))
    if any(c is not None for _, c in critics):
        from .critic import CheckersCritic, ParticleCritic
        cls = CheckersCritic if checkers else ParticleCritic
        if checkers:        # (before the columns are read)
            for name, c in critics:
                if isinstance(c, ParticleCritic):
                    raise ValueError("train_step_feeds: %s is a ParticleCritic; env='checkers' has no device critics of that class, "
                                     "pass CheckersCritics" % name)
        base = cols[E.state]
        n_batch = base.shape[1]
        for name, c in critics:
            if c is None:
                continue
            want = "global" if (name == "q_global_target" or n_batch == 1) else "credit"
            if not isinstance(c, cls) or c.kind != want or c.n != n_batch:
                raise ValueError("train_step_feeds: %s takes a %s of kind %r for %d agents, got %s"
                                 % (name, cls.__name__, want, n_batch, "a %s" % type(c).__name__ if not isinstance(c, cls)
                                    else "kind %r for %d agents" % (c.kind, c.n)))
        if not base.is_cuda:
            raise ValueError("train_step_feeds: q_global_target / q_credit_target / q_credit evaluate device columns; call without "
                             "them for host tensors")
    if target_actor is not None or actor is not None:
        from .actor import CheckersActor
        for a in (target_actor, actor):
            if a is not None and isinstance(a, CheckersActor) != checkers:
                raise ValueError("train_step_feeds: env=%r takes %s as target_actor / actor, got a %s"
                                 % (env, "CheckersActors" if checkers else "ParticleActors", type(a).__name__))
        if not cols["obs_others"].is_cuda:
            raise ValueError("train_step_feeds: target_actor / actor evaluate device columns; call without them for host tensors")

    # (draw / keep reach the actors only when given: a call without them is the call of before)
    probs_kw = {} if keep is None else {"keep": keep}
    sample_kw = dict(probs_kw) if draw is None else dict(probs_kw, draw=draw)
    call = _Recorder(run)
    f64 = torch.float64
    v_global, goals = cols[E.state], cols["goals"]
    n_steps, N = v_global.shape[0], v_global.shape[1]
    credit = N > 1 and use_Q_credit
    # S: every feed that does not depend on a network output, under the names of the spec tables.  Columns the tiling kernels take
    # (float32 particle / float64 Checkers on the GPU, N > 1, Q-credit) come from cm3_rows_tile -- or from `static`, at no launch
    # here; everything else from the torch composition, the specification both are tested against
    tiled = static is not None or bool(use_Q_credit and device_tiling and E.static_apply(cols))
    S = static if static is not None else (E.static_device(cols, l_action) if tiled
                                           else _static_feeds_composed(cols, E, l_action, credit))
    rows = lambda x: x.reshape(n_steps * N, *x.shape[2:])                           # noqa: E731
    col = lambda name, nxt=False: cols[E.next_fmt % name if nxt else name]          # noqa: E731
    v_global_next, reward_local = col(E.state, True), cols[E.reward_local].reshape(n_steps * N)
    obs = {nxt: tuple(rows(col(name, nxt)) for name in E.actor_cols) for nxt in (False, True)}
    goals_self = goals.reshape(-1, goals.shape[2])
    one, one_next = v_global.reshape(-1, v_global.shape[2]), v_global_next.reshape(-1, v_global_next.shape[2])
    X = dict(S)                     # ... and the per-agent observation rows, for with_env
    X.update(zip(E.actor_cols, obs[False]))
    X.update(zip((name + "_next" for name in E.actor_cols), obs[True]))

    def actor_feed(nxt):
        """the feed of an actor op on this step's (the next step's) observation"""
        feed = dict(zip(E.feed_keys, obs[nxt]), v_goal=goals_self, epsilon=epsilon)
        if E.actions_prev:          # run_actor_target(actions_1hot, obs_others_next, ...) (alg_credit_checkers.py:551)
            feed["actions_prev"] = S["a1"] if nxt else S["prev1"]
        return feed

    def actor_args(nxt):
        """the same as the arguments of a device actor's rows methods"""
        prev = (cols["actions" if nxt else "actions_prev"].reshape(-1),) if E.actions_prev else ()
        return obs[nxt] + prev + (goals_self, epsilon)

    def with_env(feed, *names, f=lambda x: x):
        """Checkers: the env's state and the windows under state_env / obs_self_t / obs_self_v; particle: nothing"""
        feed.update((key, f(X[name])) for key, name in zip(E.env_keys, names))
        return feed

    def critic_cols(nxt):
        """the base columns a device critic decodes its rows from, as (those before the actions, those after them)"""
        return tuple(col(name, nxt) for name in E.critic_head) + (goals,), tuple(col(name, nxt) for name in E.critic_tail)

    def td(reward, q, multiplier):
        """reward + gamma * q * multiplier, float64 (:594, :640, :684): one launch next to the tiled feeds, torch's own otherwise"""
        return td_target(reward, q, multiplier, gamma) if tiled else reward.to(f64) + gamma * q.reshape(-1) * multiplier

    # ---- Q_n(s, a): target actions a', TD target, optimiser step (alg_credit.py:574-612) ----
    if target_actor is None:
        acts = call(["action_samples_target"], actor_feed(True))[0]
    else:
        call(["action_samples_target"], actor_feed(True), launch=False)
        acts = target_actor.sample_rows(*actor_args(True), **sample_kw)["actions"]
    if tiled and acts.is_cuda:      # one launch: both one-hot forms and the rows repeated by m (Q-credit target, :628)
        a_next, a_others_next, a_next_rep = process_actions_device(acts, n_steps, N, l_action, rep_m=credit, keep=keep)
    else:
        a_next, a_others_next, a_next_rep = process_actions(acts.reshape(n_steps, N), l_action) + (None,)
    feed = with_env({"v_state_one_agent": one_next, "v_goal": goals_self, "action_one": a_next,
                     "v_state_other_agents": S["others_next"], "action_others": a_others_next},
                    "state_env_next", "obs_self_t_next", "obs_self_v_next")
    if q_global_target is not None:     # one launch on the base columns: Q and the TD target
        call(["Q_global_target"], feed, launch=False)
        head, tail = critic_cols(True)
        td_g = q_global_target.q_rows(*head, acts, *tail, reward_local, cols["done"], gamma, **probs_kw)["td"]
    else:
        td_g = td(reward_local, call(["Q_global_target"], feed)[0], S["not_done"])
    q_res = call(["Q_global_op", "Q_global"],
                 with_env({"Q_global_td_target": td_g, "v_state_one_agent": one, "v_goal": goals_self, "action_one": S["a1"],
                           "v_state_other_agents": S["others"], "action_others": S["ao"]},
                          "state_env", "obs_self_t", "obs_self_v"))[1]
    if N == 1 and q_credit is not None:
        q_credit.repack()           # (one agent: the counterfactual below reads the Q_global_main weights this step updated)
    q_res_rep = rep_rows(q_res.reshape(n_steps, N), N)                              # :612

    if credit:                      # ---- Q_n(s, a^m) (:616-674): things indexed by n repeat per block, things indexed by m row by row ----
        feed = with_env({"v_state_one_agent": S["one_next_rep_n"], "v_goal": S["goals_self_rep"],
                         "action_one": rep_rows(a_next, N) if a_next_rep is None else a_next_rep,
                         "v_state_m": S["one_next_rep_m"], "v_state_other_agents": S["others_next_rep_n"]},
                        "env_next_rep", "ot_next_rep", "ov_next_rep")
        if q_credit_target is not None:
            call(["Q_credit_target"], feed, launch=False)
            head, tail = critic_cols(True)
            td_c = q_credit_target.q_pairs(*head, acts, *tail, reward_local, cols["done"], gamma, **probs_kw)["td"]
        else:
            td_c = td(S["r_rep"], call(["Q_credit_target"], feed)[0], S["nd_rep"])
        call(["Q_credit_op"], with_env({"Q_credit_td_target": td_c, "v_state_one_agent": S["s_n_rep"], "v_goal": S["goals_self_rep"],
                                        "action_one": S["a1_rep_m"], "v_state_m": S["s_m_rep"],
                                        "v_state_other_agents": S["s_others_rep"]}, "env_rep", "ot_rep", "ov_rep"))
        if q_credit is not None:
            q_credit.repack()       # (the counterfactual below reads the Q_credit_main weights this step updated)
    v_res_rep = None
    if N > 1 and use_V:             # ---- V_n(s) (:676-699) ----
        v_t = call(["V_target"], with_env({"v_state_one_agent": one_next, "v_goal": goals_self,
                                           "v_state_other_agents": S["others_next"]}, "state_env_next"))[0]
        v_res = call(["V_op", "V"], with_env({"V_td_target": td(reward_local, v_t, S["not_done"]), "v_state_one_agent": one,
                                              "v_goal": goals_self, "v_state_other_agents": S["others"]}, "state_env"))[1]
        v_res_rep = rep_rows(v_res.reshape(n_steps, N), N)

    # ---- policy: probabilities + counterfactual Q for every action (:704-757) ----
    def fetch_probs():
        if actor is None:
            return call(["probs"], actor_feed(False))[0]
        call(["probs"], actor_feed(False), launch=False)
        return actor.probs_rows(*actor_args(False), **probs_kw)

    def counterfactual(op, feed, n_rows):
        if q_credit is None:
            return call([op], feed)[0].reshape(n_rows, l_action)
        call([op], feed, launch=False)
        head, tail = critic_cols(False)
        return q_credit.q_counterfactual(*head, *tail, **probs_kw)

    if N == 1:                      # stage 1: Q(s, a = every action, g)
        probs = fetch_probs()
        rep_a = lambda x: rep_rows(x, l_action)                                     # noqa: E731
        eye = torch.eye(l_action, dtype=f64, device=one.device)                     # self.actions = np.eye(l_action)
        q_cf = counterfactual("Q_global", with_env({"v_state_one_agent": rep_a(one), "v_goal": rep_a(goals_self),
                                                    "action_one": eye.repeat(n_steps, 1), "v_state_other_agents": S["others"],
                                                    "action_others": S["ao"]}, "state_env", "obs_self_t", "obs_self_v", f=rep_a),
                              n_steps)
    elif use_Q_credit:
        probs = rep_rows(fetch_probs(), N)
        q_cf = counterfactual("Q_credit", with_env({"v_state_one_agent": S["cf_s_n"], "v_goal": S["cf_goals"], "action_one": S["cf_eye"],
                                                    "v_state_m": S["cf_s_m"], "v_state_other_agents": S["cf_s_others"]},
                                                   "cf_env", "cf_ot", "cf_ov"), n_steps * N * N)
    else:
        probs = torch.zeros(1, l_action, dtype=f64, device=one.device)
        q_cf = torch.zeros(1, l_action, dtype=f64, device=one.device)
    feed = actor_feed(False)
    feed.update({"action_taken": S["a1"], "Q_actual": q_res_rep, "probs_evaluated": probs, "Q_cf": q_cf})
    if N > 1 and use_V:
        feed["V_evaluated"] = v_res_rep
    call(["policy_op"], feed)
    call(["list_update_target_ops"], {})
    return call.calls


# ---- the IAC / COMA baselines (alg_baseline.py:507-655, particle env; alg_baseline_checkers.py:499-662, Checkers) -----------------

def _baseline_check_networks(cols, IAC, v_target, v_main, q_target, q_main, target_actor, actor, checkers=False):
    """The refusals of baseline_train_step_feeds, before any column is read beyond the agent count."""
    state = "vec" if checkers else "v_global"
    given = lambda *xs: [x is not None for x in xs]                                  # noqa: E731
    if any(given(v_target, v_main)) and not all(given(v_target, v_main)):
        raise ValueError("baseline_train_step_feeds: v_target and v_main come together (the reference fetches V_target and V in one "
                         "sess.run) or not at all")
    if any(given(q_main, actor)) and not all(given(q_main, actor)):
        raise ValueError("baseline_train_step_feeds: q_main and actor come together (the reference fetches Q and probs in one "
                         "sess.run) or not at all")
    nets = (("v_target", v_target), ("v_main", v_main), ("q_target", q_target), ("q_main", q_main))
    if not any(given(v_target, v_main, q_target, q_main, target_actor, actor)):
        return
    n_batch = cols[state].shape[1]
    if any(c is not None for _, c in nets):
        from . import baseline
        Value = baseline.CheckersValue if checkers else baseline.ParticleValue
        Coma = baseline.CheckersComaCritic if checkers else baseline.ParticleComaCritic
        kind = "local" if IAC else "global"
        for name, c in nets:
            if c is None:
                continue
            if name.startswith("v_"):
                if not isinstance(c, Value) or c.kind != kind or c.n != n_batch:
                    raise ValueError("baseline_train_step_feeds: %s takes a %s of kind %r for %d agents (IAC=%s), got %s"
                                     % (name, Value.__name__, kind, n_batch, bool(IAC),
                                        "a %s" % type(c).__name__ if not isinstance(c, Value) else "kind %r for %d agents" % (c.kind, c.n)))
            elif not isinstance(c, Coma) or c.n != n_batch:
                raise ValueError("baseline_train_step_feeds: %s takes a %s for %d agents, got %s"
                                 % (name, Coma.__name__, n_batch, "a %s" % type(c).__name__ if not isinstance(c, Coma)
                                    else "one for %d agents" % c.n))
    if target_actor is not None or actor is not None:
        from . import actor as _actor
        Actor = _actor.CheckersActor if checkers else _actor.ParticleActor
        for a in (target_actor, actor):
            if a is not None and not isinstance(a, Actor):
                raise ValueError("baseline_train_step_feeds: target_actor / actor take %ss, got a %s" % (Actor.__name__, type(a).__name__))
    if not cols[state].is_cuda:
        raise ValueError("baseline_train_step_feeds: the device networks evaluate device columns; call without them for host tensors")


def baseline_train_step_feeds(cols, run, gamma, epsilon, IAC=False, use_Q=1, use_V=1, l_action=5, target_actor=None, actor=None,
                              v_target=None, v_main=None, q_target=None, q_main=None, draw=None, keep=None, env="particle"):
    """The data movement of alg_baseline.Alg.train_step (alg_baseline.py:507-655; IAC and COMA, particle env), in the reference's
    call order, from the columns of ParticleRollout.as_reference_batch(numpy=False).  ``run(ops, feed)`` and the returned list of
    (ops, feed) mean what they mean in train_step_feeds; IAC / use_Q / use_V are the reference's switches (IAC: IAC=True, use_V=1,
    use_Q=0; COMA: use_Q=1, use_V=0; both critics: use_Q=1, use_V=1).

    With every device network None this is the torch composition alone -- process_goals and process_global_state in their baseline
    forms (:450-505), agent_labels, the TD targets and the three policy feeds of :618-647 -- bit-identical to the arrays the REAL
    train_step feeds (tests/golden/trainstep_baseline_*.npz).

    With a device network (CUDA columns) `run` is NOT called for its op; the (ops, feed) entry still appears in the list:
      ["V_target", "V"]            v_target / v_main, cm3_amd.baseline.ParticleValues of kind "local" with IAC, "global" without,
        (:534)                     both or neither: v_target.v_rows(next-step columns, reward_local, done, gamma)["td"] is the
                                   V_td_target feed; the same launch on v_main gives V_next_res ("v64") and the policy's V_td_target
      ["action_samples_target"]    target_actor.sample_rows(obs_others_next, v_local_next, goals, epsilon), as in train_step_feeds
      ["Q_target"] (:576)          q_target, a ParticleComaCritic: q_target.q_rows(v_global_next, goals, a', v_local_next, reward,
                                   done, gamma)["td"] is the Q_td_target feed (the GLOBAL reward)
      ["Q", "probs"] (:616)        q_main and actor, both or neither: q_main.q_rows(v_global, goals, actions, v_local)["q"] and
                                   actor.probs_rows(obs_others, v_local, goals, epsilon)
    CONTRACT, as for q_credit in train_step_feeds: `run` writes the trained variables INTO v_main.w[...] / q_main.w[...] in place;
    v_main.repack() is launched right after call(["V_op", "V"]) and q_main.repack() right after call(["Q_op"]) (the reference reads Q
    after that optimiser step).  The soft updates stay the caller's.  A ParticleValue of the wrong kind for IAC, or a network of the
    wrong agent count or class, is refused before any column is read.  draw / keep: as in train_step_feeds.

    env="checkers": alg_baseline_checkers.Alg.train_step (alg_baseline_checkers.py:499-662) on the 16 columns of
    CheckersRollout.as_reference_batch(numpy=False), bit-identical to tests/golden/trainstep_baseline_checkers_*.npz.  The device
    networks are then cm3_amd.baseline.CheckersValues / CheckersComaCritics and CheckersActors (a network of the other env's class is
    refused before any column is read), on the base columns:
      ["V_target", "V"]            v_rows(next_obs_self_t, next_obs_self_v, next_obs_others, goals, local_rewards, done, gamma) with IAC,
                                   v_rows(next_grid, next_vec, goals, local_rewards, done, gamma) without
      ["action_samples_target"]    target_actor.sample_rows(next_obs_self_t, next_obs_self_v, next_obs_others, actions, goals, epsilon):
                                   actions_prev is the action just taken, as :559 feeds it
      ["Q_target"]                 q_target.q_rows(next_grid, next_vec, goals, a', next_obs_self_t, next_obs_self_v, reward, done, gamma)
      ["Q", "probs"]               q_main.q_rows(grid, vec, goals, actions, obs_self_t, obs_self_v)["q"] and
                                   actor.probs_rows(obs_self_t, obs_self_v, obs_others, actions_prev, goals, epsilon)"""
    if env not in _ENVS:
        raise ValueError("baseline_train_step_feeds: env must be 'particle' or 'checkers', got %r" % (env,))
    if env == "checkers":
        return _baseline_train_step_feeds_checkers(cols, run, gamma, epsilon, IAC, use_Q, use_V, l_action, target_actor, actor, v_target,
                                                   v_main, q_target, q_main, draw, keep)
    _baseline_check_networks(cols, IAC, v_target, v_main, q_target, q_main, target_actor, actor)
    probs_kw = {} if keep is None else {"keep": keep}
    sample_kw = dict(probs_kw) if draw is None else dict(probs_kw, draw=draw)
    call = _Recorder(run)
    f64 = torch.float64
    v_global, v_global_next, goals = cols["v_global"], cols["v_global_next"], cols["goals"]
    n_steps, N = v_global.shape[0], v_global.shape[1]
    coma = N > 1 and bool(use_Q)
    if not use_V and not coma:
        raise ValueError("baseline_train_step_feeds: nothing to train the policy on (use_V = 0 and no COMA critic: use_Q = 0 or one agent)")
    rows = lambda x: x.reshape(n_steps * N, *x.shape[2:])                           # noqa: E731
    obs_others, v_local = rows(cols["obs_others"]), rows(cols["v_local"])
    obs_others_next, v_local_next = rows(cols["obs_others_next"]), rows(cols["v_local_next"])
    reward_local, reward_rep = cols["reward_local"].reshape(n_steps * N), rep_rows(cols["reward"], N)
    a1, ao = process_actions(cols["actions"], l_action)
    goals_self, goals_others = process_goals(goals)
    one, others, state = process_global_state(v_global)
    one_next, others_next, state_next = process_global_state(v_global_next)
    labels = torch.eye(N, dtype=f64, device=v_global.device).repeat(n_steps, 1)     # np.tile(np.eye(N), (n_steps, 1)) (:518)
    not_done = -(rep_rows(cols["done"], N).to(torch.int64) - 1)                     # if true, then 0, else 1 (:538, :580)

    def value_feed(nxt):
        if IAC:
            return {"obs_others": obs_others_next if nxt else obs_others, "v_obs": v_local_next if nxt else v_local, "v_goal": goals_self}
        return {"v_state_one_agent": one_next if nxt else one, "v_goal": goals_self,
                "v_state_other_agents": others_next if nxt else others, "v_goal_others": goals_others}

    v_res = v_td_policy = None
    if use_V:                       # ---- local critic (:522-558) ----
        if v_target is not None:
            call(["V_target", "V"], value_feed(True), launch=False)
            args = (cols["obs_others_next"], cols["v_local_next"], goals) if IAC else (v_global_next, goals)
            v_td = v_target.v_rows(*args, reward_local, cols["done"], gamma, **probs_kw)["td"]
            v_td_policy = v_main.v_rows(*args, reward_local, cols["done"], gamma, **probs_kw)["td"]      # (on V_next_res, :604)
        else:
            v_t, v_next = call(["V_target", "V"], value_feed(True))
            v_td = td_target(reward_local, v_t, not_done, gamma)
            v_td_policy = td_target(reward_local, v_next, not_done, gamma)
        v_res = call(["V_op", "V"], dict(value_feed(False), V_td_target=v_td))[1]
        if v_main is not None:
            v_main.repack()         # (the next evaluation reads the V_main weights this step updated)
        v_res = v_res.reshape(-1)

    if coma:                        # ---- global critic (:562-597) ----
        feed = {"obs_others": obs_others_next, "v_obs": v_local_next, "v_goal": goals_self, "epsilon": epsilon}
        if target_actor is None:
            acts = call(["action_samples_target"], feed)[0]
        else:
            call(["action_samples_target"], feed, launch=False)
            acts = target_actor.sample_rows(obs_others_next, v_local_next, goals_self, epsilon, **sample_kw)["actions"]
        if acts.is_cuda:
            a_next, a_others_next, _ = process_actions_device(acts, n_steps, N, l_action, keep=keep)
        else:
            a_next, a_others_next = process_actions(acts.reshape(n_steps, N), l_action)
        feed = {"v_state": state_next, "action_others": a_others_next, "v_goal": goals_self, "v_goal_others": goals_others,
                "v_labels": labels, "v_obs": v_local_next}
        if q_target is not None:
            call(["Q_target"], feed, launch=False)
            q_td = q_target.q_rows(v_global_next, goals, acts, cols["v_local_next"], cols["reward"], cols["done"], gamma, **probs_kw)["td"]
        else:
            q_t = call(["Q_target"], feed)[0]
            q_taken = (q_t.to(f64) * a_next).sum(dim=1)                             # np.sum(Q_target_res * actions_self_next, axis=1)
            q_td = td_target(reward_rep, q_taken, not_done, gamma)
        call(["Q_op"], {"Q_td_target": q_td, "actions_self_1hot": a1, "v_state": state, "action_others": ao, "v_goal": goals_self,
                        "v_goal_others": goals_others, "v_labels": labels, "v_obs": v_local})
        if q_main is not None:
            q_main.repack()         # (Q below reads the Q_main weights this step updated)
        # ---- Q(s, a, g) and pi(a | o, g) for the policy gradient (:606-616) ----
        feed = {"v_state": state, "v_obs": v_local, "action_others": ao, "obs_others": obs_others, "v_goal": goals_self,
                "v_goal_others": goals_others, "v_labels": labels, "epsilon": epsilon}
        if q_main is not None:
            call(["Q", "probs"], feed, launch=False)
            q_res = q_main.q_rows(v_global, goals, cols["actions"], cols["v_local"], **probs_kw)["q"]
            probs = actor.probs_rows(obs_others, v_local, goals_self, epsilon, **probs_kw)
        else:
            q_res, probs = call(["Q", "probs"], feed)

    # ---- policy (:618-653) ----
    feed = {"action_taken": a1, "epsilon": epsilon, "obs_others": obs_others, "v_obs": v_local, "v_goal": goals_self}
    if use_V:
        feed.update({"V_td_target": v_td_policy, "V_evaluated": v_res})
    if coma:
        feed.update({"v_goal_others": goals_others, "v_labels": labels, "Q_evaluated": q_res, "probs_evaluated": probs})
    call(["policy_op"], feed)
    call(["list_update_target_ops"], {})
    return call.calls


def _baseline_train_step_feeds_checkers(cols, run, gamma, epsilon, IAC, use_Q, use_V, l_action, target_actor, actor, v_target, v_main,
                                        q_target, q_main, draw, keep):
    """baseline_train_step_feeds(env="checkers"): alg_baseline_checkers.Alg.train_step (alg_baseline_checkers.py:499-662)."""
    _baseline_check_networks(cols, IAC, v_target, v_main, q_target, q_main, target_actor, actor, checkers=True)
    probs_kw = {} if keep is None else {"keep": keep}
    sample_kw = dict(probs_kw) if draw is None else dict(probs_kw, draw=draw)
    call = _Recorder(run)
    f64 = torch.float64
    vec, vec_next, goals = cols["vec"], cols["next_vec"], cols["goals"]
    n_steps, N = vec.shape[0], vec.shape[1]
    coma = N > 1 and bool(use_Q)
    if not use_V and not coma:
        raise ValueError("baseline_train_step_feeds: nothing to train the policy on (use_V = 0 and no COMA critic: use_Q = 0 or one agent)")
    # process_batch (:377-440): per-agent rows; grid, reward and done repeated N times; both action columns one-hot
    rows = lambda x: x.reshape(n_steps * N, *x.shape[2:])                           # noqa: E731
    obs = {nxt: {name: rows(cols[("next_%s" if nxt else "%s") % name]) for name in ("obs_others", "obs_self_t", "obs_self_v")}
           for nxt in (False, True)}
    state_env, state_env_next = rep_rows(cols["grid"], N), rep_rows(cols["next_grid"], N)
    reward_local, reward_rep = cols["local_rewards"].reshape(n_steps * N), rep_rows(cols["reward"], N)
    a1, ao = process_actions(cols["actions"], l_action)
    prev1 = torch.nn.functional.one_hot(cols["actions_prev"].long(), l_action).reshape(n_steps * N, l_action)
    goals_self, goals_others = process_goals(goals)
    one, others, state = process_global_state(vec)
    one_next, others_next, state_next = process_global_state(vec_next)
    labels = torch.eye(N, dtype=f64, device=vec.device).repeat(n_steps, 1)          # np.tile(self.agent_labels, (n_steps, 1)) (:510)
    not_done = -(rep_rows(cols["done"], N).to(torch.int64) - 1)                     # if true, then 0, else 1 (:531, :576)

    def value_feed(nxt):
        if IAC:
            return dict(obs[nxt], v_goal=goals_self)
        return {"state_env": state_env_next if nxt else state_env, "v_state_one_agent": one_next if nxt else one, "v_goal": goals_self,
                "v_state_other_agents": others_next if nxt else others}

    def base(nxt, *names):
        return tuple(cols[("next_%s" if nxt else "%s") % name] for name in names)

    v_res = v_td_policy = None
    if use_V:                       # ---- local critic (:514-552) ----
        if v_target is not None:
            call(["V_target", "V"], value_feed(True), launch=False)
            args = base(True, "obs_self_t", "obs_self_v", "obs_others") if IAC else base(True, "grid", "vec")
            v_td = v_target.v_rows(*args, goals, reward_local, cols["done"], gamma, **probs_kw)["td"]
            v_td_policy = v_main.v_rows(*args, goals, reward_local, cols["done"], gamma, **probs_kw)["td"]      # (on V_next_res, :602)
        else:
            v_t, v_next = call(["V_target", "V"], value_feed(True))
            v_td = td_target(reward_local, v_t, not_done, gamma)
            v_td_policy = td_target(reward_local, v_next, not_done, gamma)
        v_res = call(["V_op", "V"], dict(value_feed(False), V_td_target=v_td))[1]
        if v_main is not None:
            v_main.repack()         # (the next evaluation reads the V_main weights this step updated)
        v_res = v_res.reshape(-1)

    if coma:                        # ---- global critic (:556-595) ----
        # run_actor_target(actions_1hot, obs_others_next, ...): the action just taken is the previous action of the next step (:559)
        feed = dict(obs[True], v_goal=goals_self, actions_prev=a1, epsilon=epsilon)
        if target_actor is None:
            acts = call(["action_samples_target"], feed)[0]
        else:
            call(["action_samples_target"], feed, launch=False)
            acts = target_actor.sample_rows(obs[True]["obs_self_t"], obs[True]["obs_self_v"], obs[True]["obs_others"],
                                            cols["actions"].reshape(-1), goals_self, epsilon, **sample_kw)["actions"]
        if acts.is_cuda:
            a_next, a_others_next, _ = process_actions_device(acts, n_steps, N, l_action, keep=keep)
        else:
            a_next, a_others_next = process_actions(acts.reshape(n_steps, N), l_action)
        feed = {"state_env": state_env_next, "v_state": state_next, "action_others": a_others_next, "v_goal": goals_self,
                "v_goal_others": goals_others, "v_labels": labels, "obs_self_t": obs[True]["obs_self_t"],
                "obs_self_v": obs[True]["obs_self_v"]}
        if q_target is not None:
            call(["Q_target"], feed, launch=False)
            q_td = q_target.q_rows(*base(True, "grid", "vec"), goals, acts, *base(True, "obs_self_t", "obs_self_v"), cols["reward"],
                                   cols["done"], gamma, **probs_kw)["td"]
        else:
            q_t = call(["Q_target"], feed)[0]
            q_taken = (q_t.to(f64) * a_next).sum(dim=1)                             # np.sum(Q_target_res * actions_self_next, axis=1)
            q_td = td_target(reward_rep, q_taken, not_done, gamma)
        call(["Q_op"], {"Q_td_target": q_td, "actions_self_1hot": a1, "state_env": state_env, "v_state": state, "action_others": ao,
                        "v_goal": goals_self, "v_goal_others": goals_others, "v_labels": labels, "obs_self_t": obs[False]["obs_self_t"],
                        "obs_self_v": obs[False]["obs_self_v"]})
        if q_main is not None:
            q_main.repack()         # (Q below reads the Q_main weights this step updated)
        # ---- Q(s, a, g) and pi(a | o, g) for the policy gradient (:604-617) ----
        feed = dict(obs[False], state_env=state_env, v_state=state, actions_prev=prev1, action_others=ao, v_goal=goals_self,
                    v_goal_others=goals_others, v_labels=labels, epsilon=epsilon)
        if q_main is not None:
            call(["Q", "probs"], feed, launch=False)
            q_res = q_main.q_rows(*base(False, "grid", "vec"), goals, cols["actions"], *base(False, "obs_self_t", "obs_self_v"),
                                  **probs_kw)["q"]
            probs = actor.probs_rows(obs[False]["obs_self_t"], obs[False]["obs_self_v"], obs[False]["obs_others"],
                                     cols["actions_prev"].reshape(-1), goals_self, epsilon, **probs_kw)
        else:
            q_res, probs = call(["Q", "probs"], feed)

    # ---- policy (:619-660) ----
    feed = dict(obs[False], action_taken=a1, epsilon=epsilon, actions_prev=prev1, v_goal=goals_self)
    if use_V:
        feed.update({"V_td_target": v_td_policy, "V_evaluated": v_res})
    if coma:
        feed.update({"v_goal_others": goals_others, "v_labels": labels, "Q_evaluated": q_res, "probs_evaluated": probs})
    call(["policy_op"], feed)
    call(["list_update_target_ops"], {})
    return call.calls


# ---- QMIX (alg_qmix.py:236-380): everything of train_step that is not the mixer ----------------------------------------------

def process_batch_qmix(cols, l_action=5):
    """Columns of a sampled particle batch (sample_batch() / as_reference_batch(numpy=False)) -> the 13-tuple of
    alg_qmix.Alg.process_batch (alg_qmix.py:236-285): process_batch above with `done` and `goals` left per time step."""
    v_global = cols["v_global"]
    B, N = v_global.shape[0], v_global.shape[1]
    a1, ao = process_actions(cols["actions"], l_action)
    return (B, v_global, cols["obs_others"].reshape(B * N, -1), cols["v_local"].reshape(B * N, -1), a1, ao,
            rep_rows(cols["reward"], N), cols["reward_local"].reshape(B * N),
            cols["v_global_next"], cols["obs_others_next"].reshape(B * N, -1), cols["v_local_next"].reshape(B * N, -1),
            cols["done"], cols["goals"])


def _row_sum_numpy_order(x):
    """np.sum(x, axis=1) of a float64 [B, N]: left to right below 8 values, NumPy's eight-accumulator tree over the first 8 and then
    the rest one by one from 8 on (N <= 15: one block of the pairwise kernel)."""
    N = x.shape[1]
    if N > 15:
        raise ValueError("the row sum follows np.sum up to 15 values per row")
    c = [x[:, i] for i in range(N)]
    if N < 8:
        s, rest = c[0].clone(), c[1:]
    else:
        s, rest = ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7])), c[8:]
    for v in rest:
        s = s + v
    return s


def qmix_td_target(reward_local, q_tot, done, gamma):
    """np.sum(reward_local.reshape(B, N), axis=1) + gamma * np.squeeze(q_tot) * (-(done - 1)) (alg_qmix.py:367-369), float64 [B], in
    NumPy's order and types: the row sum in float64, gamma * q_tot in the type of q_tot (float32 from a session), then float64.  ONE
    launch of cm3_qmix_td_target_f64 for device tensors, the torch composition otherwise -- the same bits."""
    B, N = reward_local.shape
    q = q_tot.reshape(-1)
    if q.numel() != B or done.numel() != B:
        raise ValueError("qmix_td_target: %d transitions, %d values of q_tot, %d of done" % (B, q.numel(), done.numel()))
    if reward_local.is_cuda:
        from . import _lib
        if reward_local.dtype not in (torch.float32, torch.float64) or q.dtype not in (torch.float32, torch.float64):
            raise ValueError("qmix_td_target: reward_local and q_tot must be float32 or float64")
        r, q = reward_local.contiguous(), q.contiguous()
        d = done.reshape(-1).contiguous()
        d = d.view(torch.uint8) if d.dtype == torch.bool else (d != 0).view(torch.uint8)
        out = torch.empty(B, dtype=torch.float64, device=r.device)
        _lib.check(_lib.lib().cm3_qmix_td_target_f64(r.data_ptr(), 1 if r.dtype == torch.float64 else 0, N, q.data_ptr(),
                                                     1 if q.dtype == torch.float64 else 0, d.data_ptr(), float(gamma), out.data_ptr(), B,
                                                     torch.cuda.current_stream(r.device).cuda_stream))
        return out
    gq = q * torch.tensor(gamma, dtype=q.dtype)
    not_done = -(done.reshape(-1).to(torch.int64) - 1)                              # if true, then 0, else 1 (:367)
    return _row_sum_numpy_order(reward_local.to(torch.float64)) + gq.to(torch.float64) * not_done


def process_batch_qmix_checkers(cols, l_action=5):
    """Columns of a sampled Checkers batch (sample_batch() of either ring / CheckersRollout.as_reference_batch(numpy=False)) -> the
    18-tuple of alg_qmix_checkers.Alg.process_batch (alg_qmix_checkers.py:234-290; CHECKERS_BATCH_NAMES).  NOT process_batch_checkers,
    the CM3 learner's: here `reward` is repeated N times, state_env / state_env_next / done are left per time step, and state_agents
    stays [B, N, 4]."""
    vec = cols["vec"]
    B, N = vec.shape[0], vec.shape[1]
    rows = lambda x: x.reshape(B * N, *x.shape[2:])            # noqa: E731
    a1, ao = process_actions(cols["actions"], l_action)
    prev1 = torch.nn.functional.one_hot(cols["actions_prev"].long(), l_action).reshape(B * N, l_action)
    return (B, cols["grid"], vec, rows(cols["obs_others"]), rows(cols["obs_self_t"]), rows(cols["obs_self_v"]),
            prev1, a1, ao, rep_rows(cols["reward"], N), cols["local_rewards"].reshape(B * N), cols["next_grid"],
            cols["next_vec"], rows(cols["next_obs_others"]), rows(cols["next_obs_self_t"]),
            rows(cols["next_obs_self_v"]), cols["done"], cols["goals"])


def _onehot_rows(columns, l_action, device, keep=None):
    """The int64 one-hot rows [B * N, l_action] of each action column [B, N]: on the device all of them in ONE tiling launch (keep, if
    given, receives the flat int32 forms the launch reads), otherwise torch's one_hot."""
    A = int(l_action)
    if not device:
        return [torch.nn.functional.one_hot(c.long(), A).reshape(-1, A) for c in columns]
    from . import _lib
    t = _Tiler(columns[0].device)
    a32 = [c.reshape(-1).to(torch.int32).contiguous() for c in columns]
    _keep(keep, *a32)
    out = [t.add(a, a.numel(), A, torch.int64, _lib.TILE_ONEHOT_I64) for a in a32]
    t.run()
    return out


def _qmix_train_step_feeds_checkers(cols, run, gamma, target_agent, l_action, keep, target_mixer=None, mixer_q_agent=None, learner=None):
    """The Checkers form of qmix_train_step_feeds (alg_qmix_checkers.py:342-393)."""
    if learner is not None:
        # (before any column is read: the type; then what the learner needs beside it)
        from .qmix import CheckersQmixLearner
        if not isinstance(learner, CheckersQmixLearner):
            raise ValueError("qmix_train_step_feeds: env='checkers' takes a CheckersQmixLearner as learner, got %s: the Checkers learner is "
                             "not built from another network's weights; build a CheckersQmixLearner on the main CheckersQmixAgent and "
                             "CheckersQmixMixer, or call without learner and `run` answers mixer_op" % type(learner).__name__)
        if target_agent is None or target_mixer is None:
            raise ValueError("qmix_train_step_feeds: learner trains on the device TD target; pass target_agent and target_mixer (the "
                             "Agent_target / Mixer_target objects) as well")
        if learner.agent.n != cols["vec"].shape[1]:
            raise ValueError("qmix_train_step_feeds: learner is built for %d agents, the batch has %d"
                             % (learner.agent.n, cols["vec"].shape[1]))
    if target_mixer is not None:
        # (what needs no column comes first: the type, the target agent; then the batch's agent count and where its columns live)
        from .qmix import CheckersQmixMixer
        if not isinstance(target_mixer, CheckersQmixMixer):
            raise ValueError("qmix_train_step_feeds: env='checkers' takes a CheckersQmixMixer as target_mixer, got %s: the Checkers mixer is "
                             "not built from another network's weights; build a CheckersQmixMixer from the Mixer_target variables, or call "
                             "without target_mixer and `run` answers mixer_target" % type(target_mixer).__name__)
        if target_agent is None:
            raise ValueError("qmix_train_step_feeds: target_mixer reads the target agents' Q values on the device; pass target_agent "
                             "(a CheckersQmixAgent holding the Agent_target weights) as well")
        if target_mixer.n != cols["vec"].shape[1]:
            raise ValueError("qmix_train_step_feeds: target_mixer takes a CheckersQmixMixer for %d agents (the batch's count), got one for "
                             "%d agents" % (cols["vec"].shape[1], target_mixer.n))
        if not cols["vec"].is_cuda:
            raise ValueError("qmix_train_step_feeds: target_mixer evaluates device columns; call without it for host tensors")
    if mixer_q_agent is not None:
        if target_mixer is None:
            raise ValueError("qmix_train_step_feeds: mixer_q_agent names the agent whose Q values enter the device target mixer; pass "
                             "target_mixer as well, or leave it out and `run` answers mixer_target")
        if type(mixer_q_agent) is not type(target_agent) or mixer_q_agent.n != target_agent.n:
            raise ValueError("qmix_train_step_feeds: mixer_q_agent must be a %s for %d agents like target_agent (the main agent), got %s"
                             % (type(target_agent).__name__, target_agent.n, type(mixer_q_agent).__name__))
    call = _Recorder(run)
    vec = cols["vec"]
    B, N = vec.shape[0], vec.shape[1]
    device = target_agent is not None
    if device and not vec.is_cuda:
        raise ValueError("qmix_train_step_feeds: target_agent evaluates device columns; call without it for host tensors")
    rows = lambda x: x.reshape(B * N, *x.shape[2:])            # noqa: E731
    obs_others, obs_self_t, obs_self_v = rows(cols["obs_others"]), rows(cols["obs_self_t"]), rows(cols["obs_self_v"])
    obs_others_next, obs_self_t_next, obs_self_v_next = (rows(cols["next_obs_others"]), rows(cols["next_obs_self_t"]),
                                                         rows(cols["next_obs_self_v"]))
    goals = cols["goals"]
    goals_all, goals_self = goals.reshape(B, -1), rows(goals)                       # :348-349
    state_agents_next, state_agents = cols["next_vec"].reshape(B, -1), vec.reshape(B, -1)   # :350-351
    actions_1hot, actions_prev_1hot = _onehot_rows((cols["actions"], cols["actions_prev"]), l_action, device, keep)

    # ---- argmax actions of the target agents, one-hot (:353-362).  The reference feeds actions_prev : actions_1hot here and in the
    # mixer_target feed -- the action JUST TAKEN, next to the next_* observations -- not the actions_prev column ----
    agent_next = {"actions_prev": actions_1hot, "obs_others": obs_others_next, "obs_self_t": obs_self_t_next,
                  "obs_self_v": obs_self_v_next, "v_goal": goals_self}
    if device:
        call(["argmax_Q_target"], dict(agent_next), launch=False)
        greedy = target_agent.greedy_rows(obs_self_t_next, obs_self_v_next, obs_others_next, cols["actions"].reshape(B * N), goals_self,
                                          onehot=True, q_max=target_mixer is not None)
        target_1hot = greedy["onehot"]
    else:
        argmax = call(["argmax_Q_target"], dict(agent_next))[0]
        target_1hot = torch.nn.functional.one_hot(argmax.reshape(-1).long(), int(l_action))
    # ---- Q_tot of the target mixer, TD target (:364-379; the arithmetic of the particle train_step) ----
    feed = {"state_env": cols["next_grid"], "v_state": state_agents_next, "v_goal_all": goals_all, "actions_1hot": target_1hot}
    feed.update(agent_next)
    if target_mixer is not None:
        # agent_qs of the target evaluation is reduce_sum(Q_target * actions_1hot) (alg_qmix_checkers.py:93-95): the Q at the argmax
        call(["mixer_target"], feed, launch=False)
        agent_qs = greedy["q_max"]
        if mixer_q_agent is not None:
            # the reference's Checkers graph builds mixer_target on mixer_q_input (alg_qmix_checkers.py:96-97, :106): the Q values of
            # Agent_MAIN on this feed, selected by the fed one-hot actions -- the target agents' argmax
            q_main = mixer_q_agent.greedy_rows(obs_self_t_next, obs_self_v_next, obs_others_next, cols["actions"].reshape(B * N),
                                               goals_self, q=True, onehot=False)["q"]
            agent_qs = q_main.gather(1, greedy["argmax"].long().unsqueeze(1))
        target = target_mixer.q_tot(cols["next_grid"], cols["next_vec"], goals, agent_qs.reshape(B, N),
                                    cols["local_rewards"].reshape(B, N), cols["done"], gamma)["td"]
    else:
        q_tot = call(["mixer_target"], feed)[0]
        target = qmix_td_target(cols["local_rewards"].reshape(B, N), q_tot, cols["done"], gamma)
    # ---- optimiser step of the main mixer, soft update (:381-393) ----
    call(["mixer_op"], {"state_env": cols["grid"], "v_state": state_agents, "v_goal_all": goals_all, "actions_1hot": actions_1hot,
                        "actions_prev": actions_prev_1hot, "obs_others": obs_others, "obs_self_t": obs_self_t,
                        "obs_self_v": obs_self_v, "v_goal": goals_self, "td_target": target}, launch=learner is None)
    if learner is not None:
        learner.step(cols, target, keep=keep)
    call(["list_update_target_ops"], {})
    return call.calls


def qmix_train_step_feeds(cols, run, gamma, target_agent=None, l_action=5, env="particle", target_mixer=None, keep=None,
                          mixer_q_agent=None, learner=None):
    """The data side of the QMIX train_step (alg_qmix.py:338-380) from the columns of a sampled particle batch: builds, in the
    reference's order, the feed_dict of its four sess.run calls -- ["argmax_Q_target"], ["mixer_target"], ["mixer_op"],
    ["list_update_target_ops"] -- and returns the list of (ops, feed).  ``run(ops, feed)`` plays sess.run as in train_step_feeds: ops
    and placeholders are the reference's attribute names (v_state, v_goal_all, actions_1hot, obs_others, v_obs, v_goal, td_target);
    it returns one tensor per op (None for mixer_op and list_update_target_ops).  The main mixer's loss, gradient and optimiser step
    are `run`'s, and without target_mixer the target mixer's forward pass as well.

    Without target_agent everything is the torch composition -- the specification, pinned bit for bit to the arrays the REAL
    train_step fed (tests/golden/trainstep_qmix_particle_n*.npz); it runs on CPU tensors and calls `run` for the argmax.
    With target_agent (a ParticleQmixAgent holding the Agent_target weights) and CUDA columns, `run` is NOT called for
    argmax_Q_target (its (ops, feed) entry still appears in the list): the one-hot target actions come from
    target_agent.greedy_rows in one launch, actions_1hot from one tiling launch, the TD target from cm3_qmix_td_target_f64.
    The soft update of the agent's target weights -- the agent half of list_update_target_ops -- is left to the caller:
    ``target_agent.soft_update_from(main_agent, tau)`` after this function returns.
    With target_mixer as well (a ParticleQmixMixer holding the Mixer_target weights), `run` is NOT called for
    mixer_target either (its (ops, feed) entry still appears, in the same place with the same keys): greedy_rows runs once with
    q_max, and ONE launch of target_mixer.q_tot on v_global_next, goals and those Q values gives mixer_op's td_target, so `run` is
    left with what needs a gradient or an optimiser.  The caller's contract: `run` trains the main mixer (mixer_op) and writes the
    trained variables into its ParticleQmixMixer in place; after this function returns the caller does
    ``target_mixer.soft_update_from(main_mixer, tau)`` next to ``target_agent.soft_update_from(main_agent, tau)`` -- the two halves of
    list_update_target_ops.  Refused with a ValueError that names the remedy: target_mixer without target_agent, host columns, a
    mixer for another agent count, an object that is no ParticleQmixMixer (a CheckersQmixMixer included).  Without target_mixer
    nothing changes.

    env="checkers": the same four calls of alg_qmix_checkers.train_step (alg_qmix_checkers.py:342-393) from the columns of a sampled
    Checkers batch; placeholders state_env, v_state, v_goal_all, actions_1hot, actions_prev, obs_others, obs_self_t, obs_self_v,
    v_goal, td_target.  In the two TARGET feeds actions_prev is fed actions_1hot (the action just taken, as the reference does),
    in mixer_op the one-hot actions_prev column.  target_agent: a CheckersQmixAgent holding the Agent_target weights; both one-hot
    action feeds come from one tiling launch.  Pinned to tests/golden/trainstep_qmix_checkers_n*.npz.
    target_mixer: a CheckersQmixMixer holding the Mixer_target weights, under the same contract as the particle one -- greedy_rows
    runs once with q_max, the ["mixer_target"] entry is recorded in its place with its keys but `run` is not called for it, and ONE
    launch of target_mixer.q_tot on next_grid, next_vec, goals, those Q values, local_rewards and done gives mixer_op's td_target;
    the caller does ``target_mixer.soft_update_from(main_mixer, tau)`` next to the agent's afterwards.  Refused with a ValueError that
    names the remedy, before a column is read: an object that is no CheckersQmixMixer (a ParticleQmixMixer included), target_mixer
    without target_agent; then a mixer for another agent count than the batch's, host columns.
    mixer_q_agent (with target_mixer only): WHOSE Q values enter the target mixer.  Default None: the target agents' Q at their argmax
    (q_max of the one greedy_rows launch), the wiring of the particle graph (alg_qmix.py:107, :113) and of QMIX as published.  The
    reference's CHECKERS graph is wired differently: alg_qmix_checkers.py:106 builds mixer_target on mixer_q_input (:96-97), the Q
    values of Agent_MAIN on the fed next observations, selected by the fed one-hot actions (the target agents' argmax).  Pass the main
    CheckersQmixAgent as mixer_q_agent to evaluate exactly that: one more greedy_rows launch on the main agent, its Q gathered at the
    target's argmax.  A `run` that plays the reference's session computes the same inside sess.run(mixer_target).

    learner: a cm3_amd.qmix.ParticleQmixLearner (env="checkers": a CheckersQmixLearner) on the main agent and mixer.  The ["mixer_op"] entry is still recorded
    in its place with its keys, but `run` is NOT called for it: ``learner.step(cols, td_target)`` computes loss and gradients and
    applies Adam to the main networks on the device, so `run` is left with list_update_target_ops alone (the caller's two
    soft_update_from calls, as above; ParticleQmixLearner.train_step does the whole step with no `run`).  It needs target_agent and
    target_mixer (the TD target must be on the device) and a learner whose agent count is the batch's; env="checkers" refuses
    anything but a CheckersQmixLearner, before a column is read (the Checkers learner is not built from another network's weights;
    CheckersQmixLearner.train_step is this function with mixer_q_agent=learner.agent).  Without learner nothing changes.

    keep: an optional list that receives the int32 action temporaries the one-hot tiling launch reads -- whoever captures this
    function's launches into a hipGraph holds them for as long as the graph is replayed."""
    if env == "checkers":
        return _qmix_train_step_feeds_checkers(cols, run, gamma, target_agent, l_action, keep, target_mixer, mixer_q_agent, learner)
    if env != "particle":
        raise ValueError("qmix_train_step_feeds: env must be 'particle' or 'checkers', got %r" % (env,))
    if mixer_q_agent is not None:
        raise ValueError("qmix_train_step_feeds: mixer_q_agent belongs to env='checkers'; the particle graph builds mixer_target on the "
                         "target agents' Q values (alg_qmix.py:113), leave it out")
    if learner is not None:
        if target_agent is None or target_mixer is None:
            raise ValueError("qmix_train_step_feeds: learner trains on the device TD target; pass target_agent and target_mixer (the "
                             "Agent_target / Mixer_target objects) as well")
        if learner.agent.n != cols["v_global"].shape[1]:
            raise ValueError("qmix_train_step_feeds: learner is built for %d agents, the batch has %d"
                             % (learner.agent.n, cols["v_global"].shape[1]))
    if target_mixer is not None:
        from .qmix import ParticleQmixMixer
        n_batch = cols["v_global"].shape[1]
        if not isinstance(target_mixer, ParticleQmixMixer) or target_mixer.n != n_batch:
            raise ValueError("qmix_train_step_feeds: target_mixer takes a ParticleQmixMixer for %d agents (the batch's count), got %s"
                             % (n_batch, "one for %d agents" % target_mixer.n if isinstance(target_mixer, ParticleQmixMixer)
                                else type(target_mixer).__name__))
        if target_agent is None:
            raise ValueError("qmix_train_step_feeds: target_mixer reads the target agents' Q values on the device; pass target_agent "
                             "(a ParticleQmixAgent holding the Agent_target weights) as well")
        if not cols["v_global"].is_cuda:
            raise ValueError("qmix_train_step_feeds: target_mixer evaluates device columns; call without it for host tensors")
    call = _Recorder(run)
    vg = cols["v_global"]
    B, N = vg.shape[0], vg.shape[1]
    device = target_agent is not None
    if device and not vg.is_cuda:
        raise ValueError("qmix_train_step_feeds: target_agent evaluates device columns; call without it for host tensors")
    rows = lambda x: x.reshape(B * N, -1)                                           # noqa: E731
    obs_others, v_local = rows(cols["obs_others"]), rows(cols["v_local"])
    obs_others_next, v_local_next = rows(cols["obs_others_next"]), rows(cols["v_local_next"])
    goals = cols["goals"]
    goals_all, goals_self = goals.reshape(B, -1), rows(goals)                       # :344-345
    state_next, state = cols["v_global_next"].reshape(B, -1), vg.reshape(B, -1)     # :346-347
    actions_1hot, = _onehot_rows((cols["actions"],), l_action, device, keep)

    # ---- argmax actions of the target agents, one-hot (:349-356) ----
    feed = {"obs_others": obs_others_next, "v_obs": v_local_next, "v_goal": goals_self}
    if device:
        call(["argmax_Q_target"], feed, launch=False)
        greedy = target_agent.greedy_rows(obs_others_next, v_local_next, goals_self, onehot=True, q_max=target_mixer is not None)
        target_1hot = greedy["onehot"]
    else:
        argmax = call(["argmax_Q_target"], feed)[0]
        target_1hot = torch.nn.functional.one_hot(argmax.reshape(-1).long(), int(l_action))
    # ---- Q_tot of the target mixer, TD target (:358-369) ----
    feed = {"v_state": state_next, "v_goal_all": goals_all, "actions_1hot": target_1hot, "obs_others": obs_others_next,
            "v_obs": v_local_next, "v_goal": goals_self}
    if target_mixer is not None:
        # agent_qs of the target evaluation is reduce_sum(Q_target * actions_1hot) (alg_qmix.py:101-103): the Q at the argmax
        call(["mixer_target"], feed, launch=False)
        target = target_mixer.q_tot(cols["v_global_next"], goals, greedy["q_max"].reshape(B, N), cols["reward_local"].reshape(B, N),
                                    cols["done"], gamma)["td"]
    else:
        q_tot = call(["mixer_target"], feed)[0]
        target = qmix_td_target(cols["reward_local"].reshape(B, N), q_tot, cols["done"], gamma)
    # ---- optimiser step of the main mixer, soft update (:371-380) ----
    call(["mixer_op"], {"v_state": state, "v_goal_all": goals_all, "actions_1hot": actions_1hot, "obs_others": obs_others,
                        "v_obs": v_local, "v_goal": goals_self, "td_target": target}, launch=learner is None)
    if learner is not None:
        learner.step(cols, target, keep=keep)
    call(["list_update_target_ops"], {})
    return call.calls
