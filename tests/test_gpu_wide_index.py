"""GPU: the 64-bit index builds of the data-movement kernels of csrc/batch.hip, and addressing beyond 4 GiB.

Five kernels exist in two index widths (csrc/rows_index_width.h has the rules, tests/test_rows_index_width.py pins them): k_rows_copy,
k_rows_tile, k_ck_transitions_gather, k_ck_transitions_pack and -- decided inside the kernel -- k_transitions_gather.  The wide builds
run by rule only near 2^32 units; cm3_rows_force_index_width(64) runs them at any size.  Every case here runs its operation twice, under
the rule and forced wide, and asserts
  * cm3_rows_last_index_width() is 32, then 64,
  * the forced output equals, bit for bit, a plain restatement of the operation on the host (NumPy / CPU torch indexing, repeat,
    one_hot and casts in int64 / float64; the particle export against as_reference_batch_torch),
  * the two outputs equal each other.
The kernels move bytes and make exact int -> float64 casts: every comparison is exact, most of them on the raw bytes.  Shapes are the
smallest at which the index code can still go wrong: several workgroups per column (blockIdx-derived offsets are non-zero), a ragged
last workgroup, rings that wrap, odd record strides.

What this does NOT prove: the forced runs execute the wide code at small values only.  Truncation at real sizes is covered for
k_rows_copy's addressing alone (the last test: one 4 GiB + 1 MiB column, narrow unit arithmetic with size_t addressing).  A Checkers
ring with a column above 4 GiB is deliberately not tested: all 16 columns would have to be allocated at that row count, 13 GB or more.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _both(run):
    """run() under the rule and forced wide -> (rule output, forced output); the widths the launchers report are asserted"""
    from cm3_amd import _lib
    assert _lib.lib().cm3_rows_force_index_width(0) == 0
    a = run()
    wa = _lib.rows_last_index_width()
    with _lib.force_rows_index_width(64):
        b = run()
        wb = _lib.rows_last_index_width()
    torch.cuda.synchronize()
    assert (wa, wb) == (32, 64)
    return a, b


def _u8(t):
    """the bytes of a tensor as uint8 [rows, row bytes] on the host"""
    t = t.contiguous()
    return t.view(torch.uint8).reshape(t.shape[0], -1).cpu().numpy()


def _np_u8(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    return a.reshape(a.shape[0], -1).view(np.uint8)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _dev(a):
    return torch.as_tensor(a, device=DEV)


# ---- cm3_rows_scatter / cm3_rows_gather ------------------------------------------------------------------------------------------
ROW_BYTES = (48, 24, 12, 7)        # -> 16-, 8-, 4- and 1-byte units


@pytest.mark.parametrize("mode", ["dst_row", "gather", "ring"])
def test_rows_copy_wide_build(mode):
    from cm3_amd import _lib
    rng = np.random.default_rng(31)
    n_src, n_dst = 1500, 1700
    src = [rng.integers(0, 256, (n_src, rb), dtype=np.uint8) for rb in ROW_BYTES]
    init = [rng.integers(0, 256, (n_dst, rb), dtype=np.uint8) for rb in ROW_BYTES]
    d_src = [_dev(s) for s in src]
    units = []
    for s, rb in zip(d_src, ROW_BYTES):      # (the unit the launcher takes: what divides the row size and both base addresses)
        a = s.data_ptr() | rb
        units.append(16 if a % 16 == 0 else 8 if a % 8 == 0 else 4 if a % 4 == 0 else 1)
    assert units == [16, 8, 4, 1]            # (destinations below are fresh allocations, aligned like the sources)
    if mode == "dst_row":
        dst_row = rng.permutation(n_dst)[:n_src].astype(np.int64)
        dst_row[rng.permutation(n_src)[:n_src // 3]] = -1
        want = [w.copy() for w in init]
        for w, s in zip(want, src):
            w[dst_row[dst_row >= 0]] = s[dst_row >= 0]
        d_row = _dev(dst_row)
        n_out = n_dst
    elif mode == "gather":
        idx = rng.integers(0, n_src, n_dst)
        idx[:50] = idx[50]                   # repeated indices
        want = [s[idx] for s in src]
        d_row = _dev(idx.astype(np.int64))
        n_out = n_dst
    else:
        start = n_dst - 40                   # wraps 40 rows in
        pos = (start + np.arange(n_src)) % n_dst
        want = [w.copy() for w in init]
        for w, s in zip(want, src):
            w[pos] = s
        n_out = n_dst

    def run():
        dst = [_dev(w) for w in init]
        assert all((d.data_ptr() | rb) % u == 0 for d, rb, u in zip(dst, ROW_BYTES, units))
        pairs = list(zip(dst, d_src))
        if mode == "dst_row":
            _lib.rows_scatter(pairs, n_src, _stream(), dst_row=d_row)
        elif mode == "gather":
            _lib.rows_gather(pairs, n_dst, d_row, _stream())
        else:
            _lib.rows_scatter(pairs, n_src, _stream(), ring_start=start, ring_size=n_dst)
        return dst
    rule, forced = _both(run)
    for k, rb in enumerate(ROW_BYTES):
        assert forced[k].shape == (n_out, rb)
        assert np.array_equal(forced[k].cpu().numpy(), want[k]), (mode, rb)
        assert torch.equal(rule[k], forced[k]), (mode, rb)


# ---- cm3_rows_tile -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 3, 8])
def test_rows_tile_wide_build(N):
    """every CM3_TILE_* kind in one launch (the column set of test_row_kernels_against_torch_indexing_on_random_layouts, both `others`
    forms and EYE) plus COPY columns of 1-, 4- and 8-byte elements"""
    from cm3_amd import _lib
    from cm3_amd.batch import _Tiler
    g = torch.Generator(device="cpu").manual_seed(50 + N)
    B, A = 37, 5
    R = B * N
    x = torch.randn(B, N, 4, generator=g)
    x8 = torch.randint(-2 ** 62, 2 ** 62, (B, N, 3), generator=g, dtype=torch.int64)
    x1 = torch.randint(0, 256, (B, N, 7), generator=g, dtype=torch.int64).to(torch.uint8)
    acts = torch.randint(0, A, (B, N), generator=g).to(torch.int32)
    done = torch.rand(B, generator=g) < 0.3
    dx, dx8, dx1, dacts, ddone = (t.to(DEV) for t in (x, x8, x1, acts, done))
    rep = ((N * N, 0, N), (1, N, 1))

    def run():
        t = _Tiler(torch.device(DEV))
        out = dict(
            rep_n=t.add(dx, R * N, 4, dx.dtype, _lib.TILE_COPY, terms=rep),
            rep_n8=t.add(dx8, R * N, 3, dx8.dtype, _lib.TILE_COPY, terms=rep),
            rep_n1=t.add(dx1, R * N, 7, dx1.dtype, _lib.TILE_COPY, terms=rep),
            rep_m_a=t.add(dx, R * N * A, 4, torch.float64, _lib.TILE_F32_TO_F64, terms=((A * N, 0, 1), (1, 0, 0))),
            oh=t.add(dacts, R, A, torch.int64, _lib.TILE_ONEHOT_I64),
            oth=t.add(dx, R * (N - 1), 4, torch.float64, _lib.TILE_F32_TO_F64, others=(N, N * (N - 1), N - 1), shape=(R, (N - 1) * 4)),
            oth_oh=t.add(dacts, R * (N - 1), A, torch.float64, _lib.TILE_ONEHOT_F64, others=(N, N * (N - 1), N - 1), shape=(R, N - 1, A)),
            eye=t.add(None, R * A, A, torch.float64, _lib.TILE_EYE_F64),
            nd=t.add(ddone.view(torch.uint8), R, 1, torch.int64, _lib.TILE_NOT_I64, terms=((N, 0, 1), (1, 0, 0)), shape=(R,)))
        t.run()
        return out
    rule, forced = _both(run)
    idx = torch.tensor([[j for j in range(N) if j != n] for n in range(N)])
    onehot = torch.nn.functional.one_hot(acts.long(), A)
    want = dict(
        rep_n=x.repeat_interleave(N, dim=0).reshape(-1, 4),
        rep_n8=x8.repeat_interleave(N, dim=0).reshape(-1, 3),
        rep_n1=x1.repeat_interleave(N, dim=0).reshape(-1, 7),
        rep_m_a=x.reshape(R, 4).repeat_interleave(N, dim=0).repeat_interleave(A, dim=0).to(torch.float64),
        oh=onehot.reshape(R, A),
        oth=x[:, idx].reshape(R, (N - 1) * 4).to(torch.float64),
        oth_oh=onehot[:, idx].reshape(R, N - 1, A).to(torch.float64),
        eye=torch.eye(A, dtype=torch.float64).repeat(R, 1),
        nd=1 - done.repeat_interleave(N).to(torch.int64))
    assert R * N * A * 4 > 4 * 256 and (R * A * A) % 256 != 0              # several workgroups; columns that end inside one
    for k, w in want.items():
        assert forced[k].dtype == w.dtype and tuple(forced[k].shape) == tuple(w.shape), k
        assert torch.equal(forced[k].cpu(), w), (N, k)
        assert torch.equal(rule[k], forced[k]), (N, k)


# ---- the Checkers export, pack and expand: synthetic trajectories through the C ABI ------------------------------------------------
CK_T, CK_E, CK_R, CK_C, CK_O = 9, 37, 3, 8, 2
CK_K = 2 * CK_O + 1
CK_GRID_REC = CK_R * (CK_C + 1) * 2                      # 54 bytes
# name -> (agents, grid stride, obs_self_t stride): N = 1 the 8-byte unit rows of 75 doubles; N = 2 padded (strides rounded up to 4) and
# unpadded; N = 3 odd 225-byte records and an odd grid stride, so that no int8 record pair can be read two bytes at a time (pair16 = 0)
CK_CASES = {"n1": (1, 54, 75), "n2_padded": (2, 56, 152), "n2": (2, 54, 150), "n3_odd": (3, 55, 225)}


class _CkTraj(object):
    """A synthetic Checkers trajectory with terminal capture on the device (full-range int8 / int32 values: a misplaced byte shows),
    its descriptor structs, and the host arrays the restatement indexes."""

    def __init__(self, case):
        from cm3_amd import _lib
        N, gs, os_ = CK_CASES[case]
        T, E = CK_T, CK_E
        self.N, self.gs, self.os = N, gs, os_
        self.Lo = 2 * max(N - 1, 1)
        self.obst_rec = N * CK_K * CK_K * 3
        rng = np.random.default_rng(1000 + N + gs)
        h = dict(
            grid=rng.integers(-128, 128, (T + 1, E, gs), dtype=np.int8), term_grid=rng.integers(-128, 128, (T, E, gs), dtype=np.int8),
            obs_self_t=rng.integers(-128, 128, (T + 1, E, os_), dtype=np.int8),
            term_obs_self_t=rng.integers(-128, 128, (T, E, os_), dtype=np.int8),
            vec=rng.integers(-2 ** 31, 2 ** 31, (T + 1, E, N, 4)).astype(np.int32),
            term_vec=rng.integers(-2 ** 31, 2 ** 31, (T, E, N, 4)).astype(np.int32),
            obs_others=rng.standard_normal((T + 1, E, N, self.Lo)), term_obs_others=rng.standard_normal((T, E, N, self.Lo)),
            obs_self_v=rng.standard_normal((T + 1, E, N, 4)), term_obs_self_v=rng.standard_normal((T, E, N, 4)),
            actions=rng.integers(0, 5, (T, E, N)).astype(np.int32), local_rewards=rng.standard_normal((T, E, N)),
            reward=rng.standard_normal((T, E)), done=(rng.random((T, E)) < 0.25).astype(np.uint8) * rng.integers(1, 256, (T, E), dtype=np.uint8),
            goal_slots=rng.integers(0, 2, (T + 1, E, N)).astype(np.uint8), prev0=rng.integers(0, 5, (E, N)).astype(np.int32))
        h["done"][0, :3], h["done"][T - 1, -3:] = 1, 7        # tick 0 and the last tick among the done bytes
        assert 0.1 < (h["done"] != 0).mean() < 0.45
        self.h = h
        self.d = {k: _dev(v) for k, v in h.items()}
        desc = _lib.CheckersDesc()
        desc.n_envs, desc.n_agents, desc.n_rows, desc.n_columns, desc.n_obs, desc.max_steps = E, N, CK_R, CK_C, CK_O, 33
        desc.grid_stride, desc.obs_self_t_stride = gs, os_
        tr = _lib.CheckersTraj()
        for name in ("actions", "grid", "vec", "obs_others", "obs_self_t", "obs_self_v", "local_rewards", "reward", "done"):
            x = self.d[name]
            setattr(tr, name, x.data_ptr())
            setattr(tr, name + ("_slot_stride" if name in ("grid", "obs_self_t") else "_stride"), x[0].numel() * x.element_size())
        for name in ("grid", "vec", "obs_others", "obs_self_t", "obs_self_v"):
            x = self.d["term_" + name]
            setattr(tr, "term_" + name, x.data_ptr())
            setattr(tr, "term_" + name + ("_slot_stride" if name in ("grid", "obs_self_t") else "_stride"), x[0].numel() * x.element_size())
        tr.goals_slots, tr.goals_slots_stride = self.d["goal_slots"].data_ptr(), E * N
        self.desc, self.traj = desc, tr

    def columns(self, tt, ee, wide):
        """The 16 columns of transitions (tt, ee) on the host: the reference's float64 / int32 / bool / int64 columns (wide), or the
        compact ring's, which keep the trajectory's dtypes and the goal byte."""
        h, N, B = self.h, self.N, len(tt)
        done = h["done"][tt, ee] != 0
        f = (lambda a: a.astype(np.float64)) if wide else (lambda a: a)

        def now(name):
            return h[name][tt, ee]

        def nxt(name):
            a, t = h[name][tt + 1, ee], h["term_" + name][tt, ee]
            return np.where(done.reshape((B,) + (1,) * (a.ndim - 1)), t, a)

        def shaped(get):
            return dict(grid=f(get("grid")[:, :CK_GRID_REC]).reshape(B, CK_R, CK_C + 1, 2), vec=f(get("vec")),
                        obs_others=get("obs_others"), obs_self_t=f(get("obs_self_t")[:, :self.obst_rec]).reshape(B, N, CK_K, CK_K, 3),
                        obs_self_v=get("obs_self_v"))
        cols = shaped(now)
        cols.update({"next_" + k: v for k, v in shaped(nxt).items()})
        before = np.maximum(tt - 1, 0)
        prev = np.where((tt > 0)[:, None], h["actions"][before, ee], h["prev0"][ee])
        prev = np.where(((tt > 0) & (h["done"][before, ee] != 0))[:, None], 0, prev).astype(np.int32)    # zeros behind a done
        goal = h["goal_slots"][tt, ee]
        cols.update(actions_prev=prev, actions=now("actions"), reward=now("reward"), local_rewards=now("local_rewards"), done=done,
                    goals=np.stack([goal == 0, goal == 1], -1).astype(np.int64) if wide else goal)
        return cols


def _ck_row_bytes(tj, wide):
    """name -> bytes per row of the wide (reference) or compact columns, from the geometry"""
    from cm3_amd import _lib
    N = tj.N
    rec = dict(grid=CK_GRID_REC, vec=4 * N * 4, obs_others=8 * N * tj.Lo, obs_self_t=tj.obst_rec, obs_self_v=8 * N * 4, actions=4 * N,
               reward=8, local_rewards=8 * N, done=1, goals=N)
    widen = dict(grid=8, obs_self_t=8, vec=2, goals=16) if wide else {}
    return {name: rec[record] * widen.get(record, 1) for name, record in _lib.CHECKERS_COLUMN_RECORDS}


def _ck_alloc(init):
    return {k: _dev(v) for k, v in init.items()}


def _ck_assert(forced, rule, want, what):
    for name, w in want.items():
        assert np.array_equal(_u8(forced[name]), w), (what, name)
        assert torch.equal(rule[name], forced[name]), (what, name)


@pytest.mark.parametrize("case", sorted(CK_CASES))
def test_checkers_transitions_gather_wide_build(case):
    from cm3_amd import _lib
    tj = _CkTraj(case)
    T, E = CK_T, CK_E
    rng = np.random.default_rng(7)
    rb = _ck_row_bytes(tj, True)
    pick_t, pick_e = rng.integers(0, T, 200), rng.integers(0, E, 200)
    pick_t[:20], pick_t[20:40] = 0, T - 1
    pick_t[40:50], pick_e[40:50] = pick_t[0], pick_e[0]      # repeats
    whole = np.arange(T * E)
    for what, tt, ee, indexed in (("whole", whole // E, whole % E, False), ("indexed", pick_t, pick_e, True)):
        n = len(tt)
        cols = {k: _np_u8(v) for k, v in tj.columns(tt, ee, True).items()}
        assert {k: v.shape[1] for k, v in cols.items()} == rb
        d_tt, d_ee = (_dev(tt.astype(np.int64)), _dev(ee.astype(np.int64))) if indexed else (None, None)
        for ring in (False, True):
            rows = n + 11 if ring else n
            start = rows - 7 if ring else 0                  # the chunk wraps 7 rows in
            init = {k: rng.integers(0, 256, (rows, b), dtype=np.uint8) for k, b in rb.items()}
            want = {k: v.copy() for k, v in init.items()}
            for k in want:
                want[k][(start + np.arange(n)) % rows] = cols[k]

            def run():
                out = _ck_alloc(init)
                st = _lib.fill_checkers_cols(_lib.CheckersTransitionCols(), out, start, rows if ring else 0)
                _lib.check(_lib.lib().cm3_checkers_transitions_gather(ctypes.byref(tj.desc), ctypes.byref(tj.traj), tj.d["prev0"].data_ptr(),
                                                                      _lib.ptr(d_tt), _lib.ptr(d_ee), n, ctypes.byref(st), _stream()))
                return out
            rule, forced = _both(run)
            _ck_assert(forced, rule, want, (case, what, ring))


def _granule(tj, name, record, rb):
    """The granule cm3_checkers_transitions_pack takes for a column: the largest power of two <= 16 that divides the ring row, every
    source stride and every source base address -- from the column's spec as this test built it."""
    d = tj.d
    src = {"grid": ("grid", tj.gs), "obs_self_t": ("obs_self_t", tj.os), "done": ("done", 1), "goals": ("goal_slots", tj.N)}.get(record, (record, None))
    x = d[src[0]]
    env_stride = src[1] if src[1] is not None else x[0, 0].numel() * x.element_size()
    a = x.data_ptr() | (x[0].numel() * x.element_size()) | env_stride | rb
    if name.startswith("next_"):
        t = d["term_" + record]
        a |= t.data_ptr() | (t[0].numel() * t.element_size())
    if name == "actions_prev":
        a |= d["prev0"].data_ptr()
    return next(g for g in (16, 8, 4, 2, 1) if a % g == 0)


def test_checkers_pack_case_set_covers_every_granule_and_both_row_widths():
    """asserted from the column specs, not from the kernel: granules 16 / 8 / 4 / 2 / 1, rows of >= 16 bytes (pk_wide) and narrower ones
    (pk_narrow) all occur among the cases of the next test"""
    from cm3_amd import _lib
    seen = set()
    for case in CK_CASES:
        tj = _CkTraj(case)
        rb = _ck_row_bytes(tj, False)
        for name, record in _lib.CHECKERS_COLUMN_RECORDS:
            seen.add((_granule(tj, name, record, rb[name]), rb[name] >= 16))
    assert {g for g, _ in seen} == {16, 8, 4, 2, 1}
    assert {g for g, wide in seen if wide} >= {16, 8, 2, 1} and {g for g, wide in seen if not wide} == {8, 4, 2, 1}


@pytest.mark.parametrize("case", sorted(CK_CASES))
def test_checkers_pack_and_expand_wide_build(case):
    from cm3_amd import _lib
    tj = _CkTraj(case)
    T, E = CK_T, CK_E
    n, size = T * E, T * E + 11
    rng = np.random.default_rng(11)
    rb, rb_wide = _ck_row_bytes(tj, False), _ck_row_bytes(tj, True)
    whole = np.arange(n)
    cols = {k: _np_u8(v) for k, v in tj.columns(whole // E, whole % E, False).items()}
    assert {k: v.shape[1] for k, v in cols.items()} == rb
    for start in (0, 5, size - 7):       # no wrap; an unaligned first piece; a wrap with both the [lo_a, hi_a) and the [0, hi_b) chunk
        init = {k: rng.integers(0, 256, (size, b), dtype=np.uint8) for k, b in rb.items()}
        want = {k: v.copy() for k, v in init.items()}
        for k in want:
            want[k][(start + whole) % size] = cols[k]

        def pack():
            ring = _ck_alloc(init)
            st = _lib.fill_checkers_cols(_lib.CheckersCompactCols(), ring, start, size)
            _lib.check(_lib.lib().cm3_checkers_transitions_pack(ctypes.byref(tj.desc), ctypes.byref(tj.traj), tj.d["prev0"].data_ptr(), n,
                                                                ctypes.byref(st), _stream()))
            return ring
        rule, forced = _both(pack)
        _ck_assert(forced, rule, want, (case, "pack", start))
        # expand: ring rows -> the reference's columns.  Rows the pack left alone hold random bytes: whatever they hold is widened
        typed = dict(grid=np.int8, vec=np.int32, obs_self_t=np.int8)
        index = rng.integers(0, size, 300)
        index[:30] = index[30]                               # repeats
        for idx in (None, index):
            take = np.arange(size) if idx is None else idx
            exp = {}
            for name, record in _lib.CHECKERS_COLUMN_RECORDS:
                r = want[name][take]
                if record in typed:
                    exp[name] = _np_u8(np.ascontiguousarray(r).view(typed[record]).astype(np.float64))
                elif record == "done":
                    exp[name] = (r != 0).astype(np.uint8)
                elif record == "goals":
                    exp[name] = _np_u8(np.stack([r == 0, r == 1], -1).astype(np.int64))
                else:
                    exp[name] = r
            assert {k: v.shape[1] for k, v in exp.items()} == rb_wide
            d_idx = None if idx is None else _dev(idx.astype(np.int64))
            fill = {k: rng.integers(0, 256, (len(take), b), dtype=np.uint8) for k, b in rb_wide.items()}

            def expand():
                out = _ck_alloc(fill)
                src = _lib.fill_checkers_cols(_lib.CheckersCompactCols(), forced, 0, size)
                dst = _lib.fill_checkers_cols(_lib.CheckersTransitionCols(), out)
                _lib.check(_lib.lib().cm3_checkers_ring_expand(ctypes.byref(tj.desc), ctypes.byref(src), _lib.ptr(d_idx), len(take),
                                                               ctypes.byref(dst), _stream()))
                return out
            e_rule, e_forced = _both(expand)
            _ck_assert(e_forced, e_rule, exp, (case, "expand", start, idx is None))


# ---- cm3_transitions_gather_f32 / cm3_transitions_route_f32 -----------------------------------------------------------------------
@pytest.mark.parametrize("N,cfg", [(1, "particle_stage1.json"), (2, "particle_stage2_merge.json"), (4, "particle_stage2_cross.json")])
def test_particle_transition_export_wide_build(N, cfg):
    from cm3_amd.particle import VecParticleEnv
    from cm3_amd.rollout import ParticleRollout
    E, T = 96, 12
    env = VecParticleEnv(load_cfg(cfg), N, 0.2, 5, E, device=DEV, dtype=torch.float32, auto_reset=True, seed=21)
    env.reset()
    ro = ParticleRollout(env, n_ticks=T, use_graph=False).collect()
    assert ro.term_state is not None and int(ro.done.sum()) >= E        # terminal capture; max_steps = 5: every env ends twice
    g = torch.Generator(device="cpu").manual_seed(4)
    B = T * E
    whole = torch.arange(B, device=DEV)
    tt_all, ee_all = torch.div(whole, E, rounding_mode="floor"), whole % E
    want_all = ro.as_reference_batch_torch(tt_all, ee_all, numpy=False)

    def same(forced, rule, want, what):
        assert set(forced) == set(want)
        for k in want:
            assert forced[k].dtype == want[k].dtype and forced[k].shape == want[k].shape, (what, k)
            assert torch.equal(forced[k], want[k]), (what, k)
            assert torch.equal(rule[k], forced[k]), (what, k)
    # the whole trajectory, no index arrays
    rule, forced = _both(lambda: ro.as_reference_batch(numpy=False))
    same(forced, rule, want_all, "whole")
    # 500 random (tick, env) pairs with repeats
    pick = torch.randint(0, B, (500,), generator=g).to(DEV)
    pick[:20] = pick[20]
    rule, forced = _both(lambda: ro.as_reference_batch(tt_all[pick], ee_all[pick], numpy=False))
    same(forced, rule, ro.as_reference_batch_torch(tt_all[pick], ee_all[pick], numpy=False), "indexed")
    # routed: rows to each of three column sets, some skipped
    sel = torch.tensor([0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 4, (B,), generator=g)]
    row = torch.full((B,), -1, dtype=torch.int64)
    rows = B + 3
    for k in range(3):
        m = (sel == k).nonzero().reshape(-1)
        assert m.numel() > 0
        row[m] = torch.randperm(rows, generator=g)[:m.numel()]
    assert int((sel == 255).sum()) > 0
    d_sel, d_row = sel.to(DEV), row.to(DEV)

    def route():
        sets = [(ro.empty_columns(rows, zero=True), rows) for _ in range(3)]
        ro.route_into(sets, d_sel, d_row)
        return sets
    rule, forced = _both(route)
    for k in range(3):
        m = (d_sel == k).nonzero().reshape(-1)
        want = {}
        for name, v in want_all.items():
            w = torch.zeros((rows,) + tuple(v.shape[1:]), dtype=v.dtype, device=DEV)
            w[d_row[m]] = v[m]
            want[name] = w
        same(forced[k][0], rule[k][0], want, ("route", k))
    ro.close()


# ---- the flag itself -----------------------------------------------------------------------------------------------------------------
def test_force_refuses_other_widths_and_the_rule_returns():
    from cm3_amd import _lib
    lib = _lib.lib()
    assert lib.cm3_rows_force_index_width(32) != 0          # refused on purpose: narrow above the limit would write out of range
    assert lib.cm3_rows_force_index_width(7) != 0
    src, idx = torch.arange(64, dtype=torch.int32, device=DEV).reshape(16, 4), torch.tensor([3, 3, 0, 15], device=DEV)

    def launch():
        dst = torch.empty(4, 4, dtype=torch.int32, device=DEV)
        _lib.rows_gather([(dst, src)], 4, idx, _stream())
        assert torch.equal(dst, src[idx])
        return _lib.rows_last_index_width()
    assert launch() == 32                                   # the refused calls changed nothing
    with _lib.force_rows_index_width(64):
        assert launch() == 64
    assert launch() == 32
    with pytest.raises(RuntimeError):
        with _lib.force_rows_index_width(64):
            raise RuntimeError("leaves the block")
    assert launch() == 32


# ---- addresses beyond 4 GiB ----------------------------------------------------------------------------------------------------------
def test_rows_copy_addresses_beyond_4_gib():
    """copy_units forms (size_t)row * units_per_row + unit from a caller's row index: a column above 4 GiB is reached with a handful of
    rows (a default wide Checkers ring: 10^6 rows of 4800 B).  One uint8 column of (2^20 + 256) x 4096 bytes, 4 GiB + 1 MiB, never filled
    as a whole.  Row r >= 2^20 lies 2^32 bytes behind row r - 2^20: that is where a byte offset truncated to 32 bits would land, inside
    the allocation, so a defect shows as a failed assertion.  The width is the rule's choice (32): narrow UNIT arithmetic with size_t
    ADDRESSING is what is checked.  (1.4 % of the device's memory; no skip for low memory: a skipped test would hide the case.)"""
    from cm3_amd import _lib
    HI, RB = 1 << 20, 4096
    rows = HI + 256
    big = torch.empty((rows, RB), dtype=torch.uint8, device=DEV)
    assert big.numel() > (1 << 32) and big.data_ptr() % 16 == 0
    g = torch.Generator(device="cpu").manual_seed(9)
    # dst_row mode: 32 rows below 256 (even ones), 32 above 2^20 whose truncated twins are the ODD rows below 256
    low = torch.randperm(128, generator=g)[:32] * 2
    high = HI + torch.randperm(128, generator=g)[:32] * 2 + 1
    dst_row = torch.cat([low, high])[torch.randperm(64, generator=g)].to(torch.int64)
    twins = (high - HI).to(DEV)
    for mode in ("dst_row", "ring"):
        src = torch.randint(0, 256, (64, RB), generator=g, dtype=torch.int64).to(torch.uint8).to(DEV)
        sentinel = torch.randint(0, 256, (32 if mode == "dst_row" else 5, RB), generator=g, dtype=torch.int64).to(torch.uint8).to(DEV)
        if mode == "dst_row":
            where, guard = dst_row.to(DEV), twins
            big[guard] = sentinel
            _lib.rows_scatter([(big, src)], 64, _stream(), dst_row=where)
        else:
            start = rows - 5                                 # rows - 5 .. rows - 1 lie above 4 GiB, then the ring wraps to rows 0 .. 58
            where = (start + torch.arange(64, device=DEV)) % rows
            guard = where[:5] - HI                           # rows 251 .. 255: not among the 59 the wrap writes
            assert int(guard.min()) > 58 and int((where[:5] * RB).min()) > (1 << 32)
            big[guard] = sentinel
            _lib.rows_scatter([(big, src)], 64, _stream(), ring_start=start, ring_size=rows)
        assert _lib.rows_last_index_width() == 32
        back = torch.zeros(64, RB, dtype=torch.uint8, device=DEV)
        _lib.rows_gather([(back, big)], 64, where.contiguous(), _stream())
        assert _lib.rows_last_index_width() == 32
        assert torch.equal(back, src), mode                  # what went in beyond 4 GiB comes back from there
        assert torch.equal(big[guard], sentinel), mode       # and did not land 2^32 bytes short
        assert torch.equal(big[where], src), mode            # (torch's own 64-bit indexing agrees)
    del big
