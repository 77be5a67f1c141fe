"""ParticleCritic and CheckersCritic -- the reference's CM3 critics evaluated on the device over the rows of a sampled batch.

    reference                                                    here
    ---------------------------------------------------------   -----------------------------------------------
    networks.Q_global_1output(s_n, g_n, a_n, s_others, a_others)  ParticleCritic(weights, n_agents, kind="global")
      (networks.py:97-122; scopes Q_global_main / _target)
    networks.Q_credit(s_n, g_n, a_m, s_m, s_others)               ParticleCritic(weights, n_agents, kind="credit")
      (networks.py:186-211; scopes Q_credit_main / _target)
    sess.run(Q_global_target, feed) + the TD target               critic.q_rows(v_global_next, goals, a', reward, done, gamma)
      (alg_credit.py:585-594)
    sess.run(Q_credit_target, feed) + the TD target               critic.q_pairs(v_global_next, goals, a', reward, done, gamma)
      (alg_credit.py:616-640)
    sess.run(Q_credit, n x n x l_action counterfactual feed)      critic.q_counterfactual(v_global, goals)
      (alg_credit.py:730-751; stage 1: sess.run(Q_global, ...) :716-727)

Every method is ONE launch of cm3_critic_particle_rows_f32, which takes no tiled feed: the n x n x 5 tilings the reference builds
on the host are index functions of the batch's base columns (state [B, N, 4], goals [B, N, 2], actions [B, N]) and the kernel
decodes them from the row number.  The network is float32 throughout, every contraction an exact-f32 k-ordered chain.

Weights stay float32 [in][out] as TensorFlow shapes them, in ``self.w`` under short names (NAMES below), so a session that trains
the main critics can write updated variables INTO these tensors in place; ``repack()`` (one launch on persistent tensors,
capturable) then makes the next launch follow them.  Scope prefixes "Q_global_main/", "Q_global_target/", "Q_credit_main/",
"Q_credit_target/" and a ":0" suffix of the keys are ignored.  Loading and ``soft_update_from(main, tau)`` -- the critic's part of
list_update_target_ops (alg_credit.py:186-194), for a critic holding target weights -- are cm3_amd._net._DeviceNet's.

CheckersCritic (below) is the Checkers twin: networks.Q_global_checkers / Q_credit_checkers at the widths of
config_checkers_stage{1,2}.json, one launch of cm3_critic_checkers_rows_f32 per method on the base columns grid, vec, goals, actions,
obs_self_t, obs_self_v.
"""
import ctypes

import torch

from . import _lib
from ._lib import Cm3Error
from ._net import _DeviceNet, _keep, canon, stage_td_cols, td_given, td_outputs

H1_1, H1_2, H2, N_ACTIONS = 64, 128, 64, 5
KINDS = {"global": _lib.CRITIC_GLOBAL, "credit": _lib.CRITIC_CREDIT}
NAMES = {"w_b1": "Q_branch1/kernel", "b_b1": "Q_branch1/bias", "w_b1_h2": "W_branch1_h2",
         "w_b2": "stage-2/Q_branch2/kernel", "b_b2": "stage-2/Q_branch2/bias", "w_b2_h2": "stage-2/W_branch2_h2",
         "w_out": "Q_out/kernel"}
_PREFIXES = ("Q_global_main/", "Q_global_target/", "Q_credit_main/", "Q_credit_target/")


def _canon(name):
    return canon(name, _PREFIXES)


def weight_shapes(n_agents, kind, stage):
    """short name -> shape of the TF variable, for the tensors a critic of this kind / stage has"""
    shapes = {"w_b1": (11, H1_1), "b_b1": (H1_1,), "w_b1_h2": (H1_1, H2), "w_out": (H2, 1)}
    if stage > 1:
        k2 = 9 * (n_agents - 1) if kind == "global" else 4 * n_agents
        shapes.update({"w_b2": (k2, H1_2), "b_b2": (H1_2,), "w_b2_h2": (H1_2, H2)})
    return shapes


class ParticleCritic(_DeviceNet):
    _match = ("n", "kind", "stage")
    _refusal = "the main critic must be a %(kind)s ParticleCritic for %(n)d agents at stage %(stage)d"

    def __init__(self, weights, n_agents, kind="global", stage=2, device="cuda:0"):
        """kind "global": networks.Q_global_1output -- stage 1 with one agent, stage 2 with more; kind "credit": networks.Q_credit,
        stage 2 with more than one agent.  float32 only."""
        self.device = _lib.require_gpu(device)
        if kind not in KINDS:
            raise Cm3Error("kind must be one of %s" % sorted(KINDS))
        self.kind, self.n, self.stage = kind, int(n_agents), int(stage)
        if not 1 <= self.n <= _lib.MAX_AGENTS:
            raise Cm3Error("n_agents must be in 1..%d" % _lib.MAX_AGENTS)
        if kind == "credit" and (self.n == 1 or self.stage != 2):
            raise Cm3Error("Q_credit exists at stage 2 with more than one agent only (n_agents %d, stage %d)" % (self.n, self.stage))
        if self.stage not in (1, 2) or (self.stage == 1) != (self.n == 1):
            raise Cm3Error("Q_global_1output runs at stage 1 with one agent and at stage 2 with more (n_agents %d, stage %d)"
                           % (self.n, self.stage))
        self._load(weights, _PREFIXES, NAMES, weight_shapes(self.n, kind, self.stage), "critic",
                   lambda lib: lib.cm3_critic_particle_packed_bytes(self.n, KINDS[kind]), _lib.CriticParticleWeights())

    def _desc(self):
        d = _lib.CriticParticleDesc()
        d.n_agents, d.stage, d.kind = self.n, self.stage, KINDS[self.kind]
        d.n_h1_1, d.n_h1_2, d.n_h2 = H1_1, H1_2, H2
        return d

    def repack(self):
        """Re-arrange the (possibly updated in place) TF-shaped weights into the rows kernel's layout: one launch."""
        d = self._desc()
        _lib.check(self._lib.cm3_critic_particle_pack(ctypes.byref(d), ctypes.byref(self._wt), self._packed.data_ptr(),
                                                      self._stream(None)))

    # ---- launches -------------------------------------------------------------------------------------------------------------------
    def enqueue(self, form, n_steps, state, goals, actions=None, reward=None, done=None, gamma=0.0, q=None, q64=None, td=None,
                stream=None):
        """Raw launch of cm3_critic_particle_rows_f32 on contiguous device tensors: state / goals float32, actions int32, reward
        float32 or float64, done uint8; every output is optional, one is required."""
        r = _lib.CriticRows()
        r.form, r.n_steps = int(form), int(n_steps)
        r.state, r.goals, r.actions = _lib.ptr(state), _lib.ptr(goals), _lib.ptr(actions)
        r.reward, r.done = _lib.ptr(reward), _lib.ptr(done)
        r.reward_f64 = 1 if (reward is not None and reward.dtype == torch.float64) else 0
        r.gamma = float(gamma)
        r.q, r.q64, r.td = _lib.ptr(q), _lib.ptr(q64), _lib.ptr(td)
        d = self._desc()
        s = self._stream(stream)
        _lib.check(self._lib.cm3_critic_particle_rows_f32(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(r), s))

    def _stage_cols(self, what, state, goals, actions=None, reward=None, done=None):
        """(B, state, goals, actions, reward, done) contiguous on the critic's device from [B, N, 4], [B, N, 2], [B, N], [B, N] and
        [B] (leading dimensions may be merged: [B * N, 4] ...).  Float columns of any dtype are rounded to float32, as the
        reference's tf.float32 placeholders do; reward stays float32 or float64 (another dtype is widened to float64)."""
        N = self.n
        if state.shape[-1] != 4 or goals.shape[-1] != 2 or state.numel() // 4 != goals.numel() // 2 or (state.numel() // 4) % N:
            raise Cm3Error("%s takes state [B, %d, 4] and goals [B, %d, 2], got %s and %s"
                           % (what, N, N, tuple(state.shape), tuple(goals.shape)))
        B = state.numel() // (4 * N)
        if B <= 0:
            raise Cm3Error("%s needs at least one time step" % what)
        f32 = lambda t: t.to(device=self.device, dtype=torch.float32).contiguous()      # noqa: E731
        state, goals = f32(state).reshape(B, N, 4), f32(goals).reshape(B, N, 2)
        actions, reward, done = stage_td_cols(what, self.device, B, N, actions, reward, done)
        return B, state, goals, actions, reward, done

    def _q(self, what, form, per_step, state, goals, actions, reward, done, gamma, keep):
        td = td_given(what, "reward", reward, done, gamma)
        if actions is None:
            raise Cm3Error("%s needs actions" % what)
        B, st, go, ac, rw, dn = self._stage_cols(what, state, goals, actions, reward, done)
        out = td_outputs(self.device, B * per_step, "q", td)
        _keep(keep, st, go, ac, rw, dn, *out.values())
        self.enqueue(form, B, st, go, ac, rw, dn, 0.0 if gamma is None else gamma, **out)
        return out

    def q_rows(self, state, goals, actions, reward=None, done=None, gamma=None, keep=None):
        """Q_global_1output over the B * N agent rows r = b N + n of a batch, ONE launch: s_n, g_n and a = onehot(actions[b, n]) of
        the row's agent, s_others / a_others over the other agents in ascending order -- the feed of sess.run(Q_global_target)
        (alg_credit.py:585-591) with state = v_global_next and actions = the target actor's samples.  Returns a dict of device
        tensors: "q" float32 [R, 1], "q64" the same values float64 [R, 1], and with reward [B, N] (float32 / float64), done [B] and
        gamma also "td" float64 [R] = reward + gamma * q * (1 - done), the bits of batch.td_target on q64.  keep: an optional list
        that receives every tensor the launch touches (the staged inputs, the outputs), for whoever captures the launch."""
        if self.kind != "global":
            raise Cm3Error("q_rows is the Q_global form; a credit critic takes q_pairs / q_counterfactual")
        return self._q("q_rows", _lib.CRITIC_ROWS, self.n, state, goals, actions, reward, done, gamma, keep)

    def q_pairs(self, state, goals, actions, reward=None, done=None, gamma=None, keep=None):
        """Q_credit over the B * N * N rows r = (b N + m) N + n, ONE launch: s_n, g_n, s_others of agent n, a = onehot(actions[b, m])
        and s_m = state[b, m] -- the feed of sess.run(Q_credit_target) (alg_credit.py:616-633).  Returns as q_rows; "td" takes
        reward[b, n] and done[b]."""
        if self.kind != "credit":
            raise Cm3Error("q_pairs is the Q_credit form; a global critic takes q_rows")
        return self._q("q_pairs", _lib.CRITIC_PAIRS, self.n * self.n, state, goals, actions, reward, done, gamma, keep)

    def q_counterfactual(self, state, goals, keep=None):
        """The critic at every action, float32 [R', 5], ONE launch and no action array: a credit critic over the R' = B * N * N pairs
        of q_pairs (alg_credit.py:730-751), a global critic with one agent over the R' = B time steps (stage 1, :716-727).  Column
        a of a credit row holds the bits q_pairs gives that row when actions[b, m] = a."""
        if self.kind == "global" and self.n != 1:
            raise Cm3Error("q_counterfactual of a global critic is the one-agent (stage 1) form")
        B, st, go, _, _, _ = self._stage_cols("q_counterfactual", state, goals)
        per_step = 1 if self.kind == "global" else self.n * self.n
        q = torch.empty(B * per_step, N_ACTIONS, dtype=torch.float32, device=self.device)
        _keep(keep, st, go, q)
        self.enqueue(_lib.CRITIC_CF, B, st, go, q=q)
        return q


# ---- Checkers -------------------------------------------------------------------------------------------------------------------------
CK_H1_1, CK_H1_2, CK_H2 = 256, 32, 256              # Q_n_h1_1, Q_n_h1_2, Q_n_h2 of config_checkers_stage{1,2}.json
CK_MAX_AGENTS = 8                                   # the Checkers actor's range
CK_GRID, CK_WINDOW = (3, 9, 2), (5, 5, 3)
CK_NAMES = {"conv_w": "conv/Conv/weights", "conv_b": "conv/Conv/biases", "conv_o_w": "conv_o/Conv/weights",
            "conv_o_b": "conv_o/Conv/biases", "w_b1": "Q_branch1/kernel", "b_b1": "Q_branch1/bias", "w_b1_h2": "W_branch1_h2",
            "w_b2": "stage-2/Q_branch2/kernel", "b_b2": "stage-2/Q_branch2/bias", "w_b2_h2": "stage-2/W_branch2_h2",
            "w_out": "Q_out/kernel", "b_out": "Q_out/bias"}


def checkers_weight_shapes(n_agents, kind, stage):
    """short name -> shape of the TF variable, for the tensors a Checkers critic of this kind / stage has"""
    shapes = {"conv_w": (3, 5, 2, 4), "conv_b": (4,), "conv_o_w": (3, 3, 3, 6), "conv_o_b": (6,), "w_b1": (273, CK_H1_1),
              "b_b1": (CK_H1_1,), "w_b1_h2": (CK_H1_1, CK_H2), "w_out": (CK_H2, 1), "b_out": (1,)}
    if stage > 1:
        k2 = 9 * (n_agents - 1) if kind == "global" else 4 * n_agents
        shapes.update({"w_b2": (k2, CK_H1_2), "b_b2": (CK_H1_2,), "w_b2_h2": (CK_H1_2, CK_H2)})
    return shapes


class CheckersCritic(_DeviceNet):
    """The reference's Checkers critics on the device over the rows of a sampled batch, the twin of ParticleCritic.

        reference                                                        here
        -------------------------------------------------------------   ------------------------------------------------
        networks.Q_global_checkers (networks.py:155-183)                 CheckersCritic(weights, n_agents, kind="global")
        networks.Q_credit_checkers (:244-272)                            CheckersCritic(weights, n_agents, kind="credit")
        sess.run(Q_global_target) + TD target                            critic.q_rows(next_grid, next_vec, goals, a', next_obs_self_t,
          (alg_credit_checkers.py:558-572)                                 next_obs_self_v, reward, done, gamma)
        sess.run(Q_credit_target) + TD target (:611-632)                 critic.q_pairs(...the same arguments...)
        sess.run(Q_credit, n x n x l_action feed) (:738-747;             critic.q_counterfactual(grid, vec, goals, obs_self_t, obs_self_v)
          stage 1: sess.run(Q_global) :704-713)

    Columns: grid [B, 3, 9, 2]; vec [B, N, 4]; goals one-hot [B, N, 2] or indices [B, N]; actions [B, N]; obs_self_t [B, N, 5, 5, 3]
    (or [B, N, 75]); obs_self_v [B, N, 4] (leading dimensions may be merged).  int8 grids and windows and uint8 index goals go in as
    they are; everything else is staged to float64 / int64 as cm3_amd.actor.stage_checkers_rows does, and rounded to float32 in the
    kernel as the reference's tf.float32 placeholders do.  In the pair forms the window and obs_self_v of a row are agent M's (the
    reference repeats them "indexed by m").  Weights: ``self.w`` under the short names of CK_NAMES, see ParticleCritic."""
    _match = ("n", "kind", "stage")
    _refusal = "the main critic must be a %(kind)s CheckersCritic for %(n)d agents at stage %(stage)d"

    def __init__(self, weights, n_agents, kind="global", stage=2, device="cuda:0"):
        self.device = _lib.require_gpu(device)
        if kind not in KINDS:
            raise Cm3Error("kind must be one of %s" % sorted(KINDS))
        self.kind, self.n, self.stage = kind, int(n_agents), int(stage)
        if not 1 <= self.n <= CK_MAX_AGENTS:
            raise Cm3Error("n_agents must be in 1..%d" % CK_MAX_AGENTS)
        if kind == "credit" and (self.n == 1 or self.stage != 2):
            raise Cm3Error("Q_credit_checkers exists at stage 2 with more than one agent only (n_agents %d, stage %d)"
                           % (self.n, self.stage))
        if self.stage not in (1, 2) or (self.stage == 1) != (self.n == 1):
            raise Cm3Error("Q_global_checkers runs at stage 1 with one agent and at stage 2 with more (n_agents %d, stage %d)"
                           % (self.n, self.stage))
        self._load(weights, _PREFIXES, CK_NAMES, checkers_weight_shapes(self.n, kind, self.stage), "critic",
                   lambda lib: lib.cm3_critic_checkers_packed_bytes(self.n, KINDS[kind]), _lib.CriticCheckersWeights())

    def _desc(self):
        d = _lib.CriticCheckersDesc()
        d.n_agents, d.stage, d.kind = self.n, self.stage, KINDS[self.kind]
        (d.grid_h, d.grid_w, d.grid_c), (d.win_h, d.win_w, d.win_c) = CK_GRID, CK_WINDOW
        d.n_h1_1, d.n_h1_2, d.n_h2 = CK_H1_1, CK_H1_2, CK_H2
        return d

    def repack(self):
        """Re-arrange the (possibly updated in place) TF-shaped weights into the rows kernel's layout, the two convolutions as
        Toeplitz matrices: one launch."""
        d = self._desc()
        _lib.check(self._lib.cm3_critic_checkers_pack(ctypes.byref(d), ctypes.byref(self._wt), self._packed.data_ptr(),
                                                      self._stream(None)))

    # ---- launches -------------------------------------------------------------------------------------------------------------------
    def enqueue(self, form, n_steps, grid, vec, goals, windows, obs_self_v, actions=None, reward=None, done=None, gamma=0.0, q=None,
                q64=None, td=None, stream=None):
        """Raw launch of cm3_critic_checkers_rows_f32 on contiguous device tensors: grid / windows int8 or float64, vec / obs_self_v
        float64, goals uint8 indices or int64 one-hot, actions int32, reward float32 or float64, done uint8; every output is
        optional, one is required."""
        r = _lib.CriticCheckersRows()
        r.form, r.n_steps = int(form), int(n_steps)
        r.grid_f64 = 0 if grid.dtype == torch.int8 else 1
        r.windows_f64 = 0 if windows.dtype == torch.int8 else 1
        r.goals_onehot = 0 if goals.dtype == torch.uint8 else 1
        r.grid, r.vec, r.goals, r.actions = _lib.ptr(grid), _lib.ptr(vec), _lib.ptr(goals), _lib.ptr(actions)
        r.windows, r.obs_self_v = _lib.ptr(windows), _lib.ptr(obs_self_v)
        r.reward, r.done = _lib.ptr(reward), _lib.ptr(done)
        r.reward_f64 = 1 if (reward is not None and reward.dtype == torch.float64) else 0
        r.gamma = float(gamma)
        r.q, r.q64, r.td = _lib.ptr(q), _lib.ptr(q64), _lib.ptr(td)
        d = self._desc()
        s = self._stream(stream)
        _lib.check(self._lib.cm3_critic_checkers_rows_f32(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(r), s))

    def _stage_cols(self, what, grid, vec, goals, obs_self_t, obs_self_v, actions=None, reward=None, done=None):
        """(B, grid, vec, goals, windows, obs_self_v, actions, reward, done) contiguous on the critic's device in the forms the kernel
        reads: int8 grids / windows and uint8 index goals as they are, everything else float64 / int64 one-hot."""
        N = self.n
        if vec.shape[-1] != 4 or (vec.numel() // 4) % N or vec.numel() == 0:
            raise Cm3Error("%s takes vec [B, %d, 4], got %s" % (what, N, tuple(vec.shape)))
        B = vec.numel() // (4 * N)
        if (grid.numel() != B * 54 or obs_self_t.numel() != B * N * 75 or obs_self_v.numel() != B * N * 4
                or goals.numel() not in (B * N, B * N * 2)):
            raise Cm3Error("%s takes grid [B, 3, 9, 2], goals [B, %d, 2] (or [B, %d]), obs_self_t [B, %d, 5, 5, 3] and obs_self_v "
                           "[B, %d, 4] for %d time steps, got %s, %s, %s, %s"
                           % (what, N, N, N, N, B, tuple(grid.shape), tuple(goals.shape), tuple(obs_self_t.shape),
                              tuple(obs_self_v.shape)))
        stage = lambda t, dt: t.to(device=self.device, dtype=dt).contiguous()      # noqa: E731
        narrow = lambda t: stage(t, torch.int8 if t.dtype == torch.int8 else torch.float64)      # noqa: E731
        if goals.numel() == B * N:      # indices (a one-hot column has twice as many elements)
            go = (stage(goals, torch.uint8) if goals.dtype == torch.uint8
                  else torch.nn.functional.one_hot(goals.to(self.device).long(), 2).contiguous())
        else:
            go = stage(goals, torch.int64)
        actions, reward, done = stage_td_cols(what, self.device, B, N, actions, reward, done)
        return B, narrow(grid), stage(vec, torch.float64), go, narrow(obs_self_t), stage(obs_self_v, torch.float64), actions, reward, done

    def _q(self, what, form, per_step, grid, vec, goals, actions, obs_self_t, obs_self_v, reward, done, gamma, keep):
        td = td_given(what, "reward", reward, done, gamma)
        if actions is None:
            raise Cm3Error("%s needs actions" % what)
        B, gr, ve, go, wi, ov, ac, rw, dn = self._stage_cols(what, grid, vec, goals, obs_self_t, obs_self_v, actions, reward, done)
        out = td_outputs(self.device, B * per_step, "q", td)
        _keep(keep, gr, ve, go, wi, ov, ac, rw, dn, *out.values())
        self.enqueue(form, B, gr, ve, go, wi, ov, ac, rw, dn, 0.0 if gamma is None else gamma, **out)
        return out

    def q_rows(self, grid, vec, goals, actions, obs_self_t, obs_self_v, reward=None, done=None, gamma=None, keep=None):
        """Q_global_checkers over the B * N agent rows r = b N + n of a batch, ONE launch: the grid of step b; s_n, g_n, window, v_obs
        and a = onehot(actions[b, n]) of the row's agent; s_others / a_others over the other agents in ascending order -- the feed of
        sess.run(Q_global_target) (alg_credit_checkers.py:558-569) with the next-step columns and the target actor's samples.
        Returns a dict of device tensors: "q" float32 [R, 1], "q64" the same values float64 [R, 1], and with reward [B, N] (float32 /
        float64), done [B] and gamma also "td" float64 [R] = reward + gamma * q * (1 - done), the bits of batch.td_target on q64.
        keep: an optional list that receives every tensor the launch touches, for whoever captures the launch."""
        if self.kind != "global":
            raise Cm3Error("q_rows is the Q_global form; a credit critic takes q_pairs / q_counterfactual")
        return self._q("q_rows", _lib.CRITIC_ROWS, self.n, grid, vec, goals, actions, obs_self_t, obs_self_v, reward, done, gamma, keep)

    def q_pairs(self, grid, vec, goals, actions, obs_self_t, obs_self_v, reward=None, done=None, gamma=None, keep=None):
        """Q_credit_checkers over the B * N * N rows r = (b N + m) N + n, ONE launch: s_n, g_n, s_others of agent n; a =
        onehot(actions[b, m]), s_m = vec[b, m], and the window and v_obs of agent m -- the feed of sess.run(Q_credit_target)
        (alg_credit_checkers.py:596-629).  Returns as q_rows; "td" takes reward[b, n] and done[b]."""
        if self.kind != "credit":
            raise Cm3Error("q_pairs is the Q_credit form; a global critic takes q_rows")
        return self._q("q_pairs", _lib.CRITIC_PAIRS, self.n * self.n, grid, vec, goals, actions, obs_self_t, obs_self_v, reward, done,
                       gamma, keep)

    def q_counterfactual(self, grid, vec, goals, obs_self_t, obs_self_v, keep=None):
        """The critic at every action, float32 [R', 5], ONE launch and no action array: a credit critic over the R' = B * N * N pairs
        of q_pairs (alg_credit_checkers.py:738-747), a global critic with one agent over the R' = B time steps (stage 1, :704-713).
        Column a of a credit row holds the bits q_pairs gives that row when actions[b, m] = a."""
        if self.kind == "global" and self.n != 1:
            raise Cm3Error("q_counterfactual of a global critic is the one-agent (stage 1) form")
        B, gr, ve, go, wi, ov, _, _, _ = self._stage_cols("q_counterfactual", grid, vec, goals, obs_self_t, obs_self_v)
        per_step = 1 if self.kind == "global" else self.n * self.n
        q = torch.empty(B * per_step, N_ACTIONS, dtype=torch.float32, device=self.device)
        _keep(keep, gr, ve, go, wi, ov, q)
        self.enqueue(_lib.CRITIC_CF, B, gr, ve, go, wi, ov, q=q)
        return q
