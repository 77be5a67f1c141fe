"""ParticleValue and ParticleComaCritic -- the value networks of the reference's IAC / COMA baselines (alg/alg_baseline.py) evaluated on
the device over the rows of a sampled batch.

    reference                                                       here
    ------------------------------------------------------------   --------------------------------------------------
    networks.V_particle_local(obs_others, v_obs, v_goal)             ParticleValue(weights, n_agents, kind="local")
      (networks.py:356-374; IAC; scopes V_main / V_target)
    networks.V_particle_global(s_n, g_n, s_others, g_others)         ParticleValue(weights, n_agents, kind="global")
      (networks.py:377-402; scopes V_main / V_target)
    networks.Q_global(state, a_others, g_n, g_others, label, v_obs)  ParticleComaCritic(weights, n_agents)
      (networks.py:84-94; COMA; scopes Q_main / Q_target)
    sess.run([V_target, V], next-step feed) + the TD target          value.v_rows(..., reward_local, done, gamma)
      (alg_baseline.py:524-539, :604)
    sess.run(Q_target, feed), the own action's column, TD target     critic.q_rows(v_global_next, goals, a', v_local_next, reward,
      (alg_baseline.py:565-581)                                        done, gamma)
    sess.run(Q, feed) (alg_baseline.py:608-616)                      critic.q_rows(v_global, goals, actions, v_local)["q"]

Every method is ONE launch (cm3_value_particle_rows_f32 / cm3_coma_particle_rows_f32) that takes no tiled feed: goals_others,
v_global_others, the repeated state, the others' one-hot actions and the agent labels the reference builds on the host are index
functions of the batch's base columns, and the kernel decodes them from the row number r = b N + n.  float32 throughout, every
contraction an exact-f32 k-ordered chain.

Weights stay float32 [in][out] as TensorFlow shapes them, in ``self.w`` under short names (VALUE_NAMES / COMA_NAMES below), so a
session that trains the main networks can write updated variables INTO these tensors in place; ``repack()`` (one launch on
persistent tensors, capturable) then makes the next launch follow them.  Scope prefixes "V_main/", "V_target/" ("Q_main/",
"Q_target/") and a ":0" suffix of the keys are ignored.  Loading and ``soft_update_from(main, tau)`` -- the network's part of
list_update_target_ops (alg_baseline.py:165-212), for an object holding target weights -- are cm3_amd._net._DeviceNet's.

CheckersValue and CheckersComaCritic (below) are the Checkers twins (alg/alg_baseline_checkers.py): networks.V_checkers_local /
V_checkers_global (networks.py:415-458) and networks.Q_coma_checkers (:293-306), one launch of cm3_value_checkers_rows_f32 /
cm3_coma_checkers_rows_f32 per method on the base columns grid, vec, goals, actions, obs_self_t, obs_self_v, obs_others.
"""
import ctypes

import torch

from . import _lib
from ._lib import Cm3Error
from ._net import _DeviceNet, _keep, stage_td_cols, td_given, td_outputs

H1, H_OTHERS, H2, Q_UNITS, N_ACTIONS = 64, 128, 64, 256, 5
VALUE_KINDS = {"local": _lib.VALUE_LOCAL, "global": _lib.VALUE_GLOBAL}
VALUE_NAMES = {
    "local": {"w_b1": "V_particle_branch_self/kernel", "b_b1": "V_particle_branch_self/bias", "w_b1_h2": "W_branch_self_out",
              "w_b2": "stage-2/V_local_others/kernel", "b_b2": "stage-2/V_local_others/bias", "w_b2_h2": "stage-2/W_others_out",
              "w_out": "V_particle_out/kernel"},
    "global": {"w_b1": "V_particle_branch1/kernel", "b_b1": "V_particle_branch1/bias", "w_b1_h2": "W_branch1_h2",
               "w_b2": "stage-2/V_particle_branch2/kernel", "b_b2": "stage-2/V_particle_branch2/bias",
               "w_b2_h2": "stage-2/W_branch2_h2", "w_out": "V_particle_out/kernel"}}
COMA_NAMES = {"w_h1": "stage-2/Q_goals/h1/kernel", "b_h1": "stage-2/Q_goals/h1/bias", "w_h2": "stage-2/Q_goals/h2/kernel",
              "b_h2": "stage-2/Q_goals/h2/bias", "w_out": "stage-2/Q_goals/out/kernel", "b_out": "stage-2/Q_goals/out/bias"}
_V_PREFIXES = ("V_main/", "V_target/")
_Q_PREFIXES = ("Q_main/", "Q_target/")

# ---- Checkers (alg/alg_baseline_checkers.py; widths of config_checkers_stage2.json) ------------------------------------------------
CK_MAX_AGENTS, CK_H1_1, CK_H1_2, CK_H2 = 8, 256, 32, 256
CK_VALUE_NAMES = {
    "local": {"conv_w": "conv/Conv/weights", "conv_b": "conv/Conv/biases", "w_b1": "branch_self/kernel", "b_b1": "branch_self/bias",
              "w_b1_h2": "W_self_h2", "w_b2": "stage-2/branch_others/kernel", "b_b2": "stage-2/branch_others/bias",
              "w_b2_h2": "stage-2/W_others_h2", "w_out": "V_checkers_out/kernel", "b_out": "V_checkers_out/bias"},
    "global": {"conv_w": "conv/Conv/weights", "conv_b": "conv/Conv/biases", "w_b1": "V_branch1/kernel", "b_b1": "V_branch1/bias",
               "w_b1_h2": "W_branch1_h2", "w_b2": "stage-2/V_branch2/kernel", "b_b2": "stage-2/V_branch2/bias",
               "w_b2_h2": "stage-2/W_branch2_h2", "w_out": "V_out/kernel", "b_out": "V_out/bias"}}
_QC = "stage-2/Q_coma_checkers/"
CK_COMA_NAMES = {"conv_s_w": "conv_s/Conv/weights", "conv_s_b": "conv_s/Conv/biases", "conv_o_w": "conv_o/Conv/weights",
                 "conv_o_b": "conv_o/Conv/biases", "w_h1": _QC + "h1/kernel", "b_h1": _QC + "h1/bias", "w_h2": _QC + "h2/kernel",
                 "b_h2": _QC + "h2/bias", "w_out": _QC + "out/kernel", "b_out": _QC + "out/bias"}


def checkers_value_k2(n_agents, kind):
    """the width of the second branch's input: obs_others (local), the states of the other agents (global)"""
    return (2 if kind == "local" else 4) * (n_agents - 1)


def checkers_value_weight_shapes(n_agents, kind, stage):
    """short name -> shape of the TF variable, for the tensors a Checkers value network of this kind / stage has"""
    conv, k1 = ((3, 3, 3, 6), 156) if kind == "local" else ((3, 5, 2, 4), 114)
    shapes = {"conv_w": conv, "conv_b": conv[-1:], "w_b1": (k1, CK_H1_1), "b_b1": (CK_H1_1,), "w_b1_h2": (CK_H1_1, CK_H2),
              "w_out": (CK_H2, 1), "b_out": (1,)}
    if stage > 1:
        shapes.update({"w_b2": (checkers_value_k2(n_agents, kind), CK_H1_2), "b_b2": (CK_H1_2,), "w_b2_h2": (CK_H1_2, CK_H2)})
    return shapes


def checkers_coma_weight_shapes(n_agents):
    """short name -> shape of the TF variable of the Checkers COMA critic; its input is 257 + 12 N wide"""
    return {"conv_s_w": (3, 5, 2, 4), "conv_s_b": (4,), "conv_o_w": (3, 3, 3, 6), "conv_o_b": (6,),
            "w_h1": (257 + 12 * n_agents, Q_UNITS), "b_h1": (Q_UNITS,), "w_h2": (Q_UNITS, Q_UNITS), "b_h2": (Q_UNITS,),
            "w_out": (Q_UNITS, N_ACTIONS), "b_out": (N_ACTIONS,)}


def value_k2(n_agents, kind):
    """the width of the second branch's input: obs_others (local), the others' states and goals (global)"""
    return (4 if kind == "local" else 6) * (n_agents - 1)


def value_weight_shapes(n_agents, kind, stage):
    """short name -> shape of the TF variable, for the tensors a value network of this kind / stage has"""
    shapes = {"w_b1": (6, H1), "b_b1": (H1,), "w_b1_h2": (H1, H2), "w_out": (H2, 1)}
    if stage > 1:
        shapes.update({"w_b2": (value_k2(n_agents, kind), H_OTHERS), "b_b2": (H_OTHERS,), "w_b2_h2": (H_OTHERS, H2)})
    return shapes


def coma_weight_shapes(n_agents):
    """short name -> shape of the TF variable of the COMA critic; its input is 12 N - 1 wide"""
    return {"w_h1": (12 * n_agents - 1, Q_UNITS), "b_h1": (Q_UNITS,), "w_h2": (Q_UNITS, Q_UNITS), "b_h2": (Q_UNITS,),
            "w_out": (Q_UNITS, N_ACTIONS), "b_out": (N_ACTIONS,)}


def _f32(device, t, shape):
    return t.to(device=device, dtype=torch.float32).contiguous().reshape(shape)


class ParticleValue(_DeviceNet):
    _match = ("n", "kind", "stage")
    _refusal = "the main network must be a %(kind)s ParticleValue for %(n)d agents at stage %(stage)d"

    def __init__(self, weights, n_agents, kind="local", stage=2, device="cuda:0"):
        """kind "local": networks.V_particle_local (IAC); kind "global": networks.V_particle_global -- stage 1 with one agent, stage 2
        with more.  float32 only."""
        self.device = _lib.require_gpu(device)
        if kind not in VALUE_KINDS:
            raise Cm3Error("kind must be one of %s" % sorted(VALUE_KINDS))
        self.kind, self.n, self.stage = kind, int(n_agents), int(stage)
        if not 1 <= self.n <= _lib.MAX_AGENTS:
            raise Cm3Error("n_agents must be in 1..%d" % _lib.MAX_AGENTS)
        if self.stage not in (1, 2) or (self.stage == 1) != (self.n == 1):
            raise Cm3Error("V_particle_%s runs at stage 1 with one agent and at stage 2 with more (n_agents %d, stage %d)"
                           % (kind, self.n, self.stage))
        self._load(weights, _V_PREFIXES, VALUE_NAMES[kind], value_weight_shapes(self.n, kind, self.stage), "value network",
                   lambda lib: lib.cm3_value_particle_packed_bytes(self.n, VALUE_KINDS[kind]), _lib.ValueParticleWeights())

    def _desc(self):
        d = _lib.ValueParticleDesc()
        d.n_agents, d.stage, d.kind = self.n, self.stage, VALUE_KINDS[self.kind]
        d.n_h1, d.n_others, d.n_h2 = H1, H_OTHERS, H2
        return d

    def repack(self):
        """Re-arrange the (possibly updated in place) TF-shaped weights into the rows kernel's layout: one launch."""
        d = self._desc()
        _lib.check(self._lib.cm3_value_particle_pack(ctypes.byref(d), ctypes.byref(self._wt), self._packed.data_ptr(),
                                                     self._stream(None)))

    def enqueue(self, n_steps, state, goals, obs_others=None, reward=None, done=None, gamma=0.0, v=None, v64=None, td=None,
                stream=None):
        """Raw launch of cm3_value_particle_rows_f32 on contiguous device tensors: state (local: v_obs) / goals / obs_others float32,
        reward float32 or float64, done uint8; every output is optional, one is required."""
        r = _lib.ValueRows()
        r.n_steps = int(n_steps)
        r.state, r.goals, r.obs_others = _lib.ptr(state), _lib.ptr(goals), _lib.ptr(obs_others)
        r.reward, r.done = _lib.ptr(reward), _lib.ptr(done)
        r.reward_f64 = 1 if (reward is not None and reward.dtype == torch.float64) else 0
        r.gamma = float(gamma)
        r.v, r.v64, r.td = _lib.ptr(v), _lib.ptr(v64), _lib.ptr(td)
        d = self._desc()
        _lib.check(self._lib.cm3_value_particle_rows_f32(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(r), self._stream(stream)))

    def v_rows(self, *cols, reward_local=None, done=None, gamma=None, keep=None):
        """The value network over the B * N agent rows r = b N + n of a batch, ONE launch.
          local network:   v_rows(obs_others [B, N, 4(N-1)], v_local [B, N, 4], goals [B, N, 2], ...)  (alg_baseline.py:525-527)
          global network:  v_rows(v_global [B, N, 4], goals [B, N, 2], ...): the row's own state and goal, the states and then the
                           goals of the other agents in ascending order (:530-533)
        (leading dimensions may be merged; float columns of any dtype are rounded to float32, as the reference's tf.float32
        placeholders do.)  reward_local, done and gamma may also be given in this order after the columns.  Returns a dict of device
        tensors: "v" float32 [R, 1], "v64" the same values float64 [R, 1], and with reward_local [B, N] (float32 / float64), done
        [B] and gamma also "td" float64 [R] = reward_local + gamma * v * (1 - done), the bits of batch.td_target on v64.  keep: an
        optional list that receives every tensor the launch touches, for whoever captures the launch."""
        what = "v_rows"
        n_cols = 3 if self.kind == "local" else 2
        if len(cols) < n_cols or len(cols) > n_cols + 3:
            raise Cm3Error("v_rows of a %s network takes %s and then reward_local, done, gamma"
                           % (self.kind, "obs_others, v_local, goals" if self.kind == "local" else "v_global, goals"))
        extra = cols[n_cols:] + (None, None, None)
        cols = cols[:n_cols]
        reward_local = extra[0] if reward_local is None else reward_local
        done = extra[1] if done is None else done
        gamma = extra[2] if gamma is None else gamma
        td = td_given(what, "reward_local", reward_local, done, gamma)
        N = self.n
        obs_others = cols[0] if self.kind == "local" else None
        state, goals = cols[-2], cols[-1]
        L = 4 * (N - 1)
        if (state.shape[-1] != 4 or goals.shape[-1] != 2 or state.numel() // 4 != goals.numel() // 2 or (state.numel() // 4) % N
                or state.numel() == 0 or (obs_others is not None and N > 1 and obs_others.numel() != state.numel() // 4 * L)):
            raise Cm3Error("%s takes %s[B, %d, 4] and goals [B, %d, 2], got %s"
                           % (what, "obs_others [B, %d, %d], " % (N, L) if self.kind == "local" else "", N, N,
                              ", ".join(str(tuple(c.shape)) for c in cols)))
        B = state.numel() // (4 * N)
        st, go = _f32(self.device, state, (B, N, 4)), _f32(self.device, goals, (B, N, 2))
        oo = _f32(self.device, obs_others, (B, N, L)) if (obs_others is not None and N > 1) else None
        _, rw, dn = stage_td_cols(what, self.device, B, N, None, reward_local, done, reward_name="reward_local")
        out = td_outputs(self.device, B * N, "v", td)
        _keep(keep, st, go, oo, rw, dn, *out.values())
        self.enqueue(B, st, go, oo, rw, dn, 0.0 if gamma is None else gamma, **out)
        return out


def _stage_checkers(device, t, narrow=False):
    """float64, contiguous on the device; narrow (grids and windows): an int8 column as it is"""
    return t.to(device=device, dtype=torch.int8 if (narrow and t.dtype == torch.int8) else torch.float64).contiguous()


def _stage_checkers_goals(device, goals, rows):
    """uint8 indices [rows] as they are; other indices and one-hot columns as int64 one-hot [rows, 2] (CheckersCritic._stage_cols)"""
    if goals.numel() == rows:
        if goals.dtype == torch.uint8:
            return goals.to(device).contiguous()
        return torch.nn.functional.one_hot(goals.to(device).long(), 2).contiguous()
    return goals.to(device=device, dtype=torch.int64).contiguous()


class CheckersValue(_DeviceNet):
    """networks.V_checkers_local (kind "local", IAC) / networks.V_checkers_global (kind "global") of alg_baseline_checkers.py on the
    device over the rows r = b N + n of a sampled Checkers batch, the twin of ParticleValue: ONE launch of
    cm3_value_checkers_rows_f32 on the base columns, no tiled feed.  Columns as CheckersCritic's: int8 grids / windows and uint8 index
    goals go in as they are, everything else is staged to float64 / int64 one-hot and rounded to float32 in the kernel.  Weights:
    ``self.w`` under the short names of CK_VALUE_NAMES[kind]."""
    _match = ("n", "kind", "stage")
    _refusal = "the main network must be a %(kind)s CheckersValue for %(n)d agents at stage %(stage)d"

    def __init__(self, weights, n_agents, kind="local", stage=2, device="cuda:0"):
        self.device = _lib.require_gpu(device)
        if kind not in VALUE_KINDS:
            raise Cm3Error("kind must be one of %s" % sorted(VALUE_KINDS))
        self.kind, self.n, self.stage = kind, int(n_agents), int(stage)
        if not 1 <= self.n <= CK_MAX_AGENTS:
            raise Cm3Error("n_agents must be in 1..%d" % CK_MAX_AGENTS)
        if self.stage not in (1, 2) or (self.stage == 1) != (self.n == 1):
            raise Cm3Error("V_checkers_%s runs at stage 1 with one agent and at stage 2 with more (n_agents %d, stage %d)"
                           % (kind, self.n, self.stage))
        self._load(weights, _V_PREFIXES, CK_VALUE_NAMES[kind], checkers_value_weight_shapes(self.n, kind, self.stage),
                   "Checkers value network", lambda lib: lib.cm3_value_checkers_packed_bytes(self.n, VALUE_KINDS[kind]),
                   _lib.ValueCheckersWeights())

    def _desc(self):
        d = _lib.ValueCheckersDesc()
        d.n_agents, d.stage, d.kind = self.n, self.stage, VALUE_KINDS[self.kind]
        d.n_h1_1, d.n_h1_2, d.n_h2 = CK_H1_1, CK_H1_2, CK_H2
        return d

    def repack(self):
        """Re-arrange the (possibly updated in place) TF-shaped weights into the rows kernel's layout, the convolution as a Toeplitz
        matrix: one launch."""
        d = self._desc()
        _lib.check(self._lib.cm3_value_checkers_pack(ctypes.byref(d), ctypes.byref(self._wt), self._packed.data_ptr(),
                                                     self._stream(None)))

    def enqueue(self, n_steps, goals, grid=None, vec=None, windows=None, obs_self_v=None, obs_others=None, reward=None, done=None,
                gamma=0.0, v=None, v64=None, td=None, stream=None):
        """Raw launch of cm3_value_checkers_rows_f32 on contiguous device tensors: grid / windows int8 or float64, vec / obs_self_v /
        obs_others float64, goals uint8 indices or int64 one-hot, reward float32 or float64, done uint8; every output is optional,
        one is required."""
        r = _lib.ValueCheckersRows()
        r.n_steps = int(n_steps)
        r.grid_f64 = 0 if (grid is not None and grid.dtype == torch.int8) else 1
        r.windows_f64 = 0 if (windows is not None and windows.dtype == torch.int8) else 1
        r.goals_onehot = 0 if goals.dtype == torch.uint8 else 1
        r.grid, r.vec, r.goals = _lib.ptr(grid), _lib.ptr(vec), _lib.ptr(goals)
        r.windows, r.obs_self_v, r.obs_others = _lib.ptr(windows), _lib.ptr(obs_self_v), _lib.ptr(obs_others)
        r.reward, r.done = _lib.ptr(reward), _lib.ptr(done)
        r.reward_f64 = 1 if (reward is not None and reward.dtype == torch.float64) else 0
        r.gamma = float(gamma)
        r.v, r.v64, r.td = _lib.ptr(v), _lib.ptr(v64), _lib.ptr(td)
        d = self._desc()
        _lib.check(self._lib.cm3_value_checkers_rows_f32(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(r), self._stream(stream)))

    def v_rows(self, *cols, reward_local=None, done=None, gamma=None, keep=None):
        """The value network over the B * N agent rows r = b N + n of a batch, ONE launch.
          local network:   v_rows(obs_self_t [B, N, 5, 5, 3], obs_self_v [B, N, 4], obs_others [B, N, 2(N-1)], goals, ...)
                           (the feed of alg_baseline_checkers.py:517-520)
          global network:  v_rows(grid [B, 3, 9, 2], vec [B, N, 4], goals, ...): the grid of step b, the row's own state and goal,
                           the states of the other agents in ascending order (:523-526)
        goals one-hot [B, N, 2] or indices [B, N]; leading dimensions may be merged.  reward_local, done and gamma may also be given
        in this order after the columns.  Returns what ParticleValue.v_rows returns: "v" float32 [R, 1], "v64" float64 [R, 1], and
        with reward_local [B, N], done [B] and gamma also "td" float64 [R], the bits of batch.td_target on v64.  keep: an optional
        list that receives every tensor the launch touches."""
        what = "v_rows"
        local = self.kind == "local"
        n_cols = 4 if local else 3
        if len(cols) < n_cols or len(cols) > n_cols + 3:
            raise Cm3Error("v_rows of a %s network takes %s and then reward_local, done, gamma"
                           % (self.kind, "obs_self_t, obs_self_v, obs_others, goals" if local else "grid, vec, goals"))
        extra = cols[n_cols:] + (None, None, None)
        cols = cols[:n_cols]
        reward_local = extra[0] if reward_local is None else reward_local
        done = extra[1] if done is None else done
        gamma = extra[2] if gamma is None else gamma
        td = td_given(what, "reward_local", reward_local, done, gamma)
        N = self.n
        goals = cols[-1]
        state = cols[1]                     # obs_self_v / vec: [B, N, 4] either way
        if state.shape[-1] != 4 or (state.numel() // 4) % N or state.numel() == 0:
            raise Cm3Error("%s takes %s [B, %d, 4], got %s" % (what, "obs_self_v" if local else "vec", N, tuple(state.shape)))
        B = state.numel() // (4 * N)
        Lo = 2 * (N - 1)
        if (goals.numel() not in (B * N, B * N * 2) or cols[0].numel() != (B * N * 75 if local else B * 54)
                or (local and N > 1 and cols[2].numel() != B * N * Lo)):
            raise Cm3Error("%s takes %s and goals [B, %d, 2] (or [B, %d]) for %d time steps, got %s"
                           % (what, "obs_self_t [B, %d, 5, 5, 3], obs_self_v [B, %d, 4], obs_others [B, %d, %d]" % (N, N, N, Lo) if local
                              else "grid [B, 3, 9, 2], vec [B, %d, 4]" % N, N, N, B, ", ".join(str(tuple(c.shape)) for c in cols)))
        go = _stage_checkers_goals(self.device, goals, B * N)
        st = _stage_checkers(self.device, state)
        first = _stage_checkers(self.device, cols[0], narrow=True)
        oo = _stage_checkers(self.device, cols[2]) if (local and N > 1) else None
        _, rw, dn = stage_td_cols(what, self.device, B, N, None, reward_local, done, reward_name="reward_local")
        out = td_outputs(self.device, B * N, "v", td)
        _keep(keep, first, st, go, oo, rw, dn, *out.values())
        g = 0.0 if gamma is None else gamma
        if local:
            self.enqueue(B, go, windows=first, obs_self_v=st, obs_others=oo, reward=rw, done=dn, gamma=g, **out)
        else:
            self.enqueue(B, go, grid=first, vec=st, reward=rw, done=dn, gamma=g, **out)
        return out


class CheckersComaCritic(_DeviceNet):
    """networks.Q_coma_checkers of alg_baseline_checkers.py on the device over the rows r = b N + n of a sampled Checkers batch, the
    twin of ParticleComaCritic: ONE launch of cm3_coma_checkers_rows_f32 on the base columns.  Weights: ``self.w`` under the short
    names of CK_COMA_NAMES."""
    _match = ("n",)
    _refusal = "the main critic must be a CheckersComaCritic for %(n)d agents"

    def __init__(self, weights, n_agents, device="cuda:0"):
        self.device = _lib.require_gpu(device)
        self.n = int(n_agents)
        if not 2 <= self.n <= CK_MAX_AGENTS:
            raise Cm3Error("n_agents must be in 2..%d: Q_coma_checkers exists with more than one agent only" % CK_MAX_AGENTS)
        self._load(weights, _Q_PREFIXES, CK_COMA_NAMES, checkers_coma_weight_shapes(self.n), "Checkers COMA critic",
                   lambda lib: lib.cm3_coma_checkers_packed_bytes(self.n), _lib.ComaCheckersWeights())

    def _desc(self):
        d = _lib.ComaCheckersDesc()
        d.n_agents, d.units = self.n, Q_UNITS
        return d

    def repack(self):
        """Re-arrange the (possibly updated in place) TF-shaped weights into the rows kernel's layout, the two convolutions as
        Toeplitz matrices: one launch."""
        d = self._desc()
        _lib.check(self._lib.cm3_coma_checkers_pack(ctypes.byref(d), ctypes.byref(self._wt), self._packed.data_ptr(),
                                                    self._stream(None)))

    def enqueue(self, n_steps, grid, vec, goals, windows, obs_self_v, actions, own_actions=None, reward=None, done=None, gamma=0.0,
                q=None, q_taken=None, q_taken64=None, td=None, stream=None):
        """Raw launch of cm3_coma_checkers_rows_f32 on contiguous device tensors: grid / windows int8 or float64, vec / obs_self_v
        float64, goals uint8 indices or int64 one-hot, actions / own_actions int32, reward [B] float32 or float64, done uint8; every
        output is optional, one is required."""
        r = _lib.ComaCheckersRows()
        r.n_steps = int(n_steps)
        r.grid_f64 = 0 if grid.dtype == torch.int8 else 1
        r.windows_f64 = 0 if windows.dtype == torch.int8 else 1
        r.goals_onehot = 0 if goals.dtype == torch.uint8 else 1
        r.grid, r.vec, r.goals = _lib.ptr(grid), _lib.ptr(vec), _lib.ptr(goals)
        r.actions, r.own_actions = _lib.ptr(actions), _lib.ptr(own_actions)
        r.windows, r.obs_self_v = _lib.ptr(windows), _lib.ptr(obs_self_v)
        r.reward, r.done = _lib.ptr(reward), _lib.ptr(done)
        r.reward_f64 = 1 if (reward is not None and reward.dtype == torch.float64) else 0
        r.gamma = float(gamma)
        r.q, r.q_taken, r.q_taken64, r.td = _lib.ptr(q), _lib.ptr(q_taken), _lib.ptr(q_taken64), _lib.ptr(td)
        d = self._desc()
        _lib.check(self._lib.cm3_coma_checkers_rows_f32(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(r), self._stream(stream)))

    def q_rows(self, grid, vec, goals, actions, obs_self_t, obs_self_v, reward=None, done=None, gamma=None, keep=None):
        """Q_coma_checkers over the B * N agent rows r = b N + n of a batch, ONE launch: the grid and the states of all agents of step
        b, the one-hot actions and the goals of the other agents in ascending order, the row's own goal, label, window and
        obs_self_v -- the feed of sess.run(Q_target) (alg_baseline_checkers.py:564-572) with the next-step columns and the target
        actor's samples, and of sess.run(Q) (:606-617) with this step's columns and the actions taken.  grid [B, 3, 9, 2], vec
        [B, N, 4], goals one-hot [B, N, 2] or indices [B, N], actions [B, N], obs_self_t [B, N, 5, 5, 3], obs_self_v [B, N, 4]
        (leading dimensions may be merged).  Returns what ParticleComaCritic.q_rows returns: "q" float32 [R, 5], "q_taken" float32
        [R, 1] = q[r, actions[b, n]] and "q_taken64" the same values float64; with reward [B] (the GLOBAL reward), done [B] and gamma
        also "td" float64 [R] = reward + gamma * q_taken * (1 - done) (:577), the bits of batch.td_target on q_taken64."""
        what = "q_rows"
        td = td_given(what, "reward", reward, done, gamma)
        N = self.n
        if actions is None:
            raise Cm3Error("%s needs actions" % what)
        if vec.shape[-1] != 4 or (vec.numel() // 4) % N or vec.numel() == 0:
            raise Cm3Error("%s takes vec [B, %d, 4], got %s" % (what, N, tuple(vec.shape)))
        B = vec.numel() // (4 * N)
        if (grid.numel() != B * 54 or obs_self_t.numel() != B * N * 75 or obs_self_v.numel() != B * N * 4
                or goals.numel() not in (B * N, B * N * 2)):
            raise Cm3Error("%s takes grid [B, 3, 9, 2], goals [B, %d, 2] (or [B, %d]), obs_self_t [B, %d, 5, 5, 3] and obs_self_v "
                           "[B, %d, 4] for %d time steps, got %s, %s, %s, %s"
                           % (what, N, N, N, N, B, tuple(grid.shape), tuple(goals.shape), tuple(obs_self_t.shape),
                              tuple(obs_self_v.shape)))
        if reward is not None and reward.numel() != B:
            raise Cm3Error("%s takes the global reward [B] for %d time steps, got %s" % (what, B, tuple(reward.shape)))
        gr, wi = (_stage_checkers(self.device, t, narrow=True) for t in (grid, obs_self_t))
        ve, ov = (_stage_checkers(self.device, t) for t in (vec, obs_self_v))
        go = _stage_checkers_goals(self.device, goals, B * N)
        ac, _, dn = stage_td_cols(what, self.device, B, N, actions, None, done)
        rw = None if reward is None else reward.reshape(-1).to(
            device=self.device, dtype=reward.dtype if reward.dtype == torch.float32 else torch.float64).contiguous()
        out = {"q": torch.empty(B * N, N_ACTIONS, dtype=torch.float32, device=self.device)}
        out.update(td_outputs(self.device, B * N, "q_taken", td))
        _keep(keep, gr, ve, go, wi, ov, ac, rw, dn, *out.values())
        self.enqueue(B, gr, ve, go, wi, ov, ac, ac, rw, dn, 0.0 if gamma is None else gamma, **out)
        return out


class ParticleComaCritic(_DeviceNet):
    _match = ("n",)
    _refusal = "the main critic must be a ParticleComaCritic for %(n)d agents"

    def __init__(self, weights, n_agents, device="cuda:0"):
        """networks.Q_global at Q_units = 256; more than one agent (the reference builds it under n_agents > 1).  float32 only."""
        self.device = _lib.require_gpu(device)
        self.n = int(n_agents)
        if not 2 <= self.n <= _lib.MAX_AGENTS:
            raise Cm3Error("n_agents must be in 2..%d: Q_global exists with more than one agent only" % _lib.MAX_AGENTS)
        self._load(weights, _Q_PREFIXES, COMA_NAMES, coma_weight_shapes(self.n), "COMA critic",
                   lambda lib: lib.cm3_coma_particle_packed_bytes(self.n), _lib.ComaParticleWeights())

    def _desc(self):
        d = _lib.ComaParticleDesc()
        d.n_agents, d.units = self.n, Q_UNITS
        return d

    def repack(self):
        """Re-arrange the (possibly updated in place) TF-shaped weights into the rows kernel's layout: one launch."""
        d = self._desc()
        _lib.check(self._lib.cm3_coma_particle_pack(ctypes.byref(d), ctypes.byref(self._wt), self._packed.data_ptr(),
                                                    self._stream(None)))

    def enqueue(self, n_steps, state, goals, v_obs, actions, own_actions=None, reward=None, done=None, gamma=0.0, q=None, q_taken=None,
                q_taken64=None, td=None, stream=None):
        """Raw launch of cm3_coma_particle_rows_f32 on contiguous device tensors: state / goals / v_obs float32, actions / own_actions
        int32, reward [B] float32 or float64, done uint8; every output is optional, one is required."""
        r = _lib.ComaRows()
        r.n_steps = int(n_steps)
        r.state, r.goals, r.v_obs = _lib.ptr(state), _lib.ptr(goals), _lib.ptr(v_obs)
        r.actions, r.own_actions = _lib.ptr(actions), _lib.ptr(own_actions)
        r.reward, r.done = _lib.ptr(reward), _lib.ptr(done)
        r.reward_f64 = 1 if (reward is not None and reward.dtype == torch.float64) else 0
        r.gamma = float(gamma)
        r.q, r.q_taken, r.q_taken64, r.td = _lib.ptr(q), _lib.ptr(q_taken), _lib.ptr(q_taken64), _lib.ptr(td)
        d = self._desc()
        _lib.check(self._lib.cm3_coma_particle_rows_f32(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(r), self._stream(stream)))

    def q_rows(self, v_global, goals, actions, v_local, reward=None, done=None, gamma=None, keep=None):
        """Q_global over the B * N agent rows r = b N + n of a batch, ONE launch: the state of all agents of step b, the one-hot
        actions and the goals of the other agents in ascending order, the row's own goal, label and v_obs -- the feed of
        sess.run(Q_target) (alg_baseline.py:570-576) with the next-step columns and the target actor's samples, and of sess.run(Q)
        (:608-616) with this step's columns and the actions taken.  v_global [B, N, 4], goals [B, N, 2], actions [B, N], v_local
        [B, N, 4] (leading dimensions may be merged).  Returns a dict of device tensors: "q" float32 [R, 5]; "q_taken" float32
        [R, 1] = q[r, actions[b, n]], what np.sum(Q * actions_self_1hot, axis=1) evaluates to (:577), and "q_taken64" the same values
        float64; with reward [B] (the GLOBAL reward, float32 / float64), done [B] and gamma also "td" float64 [R] = reward + gamma *
        q_taken * (1 - done) (:581), the bits of batch.td_target on q_taken64.  keep: as ParticleCritic's."""
        what = "q_rows"
        td = td_given(what, "reward", reward, done, gamma)
        N = self.n
        if actions is None:
            raise Cm3Error("%s needs actions" % what)
        if (v_global.shape[-1] != 4 or goals.shape[-1] != 2 or v_local.shape[-1] != 4 or v_global.numel() // 4 != goals.numel() // 2
                or v_local.numel() != v_global.numel() or (v_global.numel() // 4) % N or v_global.numel() == 0):
            raise Cm3Error("%s takes v_global [B, %d, 4], goals [B, %d, 2] and v_local [B, %d, 4], got %s, %s and %s"
                           % (what, N, N, N, tuple(v_global.shape), tuple(goals.shape), tuple(v_local.shape)))
        B = v_global.numel() // (4 * N)
        st, go, vo = (_f32(self.device, v_global, (B, N, 4)), _f32(self.device, goals, (B, N, 2)), _f32(self.device, v_local, (B, N, 4)))
        if reward is not None and reward.numel() != B:
            raise Cm3Error("%s takes the global reward [B] for %d time steps, got %s" % (what, B, tuple(reward.shape)))
        ac, _, dn = stage_td_cols(what, self.device, B, N, actions, None, done)
        rw = None if reward is None else reward.reshape(-1).to(
            device=self.device, dtype=reward.dtype if reward.dtype == torch.float32 else torch.float64).contiguous()
        out = {"q": torch.empty(B * N, N_ACTIONS, dtype=torch.float32, device=self.device)}
        out.update(td_outputs(self.device, B * N, "q_taken", td))
        _keep(keep, st, go, vo, ac, rw, dn, *out.values())
        self.enqueue(B, st, go, vo, ac, ac, rw, dn, 0.0 if gamma is None else gamma, **out)
        return out
