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
