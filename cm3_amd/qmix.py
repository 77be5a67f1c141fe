"""ParticleQmixAgent / CheckersQmixAgent -- the QMIX baseline's per-agent Q network and its epsilon-greedy choice, evaluated on
the device (CheckersQmixAgent: see its docstring).

    reference                                                    here
    ---------------------------------------------------------   -----------------------------------------
    networks.Qmix_single_particle(o_others, o_self, goal)        ParticleQmixAgent(weights, n_agents)
      (networks.py:581-594; variables Agent_main/{h,h2,out})       weights: dict keyed by the TF variable names
    argmax Q, else uniform with probability epsilon              agent.act(env, epsilon) -> actions [E, N]
      (alg_qmix.py:98, run_actor :160-184)                         (one launch: forward + argmax + exploration)
    alg.run_actor(local_others, local_self, goals, eps, sess)    ParticleRollout.collect(policy=agent, epsilon=..)
      (called at train_offpolicy.py:319)                           agent and step launches alternate inside ONE
                                                                   hipGraph; nothing returns to the host

Weights are float32 [in][out] as TensorFlow shapes them; an "Agent_main/" or "Agent_target/" prefix and a ":0" suffix are
ignored, so ``{v.name: sess.run(v)}`` of either scope loads unchanged.  The network is float32 on float32 and float64 envs alike
(a float64 env's observation is rounded to float32 as the inputs are staged, as the reference's tf.float32 placeholders do).

Exploration draws come from the build's own Philox stream (csrc/actor.hip, kPurposeExplore): the same law as the reference's
np.random calls, not the same numbers.  Both agents serve a
learner's data side with greedy_rows (argmax_Q_target on the rows of a sampled batch) and soft_update_from, and ParticleQmixMixer /
CheckersQmixMixer (below) evaluate the target mixer -- mixer_target and the TD target -- on the same rows; ParticleQmixLearner and
CheckersQmixLearner (at the end) are the learners themselves: loss, gradients and Adam on the device.  soft_update_from and the
weight loading are cm3_amd._net._DeviceNet's (the agent and mixer halves of list_update_target_ops, alg_qmix.py:135-156,
alg_qmix_checkers.py:128-130); CheckersQmixAgent shares descriptor and launch bodies with CheckersActor (actor._CheckersPolicyNet).
"""
import ctypes

import torch

from . import _lib
from ._lib import Cm3Error
from ._net import _DeviceNet, _keep, canon, greedy_outputs, stage_particle_rows, stage_td_cols, td_given, td_outputs
from .actor import _CheckersPolicyNet, _epsilon_args, checkers_policy_shapes, stage_checkers_rows

H, N_ACTIONS = 64, 5
# the six tensors of cm3_qmix_particle_pack, in its order
NAMES = ("h/kernel", "h/bias", "h2/kernel", "h2/bias", "out/kernel", "out/bias")


_PREFIXES = ("Agent_main/", "Agent_target/")


def _canon(name):
    return canon(name, _PREFIXES)


class ParticleQmixAgent(_DeviceNet):
    """episode_kernel=True opts this agent in to the one-launch rollout (cm3_policy_rollout_qmix_f32: the network, the epsilon-greedy
    choice and the env step of every tick in ONE launch, the same bits as the launch pairs): ParticleRollout then runs it under
    policy_mode "episode" and, where it is eligible and measured faster, "auto" (episode_ok / episode_refusal / enqueue_episode
    below).  The default agent runs as launch pairs in every mode, exactly as before."""
    # ParticleRollout's fused=True / fused_policy_tick=True kernels run the CM3 actor, and so does policy_mode="episode" unless the
    # agent was built with episode_kernel=True
    fused_kernels = False
    EPISODE_AGENTS = (1, 2, 4, 8)        # whole envs per 16-row wave tile
    _refusal = "the main agent must be a ParticleQmixAgent for %(n)d agents"

    def __init__(self, weights, n_agents, device="cuda:0", seed=12341, env_id_base=0, episode_kernel=False):
        self.episode_kernel = bool(episode_kernel)
        self.device = _lib.require_gpu(device)
        self.n = int(n_agents)
        if not 1 <= self.n <= _lib.MAX_AGENTS:
            raise Cm3Error("n_agents must be in 1..%d" % _lib.MAX_AGENTS)
        self.L = 4 * max(self.n - 1, 1)
        self.seed = int(seed)
        self.env_id_base = int(env_id_base)
        shapes = {"h/kernel": (self.L + 6, H), "h/bias": (H,), "h2/kernel": (H, H), "h2/bias": (H,),
                  "out/kernel": (H, N_ACTIONS), "out/bias": (N_ACTIONS,)}
        # (no weights struct: cm3_qmix_particle_pack takes the six pointers in the order of NAMES, the launches the packed pointer)
        self._load(weights, _PREFIXES, {k: k for k in NAMES}, shapes, "QMIX", lambda lib: lib.cm3_qmix_particle_packed_bytes(self.n))

    def repack(self):
        """Re-arrange the (possibly updated in place) TF-shaped weights into the forward kernel's layout: after every update."""
        d = self._desc(1, 0.0, 0)
        _lib.check(self._lib.cm3_qmix_particle_pack(ctypes.byref(d), self._tensors, self._packed.data_ptr(),
                                                    self._stream(None)))

    def _desc(self, n_envs, epsilon, env_id_base):
        d = _lib.ActorParticleDesc()
        d.n_envs, d.n_agents, d.stage = int(n_envs), self.n, 2
        d.n_h1_self, d.n_h1_others, d.n_h2, d.n_actions = H, 0, H, N_ACTIONS
        d.epsilon = float(epsilon)
        d.precision = 0
        d.env_id_base = int(env_id_base)
        d.seed = self.seed & 0xFFFFFFFFFFFFFFFF
        return d

    def enqueue(self, n_envs, obs_others, state, goals, meta, episode, actions, epsilon, probs=None, stream=None,
                env_id_base=None, dtype=torch.float32):
        """Raw launch on device tensors, the signature of ParticleActor.enqueue; dtype: the real of obs_others / state / goals
        (cm3_qmix_particle_f32 / _f64).  actions int32 [E, N]; probs (optional) receives the Q values float32 [E, N, 5]."""
        if dtype == torch.float32:
            fn = self._lib.cm3_qmix_particle_f32
        elif dtype == torch.float64:
            fn = self._lib.cm3_qmix_particle_f64
        else:
            raise Cm3Error("the QMIX agent reads float32 or float64 env buffers, not %s" % (dtype,))
        b = _lib.ActorParticleBufs()
        b.obs_others, b.state, b.goals = _lib.ptr(obs_others), _lib.ptr(state), _lib.ptr(goals)
        b.meta, b.episode, b.actions, b.probs = _lib.ptr(meta), _lib.ptr(episode), _lib.ptr(actions), _lib.ptr(probs)
        epsilon, b.epsilon_dev = _epsilon_args(epsilon)
        d = self._desc(n_envs, epsilon, self.env_id_base if env_id_base is None else env_id_base)
        s = self._stream(stream)
        _lib.check(fn(ctypes.byref(d), self._packed.data_ptr(), ctypes.byref(b), s))

    def act(self, env, epsilon, return_q=False):
        """Actions [E, N] int32 for the env's CURRENT observation (alg_qmix.run_actor); optionally the Q values [E, N, 5]
        (float32).  float32 and float64 envs alike."""
        if env.n != self.n:
            raise Cm3Error("QMIX agent built for %d agents, env has %d" % (self.n, env.n))
        cur = env._cur
        actions = torch.empty(env.E, env.n, dtype=torch.int32, device=self.device)
        q = torch.empty(env.E, env.n, N_ACTIONS, dtype=torch.float32, device=self.device) if return_q else None
        self.enqueue(env.E, env._obs_others[cur], env._state[cur], env._goals, env._meta, env._episode, actions,
                     epsilon, q, env_id_base=env.env_id_base, dtype=env.dtype)
        return (actions, q) if return_q else actions

    def episode_refusal(self, env):
        """Why cm3_policy_rollout_qmix_f32 does not run this agent on `env` -- the first failed condition, in words -- or None when it
        does: a float32 env, n_agents in {1, 2, 4, 8}, the agent's count equal to the env's, agent and env on one seed (one Philox
        key; the env's env_id_base is passed on by the launch)."""
        if env.dtype != torch.float32:
            return ("float32 env: the one-launch QMIX rollout has no float64 build; this env is %s and runs as launch pairs "
                    "(policy_mode='tick')" % (env.dtype,))
        if env.n not in self.EPISODE_AGENTS:
            return ("agent count: the one-launch QMIX rollout covers n_agents in {1, 2, 4, 8} (whole envs per 16-row wave tile); the "
                    "env has %d -- other counts run as launch pairs (policy_mode='tick')" % env.n)
        if env.n != self.n:
            return "agent count: QMIX agent built for %d agents, env has %d" % (self.n, env.n)
        if (self.seed & 0xFFFFFFFFFFFFFFFF) != (int(env.seed) & 0xFFFFFFFFFFFFFFFF):
            return ("seed: the one-launch QMIX rollout draws for agent and env under one Philox key; the agent has seed %d, the env "
                    "seed %d" % (self.seed, int(env.seed)))
        return None

    def episode_ok(self, env):
        """cm3_policy_rollout_qmix_f32 applies to this agent on `env` (see episode_refusal)."""
        return self.episode_refusal(env) is None

    def enqueue_episode(self, env_desc, traj, n_envs, n_ticks, epsilon, q_values=None, stream=None):
        """The whole agent-driven rollout in ONE launch (cm3_policy_rollout_qmix_f32) on a float32 env's descriptor and a
        cm3_particle_traj; q_values: optional float32 [T, E, N, 5], receives the raw Q values of every tick.  epsilon: a float, or a
        float32 device tensor of one element that the launch reads itself."""
        epsilon, eps_dev = _epsilon_args(epsilon)
        d = self._desc(n_envs, epsilon, env_desc.env_id_base)
        s = self._stream(stream)
        _lib.check(self._lib.cm3_policy_rollout_qmix_f32(
            ctypes.byref(env_desc), ctypes.byref(traj), ctypes.byref(d), self._packed.data_ptr(), _lib.ptr(q_values),
            0 if q_values is None else q_values[0].numel() * q_values.element_size(), eps_dev, int(n_ticks), s))

    def greedy_rows(self, obs_others, v_obs, goals, q=False, onehot=True, q_max=False):
        """The network over transition rows with a pure argmax head, ONE launch (cm3_qmix_particle_rows_f32): with the Agent_target
        weights this is argmax_Q_target of alg_qmix.train_step (alg_qmix.py:349-356) on the columns obs_others_next / v_local_next /
        goals of a sampled batch.  Inputs: float tensors [..., L], [..., 4], [..., 2] with equal leading shape, made contiguous
        float32 (a float64 column is rounded, as the reference's tf.float32 placeholders do).  Returns a dict of device tensors over
        the R = prod(leading shape) rows: "argmax" int32 [R] always; "q" float32 [R, 5], "onehot" int64 [R, 5] (the reference's
        actions_target_1hot), "q_max" float32 [R] when asked for.  A row's Q values are the bits act() computes for the same
        inputs."""
        rows, oo, vo, vg = stage_particle_rows("greedy_rows", self.device, self.L, obs_others, v_obs, goals)
        out = greedy_outputs(self.device, rows, q, onehot, q_max)
        self.enqueue_rows(rows, oo, vo, vg, **out)
        return out

    def enqueue_rows(self, n_rows, obs_others, v_obs, goals, q=None, argmax=None, onehot=None, q_max=None, stream=None):
        """Raw launch of cm3_qmix_particle_rows_f32 on contiguous float32 device tensors; every output is optional, one is required."""
        r = _lib.QmixRows()
        r.obs_others, r.v_obs, r.goals = _lib.ptr(obs_others), _lib.ptr(v_obs), _lib.ptr(goals)
        r.q, r.argmax, r.onehot, r.q_max = _lib.ptr(q), _lib.ptr(argmax), _lib.ptr(onehot), _lib.ptr(q_max)
        r.n_rows = int(n_rows)
        d = self._desc(1, 0.0, 0)
        s = self._stream(stream)
        _lib.check(self._lib.cm3_qmix_particle_rows_f32(ctypes.byref(d), self._packed.data_ptr(), ctypes.byref(r), s))


# ---- Checkers -------------------------------------------------------------------------------------------------------------------
# the thirteen variables of networks.Qmix_single_checkers (networks.py:617-637) by the fields of cm3_actor_checkers_weights
CK_NAMES = {
    "conv_w": "conv/Conv/weights", "conv_b": "conv/Conv/biases", "lin_w": "conv_linear/kernel", "lin_b": "conv_linear/bias",
    "self_w": "branch_self/kernel", "self_b": "branch_self/bias", "w_self_h2": "W_self_h2",
    "others_w": "branch_others/kernel", "others_b": "branch_others/bias", "w_others_h2": "W_others_h2", "b_h2": "b",
    "out_w": "Qmix_single_out/kernel", "out_b": "Qmix_single_out/bias"}
CK_PRECISIONS = {"f32": 0, "f16x3": 2}       # cm3_actor_checkers_desc.precision (bf16 is refused: argmax would flip)


class CheckersQmixAgent(_CheckersPolicyNet):
    """The QMIX baseline's Checkers agent network and its epsilon-greedy choice, evaluated on the device.

        reference                                                        here
        -------------------------------------------------------------   ----------------------------------------
        networks.Qmix_single_checkers(a_prev, t_obs_self, v_obs_self,    CheckersQmixAgent(weights, n_agents)
            v_obs_others, v_goal, f1=6, k1=[3,3], n_h1=256, n_h2=256)      weights: dict keyed by the TF variable names
            (networks.py:617-637; variables Agent_main/...)
        argmax Q, else uniform with probability epsilon                  agent.act(env, epsilon, actions_prev)
            (alg_qmix_checkers.py:90, run_actor :153-182)                  -> actions [E, N] (one launch)
        alg.run_actor(actions_prev, obs_others, obs_self_t, obs_self_v,  CheckersRollout.collect(goals, policy=agent,
            goals, eps, sess)  (train_offpolicy.py:316-317)                epsilon=..): agent and step launches alternate
                                                                           inside ONE hipGraph; with
                                                                           CheckersRollout(env, policy_mode="episode") the
                                                                           whole rollout is ONE launch

    The network is the CM3 Checkers actor's forward pass (csrc/actor_checkers.hip) with the others branch at every agent count
    and a greedy head.  precision: "f32" (every layer on the exact-f32 MFMA) or "f16x3" (every layer in split float16, the
    actor's precision 2).  Exploration draws come from the particle QMIX agent's stream (keyed with the Checkers env's episode
    and step counters).

    CheckersRollout runs this agent as launch pairs under policy_mode "auto" and "tick".  policy_mode="episode" opts in to the
    one-launch rollout kernel (cm3_policy_rollout_checkers_qmix; enqueue_episode / episode_ok below): "f16x3", one or two agents,
    agent and env on one seed and env_id_base -- the same bits as the launch pairs.  (The hooks are NOT named like CheckersActor's
    enqueue_rollout / fused_rollout_ok: "auto" picks the one-launch kernel for whatever carries those names.)

    For a learner: greedy_rows evaluates the network on the rows of a sampled batch (argmax_Q_target of the reference's train_step,
    one launch, no draws), soft_update_from moves an Agent_target copy towards the main agent; cm3_amd.batch.qmix_train_step_feeds(
    env="checkers", target_agent=...) builds every feed of train_step around them; with target_mixer= (a CheckersQmixMixer, below) the
    target mixer's forward pass runs on the device too; with learner= (a CheckersQmixLearner, at the end of this module) the optimiser
    step of mixer_op as well.
    """
    _match = ("n", "precision")
    _refusal = "the main agent must be a CheckersQmixAgent for %(n)d agents at precision %(precision)r"

    def __init__(self, weights, n_agents, device="cuda:0", seed=12341, env_id_base=0, precision="f32"):
        if precision not in CK_PRECISIONS:
            raise Cm3Error("precision must be one of %s (bf16 is not a parity path: argmax would flip)" % sorted(CK_PRECISIONS))
        self.device = _lib.require_gpu(device)
        self.precision = precision
        self.n = int(n_agents)
        if not 1 <= self.n <= 8:
            raise Cm3Error("the Checkers QMIX agent supports 1..8 agents")
        self.Lo = 2 * max(self.n - 1, 1)
        self.seed = int(seed)
        self.env_id_base = int(env_id_base)
        self._load(weights, _PREFIXES, CK_NAMES, checkers_policy_shapes(self.Lo), "QMIX",
                   lambda lib: lib.cm3_actor_checkers_packed_bytes(), _lib.ActorCheckersWeights())

    def repack(self):
        """Re-arrange the (possibly updated in place) TF-shaped weights into the forward kernel's layout: after every update."""
        d = self._desc(1, 0.0, 0, 75 * self.n)
        _lib.check(self._lib.cm3_qmix_checkers_pack(ctypes.byref(d), ctypes.byref(self._wt), self._packed.data_ptr(),
                                                    self._stream(None)))

    def enqueue(self, n_envs, obs_self_t_raw, obst_stride, obs_self_v, obs_others, goals, actions_prev, steps, episode,
                actions, epsilon, probs=None, stream=None, env_id_base=None, prev_done=None):
        """Raw launch on the env's device buffers, the signature of CheckersActor.enqueue.  probs (optional) receives the Q
        values float32 [E, N, 5]."""
        self._enqueue_tick(self._lib.cm3_qmix_checkers_f32, n_envs, obs_self_t_raw, obst_stride, obs_self_v, obs_others, goals,
                           actions_prev, steps, episode, actions, epsilon, probs, stream, env_id_base, prev_done)

    def enqueue_episode(self, env_desc, traj, n_envs, obst_stride, n_ticks, epsilon, prev0=None, probs=None, stream=None,
                        final_obs=None, prev0_next=None):
        """The whole agent-driven rollout in ONE launch (cm3_policy_rollout_checkers_qmix), the signature of
        CheckersActor.enqueue_rollout; probs: optional float32 [T, E, N, 5], receives the Q values."""
        self._enqueue_whole(self._lib.cm3_policy_rollout_checkers_qmix, env_desc, traj, n_envs, obst_stride, n_ticks, epsilon, prev0,
                            probs, stream, final_obs, prev0_next)

    def episode_ok(self, env):
        """cm3_policy_rollout_checkers_qmix applies: split float16, one or two agents (the env's count), the 3 x 8 band with
        n_obs 2 and 4-byte padded records, agent and env on one seed and env_id_base (one Philox key)."""
        same_key = (self.seed & 0xFFFFFFFFFFFFFFFF) == int(env._desc.seed) and self.env_id_base == int(env._desc.env_id_base)
        return (self.precision == "f16x3" and same_key and env.n == self.n and env.n in (1, 2) and env.K == 5 and env.R == 3
                and env.C == 8 and env.grid_stride % 4 == 0 and env.obst_stride % 4 == 0)

    def act(self, env, epsilon, actions_prev=None, return_q=False):
        """Actions [E, N] int32 for the env's CURRENT observation (alg_qmix_checkers.run_actor); actions_prev None = zeros
        (train_offpolicy.py:300); optionally the Q values [E, N, 5] (float32)."""
        if env.n != self.n:
            raise Cm3Error("QMIX agent built for %d agents, env has %d" % (self.n, env.n))
        if env.K != 5:
            raise Cm3Error("the device agent reads 5x5 windows (n_obs = 2)")
        s = env._slots[env._cur]
        prev = None
        if actions_prev is not None:
            prev = torch.as_tensor(actions_prev, device=self.device).to(torch.int32).reshape(env.E, env.n).contiguous()
        actions = torch.empty(env.E, env.n, dtype=torch.int32, device=self.device)
        q = torch.empty(env.E, env.n, N_ACTIONS, dtype=torch.float32, device=self.device) if return_q else None
        self.enqueue(env.E, s["obs_self_t_raw"], env.obst_stride, s["obs_self_v"], s["obs_others"], env._goals, prev,
                     env._steps, env._episode, actions, epsilon, q, env_id_base=env._desc.env_id_base)
        return (actions, q) if return_q else actions

    def greedy_rows(self, obs_self_t, obs_self_v, obs_others, actions_prev, goals, q=False, onehot=True, q_max=False):
        """The network over transition rows with a pure argmax head, ONE launch (cm3_qmix_checkers_rows_f32): with the Agent_target
        weights this is argmax_Q_target of alg_qmix_checkers.train_step (alg_qmix_checkers.py:353-359) on the columns
        next_obs_self_t / next_obs_self_v / next_obs_others / actions / goals of a sampled batch (the reference feeds the action just
        taken as actions_prev next to the next observation).  Inputs share a leading shape [...]: obs_self_t [..., 5, 5, 3] or
        [..., 75]; obs_self_v [..., 4]; obs_others [..., Lo]; actions_prev [...] (0..4); goals a one-hot [..., 2] or an index [...].
        The form follows from the dtype: int8 windows and uint8 index goals go in as they are (what the trajectory and the compact
        ring keep); everything else is made float64 windows / int64 one-hot goals (no copy for the columns sample_batch returns).
        At precision "f16x3" float64 windows must hold float16-exact values (the env's are -1 / 0 / 1): the window plane is one
        float16 plane, as in the collection kernel.  Returns a dict of device tensors over the R = prod(leading shape) rows:
        "argmax" int32 [R] always; "q" float32 [R, 5], "onehot" int64 [R, 5] (the reference's actions_target_1hot), "q_max" float32
        [R] when asked for.  A row's Q values are the bits act() computes for the same inputs at the same precision."""
        rows, ot, ov, oo, ap, vg = stage_checkers_rows("greedy_rows", self.device, self.Lo, obs_self_t, obs_self_v, obs_others,
                                                       actions_prev, goals)
        out = greedy_outputs(self.device, rows, q, onehot, q_max)
        self.enqueue_rows(rows, ot, ov, oo, ap, vg, **out)
        return out

    def enqueue_rows(self, n_rows, obs_self_t, obs_self_v, obs_others, actions_prev, goals, q=None, argmax=None, onehot=None,
                     q_max=None, stream=None):
        """Raw launch of cm3_qmix_checkers_rows_f32 on contiguous device tensors: obs_self_t int8 or float64 [R, 75], obs_self_v /
        obs_others float64, actions_prev int32 [R], goals uint8 [R] or int64 [R, 2]; every output is optional, one is required."""
        if obs_self_t.dtype not in (torch.int8, torch.float64) or goals.dtype not in (torch.uint8, torch.int64):
            raise Cm3Error("enqueue_rows reads int8 or float64 windows and uint8 index or int64 one-hot goals, not %s / %s"
                           % (obs_self_t.dtype, goals.dtype))
        r = _lib.QmixCheckersRows()
        r.obs_self_t, r.obs_self_v, r.obs_others = _lib.ptr(obs_self_t), _lib.ptr(obs_self_v), _lib.ptr(obs_others)
        r.actions_prev, r.goals = _lib.ptr(actions_prev), _lib.ptr(goals)
        r.obs_self_t_f64 = 1 if obs_self_t.dtype == torch.float64 else 0
        r.goals_onehot = 1 if goals.dtype == torch.int64 else 0
        r.q, r.argmax, r.onehot, r.q_max = _lib.ptr(q), _lib.ptr(argmax), _lib.ptr(onehot), _lib.ptr(q_max)
        r.n_rows = int(n_rows)
        d = self._desc(1, 0.0, 0, 75 * self.n)
        s = self._stream(stream)
        _lib.check(self._lib.cm3_qmix_checkers_rows_f32(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(r), s))


# ---- the particle mixer ---------------------------------------------------------------------------------------------------------------
EMBED = 64                                          # embed_dim of networks.Qmix_mixer
# the five variables of networks.Qmix_mixer (networks.py:657-665) by the fields of cm3_qmix_mixer_particle_weights
MIXER_NAMES = {"w1": "hyper_w_1", "w_final": "hyper_w_final", "b1": "hyper_b_1", "b_final_l1": "hyper_b_final_l1/kernel",
               "b_final": "hyper_b_final/kernel"}
_MIXER_FIELDS = {"w1": "hyper_w_1", "w_final": "hyper_w_final", "b1": "hyper_b_1", "b_final_l1": "hyper_b_final_l1",
                 "b_final": "hyper_b_final"}
_MIXER_PREFIXES = ("Mixer_main/", "Mixer_target/")


def _mixer_canon(name):
    return canon(name, _MIXER_PREFIXES)


def mixer_weight_shapes(n_agents):
    """short name -> shape of the TF variable of networks.Qmix_mixer for this agent count"""
    k = 6 * n_agents
    return {"w1": (k, EMBED * n_agents), "w_final": (k, EMBED), "b1": (k, EMBED), "b_final_l1": (k, EMBED), "b_final": (EMBED, 1)}


class ParticleQmixMixer(_DeviceNet):
    """The reference's particle QMIX mixer evaluated on the device over the transitions of a sampled batch.

        reference                                                    here
        ---------------------------------------------------------   -----------------------------------------------
        networks.Qmix_mixer(agent_qs, state, goals_all, ...)         ParticleQmixMixer(weights, n_agents)
          (networks.py:640-685; scopes Mixer_main / Mixer_target)
        sess.run(mixer_target, feed) + the TD target                 mixer.q_tot(v_global_next, goals, q_max, reward_local, done, gamma)
          (alg_qmix.py:358-369)                                        (ONE launch of cm3_qmix_mixer_particle_rows_f32)
        the mixer half of list_update_target_ops (:139-156)          mixer.soft_update_from(main_mixer, tau)

    The forward pass only: the main mixer's loss, gradient and optimiser step are ParticleQmixLearner's (below), or a session's.  Weights stay
    float32 [in][out] as TensorFlow shapes them, in ``self.w`` under the short names of MIXER_NAMES, so a session that trains the
    main mixer can write updated variables INTO these tensors in place; ``repack()`` (one launch on persistent tensors, capturable)
    then makes the next launch follow them.  The prefixes "Mixer_main/", "Mixer_target/" and a ":0" suffix of the keys are ignored."""
    _refusal = "the main mixer must be a ParticleQmixMixer for %(n)d agents"

    def __init__(self, weights, n_agents, device="cuda:0"):
        self.device = _lib.require_gpu(device)
        self.n = int(n_agents)
        if not 1 <= self.n <= _lib.MAX_AGENTS:
            raise Cm3Error("n_agents must be in 1..%d" % _lib.MAX_AGENTS)
        self._load(weights, _MIXER_PREFIXES, MIXER_NAMES, mixer_weight_shapes(self.n), "mixer",
                   lambda lib: lib.cm3_qmix_mixer_particle_packed_bytes(self.n), _lib.QmixMixerParticleWeights(), _MIXER_FIELDS)

    def _desc(self):
        d = _lib.QmixMixerParticleDesc()
        d.n_agents, d.embed_dim = self.n, EMBED
        return d

    def repack(self):
        """Re-arrange the (possibly updated in place) TF-shaped weights into the rows kernel's layout: one launch."""
        d = self._desc()
        _lib.check(self._lib.cm3_qmix_mixer_particle_pack(ctypes.byref(d), ctypes.byref(self._wt), self._packed.data_ptr(),
                                                          self._stream(None)))

    # ---- launches -------------------------------------------------------------------------------------------------------------------
    def enqueue(self, n_steps, state, goals, agent_qs, reward=None, done=None, gamma=0.0, q_tot=None, q_tot64=None, td=None,
                stream=None):
        """Raw launch of cm3_qmix_mixer_particle_rows_f32 on contiguous device tensors: state / goals / agent_qs float32, reward
        float32 or float64, done uint8; every output is optional, one is required."""
        r = _lib.QmixMixerRows()
        r.n_steps = int(n_steps)
        r.state, r.goals, r.agent_qs = _lib.ptr(state), _lib.ptr(goals), _lib.ptr(agent_qs)
        r.reward, r.done = _lib.ptr(reward), _lib.ptr(done)
        r.reward_f64 = 1 if (reward is not None and reward.dtype == torch.float64) else 0
        r.gamma = float(gamma)
        r.q_tot, r.q_tot64, r.td = _lib.ptr(q_tot), _lib.ptr(q_tot64), _lib.ptr(td)
        d = self._desc()
        s = self._stream(stream)
        _lib.check(self._lib.cm3_qmix_mixer_particle_rows_f32(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(r), s))

    def _stage_cols(self, what, state, goals, agent_qs, reward=None, done=None):
        """(B, state, goals, agent_qs, reward, done) contiguous on the mixer's device from [B, N, 4], [B, N, 2], [B, N], [B, N] and
        [B] (leading dimensions may be merged or flattened: [B, 4 N], [B * N] ...), staged as ParticleCritic._stage_cols stages them:
        float columns of any dtype are rounded to float32, as the reference's tf.float32 placeholders do; reward stays float32 or
        float64 (another dtype is widened to float64); bool or integer done becomes uint8."""
        N = self.n
        if state.numel() == 0 or state.numel() % (4 * N) or goals.numel() * 2 != state.numel():
            raise Cm3Error("%s takes state [B, %d, 4] and goals [B, %d, 2], got %s and %s"
                           % (what, N, N, tuple(state.shape), tuple(goals.shape)))
        B = state.numel() // (4 * N)
        f32 = lambda t: t.to(device=self.device, dtype=torch.float32).contiguous()      # noqa: E731
        state, goals = f32(state).reshape(B, N, 4), f32(goals).reshape(B, N, 2)
        if agent_qs.numel() != B * N:
            raise Cm3Error("%s takes agent_qs [B, %d] for %d time steps, got %s" % (what, N, B, tuple(agent_qs.shape)))
        agent_qs = f32(agent_qs).reshape(B, N)
        _, reward, done = stage_td_cols(what, self.device, B, N, None, reward, done, reward_name="reward_local")
        return B, state, goals, agent_qs, reward, done

    def q_tot(self, state, goals, agent_qs, reward_local=None, done=None, gamma=None, keep=None):
        """Qmix_mixer over the B transitions of a batch, ONE launch: state = v_global_next [B, N, 4], goals [B, N, 2] and agent_qs
        [B, N] = each target agent's Q at its argmax (greedy_rows(..., q_max=True)) give sess.run(mixer_target) of
        alg_qmix.train_step (alg_qmix.py:358-365).  Returns a dict of device tensors: "q_tot" float32 [B, 1] (the shape the session
        returns), "q_tot64" the same values float64 [B, 1], and with reward_local [B, N] (float32 / float64), done [B] and gamma also
        "td" float64 [B] = sum(reward_local[b]) + gamma * q_tot * (1 - done), the bits of batch.qmix_td_target on "q_tot".  The three
        come together or not at all.  keep: an optional list that receives every tensor the launch touches (the staged inputs, the
        outputs), for whoever captures the launch."""
        td = td_given("q_tot", "reward_local", reward_local, done, gamma)
        B, st, go, aq, rw, dn = self._stage_cols("q_tot", state, goals, agent_qs, reward_local, done)
        out = td_outputs(self.device, B, "q_tot", td)
        _keep(keep, st, go, aq, rw, dn, *out.values())
        self.enqueue(B, st, go, aq, rw, dn, 0.0 if gamma is None else gamma, **out)
        return out


# ---- the Checkers mixer ---------------------------------------------------------------------------------------------------------------
CK_EMBED = 128                                      # embed_dim of networks.Qmix_mixer_checkers
# the seven variables of networks.Qmix_mixer_checkers (networks.py:697-714) by the fields of cm3_qmix_mixer_checkers_weights
CK_MIXER_NAMES = {"conv_w": "conv/Conv/weights", "conv_b": "conv/Conv/biases", "hyper_w_1": "hyper_w_1", "hyper_w_final": "hyper_w_final",
                  "hyper_b_1": "hyper_b_1", "hyper_b_final_l1": "hyper_b_final_l1/kernel", "hyper_b_final": "hyper_b_final/kernel"}


def checkers_mixer_weight_shapes(n_agents):
    """short name -> shape of the TF variable of networks.Qmix_mixer_checkers for this agent count (Q_conv_f 4, Q_conv_k [3, 5])"""
    k = 108 + 6 * n_agents
    return {"conv_w": (3, 5, 2, 4), "conv_b": (4,), "hyper_w_1": (k, CK_EMBED * n_agents), "hyper_w_final": (k, CK_EMBED),
            "hyper_b_1": (k, CK_EMBED), "hyper_b_final_l1": (k, CK_EMBED), "hyper_b_final": (CK_EMBED, 1)}


class CheckersQmixMixer(_DeviceNet):
    """The reference's Checkers QMIX mixer evaluated on the device over the transitions of a sampled batch.

        reference                                                        here
        -------------------------------------------------------------   -----------------------------------------------
        networks.Qmix_mixer_checkers(agent_qs, state_env, state,         CheckersQmixMixer(weights, n_agents)
            goals_all, ..., f1=4, k1=[3,5])
          (networks.py:688-734; scopes Mixer_main / Mixer_target)
        sess.run(mixer_target, feed) + the TD target                     mixer.q_tot(next_grid, next_vec, goals, q_max, local_rewards,
          (alg_qmix_checkers.py:364-379)                                   done, gamma)  (ONE launch of cm3_qmix_mixer_checkers_rows_f32)
        the mixer half of list_update_target_ops (:128-130)              mixer.soft_update_from(main_mixer, tau)

    The forward pass only: the main mixer's loss, gradient and optimiser step are CheckersQmixLearner's (below), or a session's.  Weights stay
    float32 as TensorFlow shapes them, in ``self.w`` under the short names of CK_MIXER_NAMES, so a session that trains the main mixer
    can write updated variables INTO these tensors in place; ``repack()`` (one launch on persistent tensors, capturable) then makes
    the next launch follow them.  The prefixes "Mixer_main/", "Mixer_target/" and a ":0" suffix of the keys are ignored."""
    _refusal = "the main mixer must be a CheckersQmixMixer for %(n)d agents"

    def __init__(self, weights, n_agents, device="cuda:0"):
        self.device = _lib.require_gpu(device)
        self.n = int(n_agents)
        if not 1 <= self.n <= 8:
            raise Cm3Error("the Checkers QMIX mixer supports 1..8 agents")
        self._load(weights, _MIXER_PREFIXES, CK_MIXER_NAMES, checkers_mixer_weight_shapes(self.n), "mixer",
                   lambda lib: lib.cm3_qmix_mixer_checkers_packed_bytes(self.n), _lib.QmixMixerCheckersWeights())

    def _desc(self):
        d = _lib.QmixMixerCheckersDesc()
        d.n_agents, d.embed_dim = self.n, CK_EMBED
        d.grid_h, d.grid_w, d.grid_c = 3, 9, 2
        d.conv_f, d.conv_kh, d.conv_kw = 4, 3, 5
        return d

    def repack(self):
        """Re-arrange the (possibly updated in place) TF-shaped weights into the rows kernel's layout: one launch."""
        d = self._desc()
        _lib.check(self._lib.cm3_qmix_mixer_checkers_pack(ctypes.byref(d), ctypes.byref(self._wt), self._packed.data_ptr(),
                                                          self._stream(None)))

    # ---- launches -------------------------------------------------------------------------------------------------------------------
    def enqueue(self, n_steps, grid, vec, goals, agent_qs, reward=None, done=None, gamma=0.0, q_tot=None, q_tot64=None, td=None,
                stream=None):
        """Raw launch of cm3_qmix_mixer_checkers_rows_f32 on contiguous device tensors: grid int8 or float64 [B, 54], vec float64
        [B, N, 4], goals uint8 [B, N] or int64 [B, N, 2], agent_qs float32 [B, N], reward float32 or float64, done uint8; every output
        is optional, one is required."""
        if grid.dtype not in (torch.int8, torch.float64) or goals.dtype not in (torch.uint8, torch.int64):
            raise Cm3Error("enqueue reads int8 or float64 grids and uint8 index or int64 one-hot goals, not %s / %s"
                           % (grid.dtype, goals.dtype))
        r = _lib.QmixMixerCheckersRows()
        r.n_steps = int(n_steps)
        r.grid, r.vec, r.goals, r.agent_qs = _lib.ptr(grid), _lib.ptr(vec), _lib.ptr(goals), _lib.ptr(agent_qs)
        r.grid_f64 = 1 if grid.dtype == torch.float64 else 0
        r.goals_onehot = 1 if goals.dtype == torch.int64 else 0
        r.reward, r.done = _lib.ptr(reward), _lib.ptr(done)
        r.reward_f64 = 1 if (reward is not None and reward.dtype == torch.float64) else 0
        r.gamma = float(gamma)
        r.q_tot, r.q_tot64, r.td = _lib.ptr(q_tot), _lib.ptr(q_tot64), _lib.ptr(td)
        d = self._desc()
        s = self._stream(stream)
        _lib.check(self._lib.cm3_qmix_mixer_checkers_rows_f32(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(r), s))

    def _stage_cols(self, what, grid, vec, goals, agent_qs, reward=None, done=None):
        """(B, grid, vec, goals, agent_qs, reward, done) contiguous on the mixer's device in the forms the kernel reads, staged as
        CheckersCritic._stage_cols stages them: int8 grids and uint8 index goals as they are, everything else float64 / int64 one-hot
        (leading dimensions may be merged or flattened: vec [B, 4 N], goals [B, 2 N] ...); agent_qs of any float dtype is rounded to
        float32; reward stays float32 or float64 (another dtype is widened to float64); bool or integer done becomes uint8."""
        N = self.n
        if vec.numel() == 0 or vec.numel() % (4 * N):
            raise Cm3Error("%s takes vec [B, %d, 4], got %s" % (what, N, tuple(vec.shape)))
        B = vec.numel() // (4 * N)
        if grid.numel() != B * 54 or goals.numel() not in (B * N, B * N * 2):
            raise Cm3Error("%s takes grid [B, 3, 9, 2] and goals [B, %d, 2] (or [B, %d]) for %d time steps, got %s and %s"
                           % (what, N, N, B, tuple(grid.shape), tuple(goals.shape)))
        if agent_qs.numel() != B * N:
            raise Cm3Error("%s takes agent_qs [B, %d] for %d time steps, got %s" % (what, N, B, tuple(agent_qs.shape)))
        stage = lambda t, dt: t.to(device=self.device, dtype=dt).contiguous()      # noqa: E731
        if goals.numel() == B * N:      # indices (a one-hot column has twice as many elements)
            go = (stage(goals, torch.uint8) if goals.dtype == torch.uint8
                  else torch.nn.functional.one_hot(goals.to(self.device).long().reshape(B, N), 2).contiguous())
        else:
            go = stage(goals, torch.int64)
        gr = stage(grid, torch.int8 if grid.dtype == torch.int8 else torch.float64)
        _, reward, done = stage_td_cols(what, self.device, B, N, None, reward, done, reward_name="reward_local")
        return B, gr, stage(vec, torch.float64), go, stage(agent_qs, torch.float32).reshape(B, N), reward, done

    def q_tot(self, grid, vec, goals, agent_qs, reward_local=None, done=None, gamma=None, keep=None):
        """Qmix_mixer_checkers over the B transitions of a batch, ONE launch: grid = next_grid [B, 3, 9, 2], vec = next_vec [B, N, 4],
        goals [B, N, 2] (or an index [B, N]) and agent_qs [B, N] = each target agent's Q at its argmax (greedy_rows(..., q_max=True))
        give sess.run(mixer_target) of alg_qmix_checkers.train_step (alg_qmix_checkers.py:364-375).  Returns a dict of device tensors:
        "q_tot" float32 [B, 1] (the shape the session returns), "q_tot64" the same values float64 [B, 1], and with reward_local [B, N]
        (float32 / float64), done [B] and gamma also "td" float64 [B] = sum(reward_local[b]) + gamma * q_tot * (1 - done), the bits of
        batch.qmix_td_target on "q_tot".  The three come together or not at all.  keep: an optional list that receives every tensor
        the launch touches (the staged inputs, the outputs), for whoever captures the launch."""
        td = td_given("q_tot", "reward_local", reward_local, done, gamma)
        B, gr, ve, go, aq, rw, dn = self._stage_cols("q_tot", grid, vec, goals, agent_qs, reward_local, done)
        out = td_outputs(self.device, B, "q_tot", td)
        _keep(keep, gr, ve, go, aq, rw, dn, *out.values())
        self.enqueue(B, gr, ve, go, aq, rw, dn, 0.0 if gamma is None else gamma, **out)
        return out


# ---- the particle learner -------------------------------------------------------------------------------------------------------------
_LEARNER_FIELDS = {"h/kernel": "h_kernel", "h/bias": "h_bias", "h2/kernel": "h2_kernel", "h2/bias": "h2_bias", "out/kernel": "out_kernel",
                   "out/bias": "out_bias", "w1": "hyper_w_1", "w_final": "hyper_w_final", "b1": "hyper_b_1",
                   "b_final_l1": "hyper_b_final_l1", "b_final": "hyper_b_final"}
_GUARD = 64          # floats left untouched after every gradient tensor and after the workspace's used part


class _QmixLearner(object):
    """What ParticleQmixLearner and CheckersQmixLearner share: the type and count checks of the two main networks, the gradient store
    (one allocation, every tensor 16-byte aligned with _GUARD floats after it), the Adam moments, powers and segment table
    (cm3_adam_step_f32), the workspace that grows outside of a capture only, and gradients() / step() around the subclass's
    _stage / enqueue_gradients.  A subclass names its two network classes, its workspace entry point and, in _tensors(), the flat
    name -> tensor table of the weights it trains."""
    _agent_cls = _mixer_cls = None
    _workspace_bytes = ""

    def __init__(self, agent, mixer, lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, max_batch=128):
        me, ac, mc = type(self).__name__, self._agent_cls.__name__, self._mixer_cls.__name__
        if not isinstance(agent, self._agent_cls) or not isinstance(mixer, self._mixer_cls):
            raise Cm3Error("%s takes the main %s and the main %s, got %s and %s: build "
                           "them from the Agent_main / Mixer_main variables" % (me, ac, mc, type(agent).__name__, type(mixer).__name__))
        if agent.n != mixer.n:
            raise Cm3Error("%s: the agent is built for %d agents, the mixer for %d; build both for one agent count" % (me, agent.n, mixer.n))
        if agent.device != mixer.device:
            raise Cm3Error("%s: the agent is on %s, the mixer on %s; build both on one device" % (me, agent.device, mixer.device))
        self.agent, self.mixer = agent, mixer
        self.n, self.device = agent.n, agent.device
        self.lr, self.beta1, self.beta2, self.epsilon = float(lr), float(beta1), float(beta2), float(epsilon)
        self._lib = _lib.lib()
        self.w = self._tensors()
        # one allocation for the gradients: every tensor 16-byte aligned with _GUARD floats after it
        offsets, at = {}, 0
        for name, t in self.w.items():
            offsets[name] = at
            at += (t.numel() + 3) // 4 * 4 + _GUARD
        self._grad_store = torch.zeros(at, dtype=torch.float32, device=self.device)
        self.grads = {name: self._grad_store[offsets[name]:offsets[name] + t.numel()].view(t.shape) for name, t in self.w.items()}
        self.m = {name: torch.zeros_like(t) for name, t in self.w.items()}
        self.v = {name: torch.zeros_like(t) for name, t in self.w.items()}
        self._state = torch.tensor([self.beta1, self.beta2, 0.0, 0.0], dtype=torch.float32, device=self.device)
        self.powers = self._state[:2]
        self._bind()
        table = [[self.w[k].data_ptr(), self.grads[k].data_ptr(), self.m[k].data_ptr(), self.v[k].data_ptr(), self.w[k].numel()]
                 for k in self.w]
        self._segments = torch.tensor(table, dtype=torch.int64, device=self.device)
        self._adam = _lib.AdamDesc()
        self._adam.lr, self._adam.beta1, self._adam.beta2, self._adam.epsilon = self.lr, self.beta1, self.beta2, self.epsilon
        self._adam.n_segments, self._adam.total = len(table), sum(row[4] for row in table)
        self.max_batch, self._workspace = 0, None
        self._reserve(int(max_batch))

    def workspace_floats(self, batch):
        """Floats of the workspace the gradient launches use for `batch` transitions (the library's *_workspace_bytes)."""
        nbytes = getattr(self._lib, self._workspace_bytes)(self.n, int(batch))
        if nbytes == 0:
            raise Cm3Error("%s: a batch of %d transitions is out of range" % (type(self).__name__, int(batch)))
        return nbytes // 4

    def _reserve(self, batch):
        if batch <= self.max_batch:
            return
        need = self.workspace_floats(batch)
        if torch.cuda.is_current_stream_capturing():
            raise Cm3Error("%s: a batch of %d transitions needs a larger workspace than max_batch=%d reserved, and a "
                           "capture cannot allocate; build the learner with max_batch >= %d"
                           % (type(self).__name__, batch, self.max_batch, batch))
        self._workspace = torch.zeros(need + _GUARD, dtype=torch.float32, device=self.device)
        self.max_batch = batch

    def _workspace_args(self):
        return self._workspace.data_ptr(), (self._workspace.numel() - _GUARD) * 4

    def enqueue_adam(self, stream=None):
        """Raw launch of cm3_adam_step_f32 over the trained tensors on whatever ``grads`` holds; advances ``powers``."""
        s = _lib.current_stream_handle(self.device) if stream is None else stream
        _lib.check(self._lib.cm3_adam_step_f32(ctypes.byref(self._adam), self._segments.data_ptr(), self._state.data_ptr(), s))

    def gradients(self, cols, td_target, keep=None):
        """Loss and gradients of mixer_op's loss on the columns of a sampled batch (sample_batch / as_reference_batch(numpy=False);
        float64 columns are rounded to float32) and td_target [B] (float64 is rounded as it is read, as the tf.float32 placeholder
        rounds its feed).  Returns {"loss": float32 [1], "q_tot": float32 [B, 1], "grads": {short name: tensor}}; the gradient tensors
        are the learner's own and hold the latest call's values.  Changes no weight, moment or power.  keep: an optional list that
        receives the staged inputs and the outputs, for whoever captures the launches."""
        staged = self._stage(cols, td_target, keep)
        B = staged[0]
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        q_tot = torch.empty(B, 1, dtype=torch.float32, device=self.device)
        _keep(keep, loss, q_tot)
        self.enqueue_gradients(*(staged + (loss, q_tot)))
        return {"loss": loss, "q_tot": q_tot, "grads": self.grads}

    def step(self, cols, td_target, keep=None):
        """sess.run(mixer_op): the launches of gradients(), then ONE Adam launch on agent.w / mixer.w in place, then both repack()s.
        Returns the loss tensor float32 [1] (of the weights before the step, as the session evaluates it)."""
        out = self.gradients(cols, td_target, keep)
        self.enqueue_adam()
        self.agent.repack()
        self.mixer.repack()
        return out["loss"]


def _stage_td(learner, B, td_target):
    """td_target [B] contiguous on the learner's device, float32 as it is or float64 (the launch rounds it as it reads)"""
    if td_target.numel() != B:
        raise Cm3Error("%s takes td_target [B] for %d time steps, got %s" % (type(learner).__name__, B, tuple(td_target.shape)))
    return td_target.reshape(-1).to(device=learner.device,
                                    dtype=td_target.dtype if td_target.dtype == torch.float32 else torch.float64).contiguous()


class ParticleQmixLearner(_QmixLearner):
    """mixer_op of the reference's particle QMIX on the device: loss, gradients and tf.train.AdamOptimizer's step, no session.

        reference                                                    here
        ---------------------------------------------------------   -----------------------------------------------
        self.loss_mixer, self.mixer_op = AdamOptimizer(lr)           ParticleQmixLearner(agent, mixer, lr)
          .minimize(loss) (alg_qmix.py:186-192)                        agent / mixer: the Agent_main / Mixer_main objects
        sess.run(self.mixer_op, feed) (:371-378)                     learner.step(cols, td_target) -> loss
        the whole of train_step (:338-380)                           learner.train_step(cols, gamma, target_agent, target_mixer, tau)

    agent is the main ParticleQmixAgent, mixer the main ParticleQmixMixer, for one agent count on one device.  The learner owns the
    Adam moments ``m`` / ``v`` and the gradient tensors ``grads`` (TF-shaped float32, under the short names of NAMES and MIXER_NAMES),
    the two power scalars ``powers`` (device memory, advanced by every Adam launch, as TF keeps beta1_power / beta2_power) and a
    persistent workspace sized for max_batch transitions; a larger batch grows it, outside of a capture only.  step() trains
    ``agent.w`` / ``mixer.w`` in place and repacks both, so the next launch of either follows the new weights.  Not a _DeviceNet: it
    holds no weights of its own and none of the launch-hook names cm3_amd.rollout dispatches on.  (gradients, step, enqueue_adam,
    workspace_floats: _QmixLearner, shared with CheckersQmixLearner.)"""
    _agent_cls, _mixer_cls = ParticleQmixAgent, ParticleQmixMixer
    _workspace_bytes = "cm3_qmix_learner_particle_workspace_bytes"

    def _tensors(self):
        w = dict(self.agent.w)
        w.update(self.mixer.w)
        return w

    def _bind(self):
        self._wt, self._gt = _lib.QmixLearnerTensors(), _lib.QmixLearnerTensors()
        for name, field in _LEARNER_FIELDS.items():
            setattr(self._wt, field, self.w[name].data_ptr())
            setattr(self._gt, field, self.grads[name].data_ptr())

    def _desc(self):
        d = _lib.QmixLearnerParticleDesc()
        d.n_agents, d.n_h, d.n_actions, d.embed_dim = self.n, H, N_ACTIONS, EMBED
        return d

    def _stage(self, cols, td_target, keep):
        vg = cols["v_global"]
        if vg.dim() != 3 or vg.shape[1] != self.n or vg.shape[2] != 4 or vg.shape[0] == 0:
            raise Cm3Error("ParticleQmixLearner for %d agents takes v_global [B, %d, 4], got %s" % (self.n, self.n, tuple(vg.shape)))
        B, N, L = int(vg.shape[0]), self.n, self.agent.L
        f32 = lambda t: t.to(device=self.device, dtype=torch.float32).contiguous()      # noqa: E731
        want = {"obs_others": (B, N, L), "v_local": (B, N, 4), "goals": (B, N, 2), "actions": (B, N)}
        for name, shape in want.items():
            if tuple(cols[name].shape) != shape:
                raise Cm3Error("ParticleQmixLearner takes %s %s, got %s" % (name, list(shape), tuple(cols[name].shape)))
        td = _stage_td(self, B, td_target)
        staged = (f32(cols["obs_others"]), f32(cols["v_local"]), f32(cols["goals"]),
                  cols["actions"].to(device=self.device, dtype=torch.int32).contiguous(), f32(vg), td)
        _keep(keep, *staged)
        return (B,) + staged

    def enqueue_gradients(self, B, obs_others, v_local, goals, actions, v_global, td, loss, q_tot, stream=None):
        """Raw launches of cm3_qmix_learner_particle_grad_f32 on contiguous device tensors (float32 columns, int32 actions, float32 or
        float64 td [B]); loss float32 [1], q_tot float32 [B]."""
        self._reserve(B)
        r = _lib.QmixLearnerRows()
        r.td_f64 = 1 if td.dtype == torch.float64 else 0
        r.obs_others, r.v_obs, r.goals, r.actions = _lib.ptr(obs_others), _lib.ptr(v_local), _lib.ptr(goals), _lib.ptr(actions)
        r.state, r.td, r.loss, r.q_tot = _lib.ptr(v_global), _lib.ptr(td), _lib.ptr(loss), _lib.ptr(q_tot)
        r.n_steps = int(B)
        d = self._desc()
        s = _lib.current_stream_handle(self.device) if stream is None else stream
        ws, ws_bytes = self._workspace_args()
        _lib.check(self._lib.cm3_qmix_learner_particle_grad_f32(
            ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(self._gt), ctypes.byref(r), ws, ws_bytes, s))

    def train_step(self, cols, gamma, target_agent, target_mixer, tau, keep=None):
        """The whole of alg_qmix.train_step (alg_qmix.py:338-380) with no `run`: the target agents' argmax Q on the next
        observations (target_agent.greedy_rows), the target mixer's q_tot and the TD target (target_mixer.q_tot), step(), then the
        soft updates of both target networks (list_update_target_ops).  Returns the loss tensor."""
        vg = cols["v_global"]
        B, N = vg.shape[0], vg.shape[1]
        rows = lambda x: x.reshape(B * N, -1)      # noqa: E731
        greedy = target_agent.greedy_rows(rows(cols["obs_others_next"]), rows(cols["v_local_next"]), rows(cols["goals"]), onehot=False,
                                          q_max=True)
        td = target_mixer.q_tot(cols["v_global_next"], cols["goals"], greedy["q_max"].reshape(B, N), cols["reward_local"].reshape(B, N),
                                cols["done"], gamma, keep=keep)["td"]
        _keep(keep, *greedy.values())
        loss = self.step(cols, td, keep)
        target_agent.soft_update_from(self.agent, tau)
        target_mixer.soft_update_from(self.mixer, tau)
        return loss


# ---- the Checkers learner -------------------------------------------------------------------------------------------------------------
class CheckersQmixLearner(_QmixLearner):
    """mixer_op of the reference's Checkers QMIX on the device: loss, gradients and tf.train.AdamOptimizer's step, no session -- the
    twin of ParticleQmixLearner.

        reference                                                    here
        ---------------------------------------------------------   -----------------------------------------------
        self.loss_mixer, self.mixer_op = AdamOptimizer(lr)           CheckersQmixLearner(agent, mixer, lr)
          .minimize(loss) (alg_qmix_checkers.py:184-190)               agent / mixer: the Agent_main / Mixer_main objects
        sess.run(self.mixer_op, feed) (:381-391)                     learner.step(cols, td_target) -> loss
        the whole of train_step (:342-393)                           learner.train_step(cols, gamma, target_agent, target_mixer, tau)

    agent is the main CheckersQmixAgent (either precision), mixer the main CheckersQmixMixer, for one agent count (1..8) on one device.
    The twenty trained tensors -- ``w``, and with the same keys ``grads``, ``m`` and ``v`` -- are named "agent/<short name of
    CK_NAMES>" and "mixer/<short name of CK_MIXER_NAMES>" (both networks have a conv_w and a conv_b); ``w`` holds the very tensors of
    ``agent.w`` / ``mixer.w``.  The learner's forward pass is exact float32 on those tensors whatever the agent's precision (at "f32"
    its Q values are greedy_rows' bits); step() trains them in place and repacks both networks at their own precision.  cols: the
    columns of a sampled Checkers batch (either ring's sample_batch, as_reference_batch(numpy=False)), read in the forms the rows
    kernels read: int8 windows / grids and uint8 index goals as they are, everything else float64 / int64 one-hot."""
    _agent_cls, _mixer_cls = CheckersQmixAgent, CheckersQmixMixer
    _workspace_bytes = "cm3_qmix_learner_checkers_workspace_bytes"

    def _tensors(self):
        w = {"agent/" + k: t for k, t in self.agent.w.items()}
        w.update({"mixer/" + k: t for k, t in self.mixer.w.items()})
        return w

    def _bind(self):
        self._agt, self._mgt = _lib.ActorCheckersWeights(), _lib.QmixMixerCheckersWeights()
        for k in self.agent.w:
            setattr(self._agt, k, self.grads["agent/" + k].data_ptr())
        for k in self.mixer.w:
            setattr(self._mgt, k, self.grads["mixer/" + k].data_ptr())

    def _desc(self):
        d = _lib.QmixLearnerCheckersDesc()
        d.n_agents, d.conv_f, d.n_conv_linear, d.n_h1, d.n_h2, d.n_actions = self.n, 6, 32, 256, 256, N_ACTIONS
        d.embed_dim, d.mixer_conv_f = CK_EMBED, 4
        return d

    def _stage(self, cols, td_target, keep):
        vec = cols["vec"]
        if vec.dim() != 3 or vec.shape[1] != self.n or vec.shape[2] != 4 or vec.shape[0] == 0:
            raise Cm3Error("CheckersQmixLearner for %d agents takes vec [B, %d, 4], got %s" % (self.n, self.n, tuple(vec.shape)))
        B, N = int(vec.shape[0]), self.n
        if tuple(cols["actions"].shape) != (B, N):
            raise Cm3Error("CheckersQmixLearner takes actions [%d, %d], got %s" % (B, N, tuple(cols["actions"].shape)))
        _, ot, ov, oo, ap, vg = stage_checkers_rows("CheckersQmixLearner", self.device, self.agent.Lo, cols["obs_self_t"], cols["obs_self_v"],
                                                    cols["obs_others"], cols["actions_prev"], cols["goals"])
        if cols["grid"].numel() != B * 54:
            raise Cm3Error("CheckersQmixLearner takes grid [B, 3, 9, 2] for %d time steps, got %s" % (B, tuple(cols["grid"].shape)))
        grid = cols["grid"]
        grid = grid.to(device=self.device, dtype=torch.int8 if grid.dtype == torch.int8 else torch.float64).contiguous()
        staged = (ot, ov, oo, ap, cols["actions"].to(device=self.device, dtype=torch.int32).contiguous(), vg, grid,
                  vec.to(device=self.device, dtype=torch.float64).contiguous(), _stage_td(self, B, td_target))
        _keep(keep, *staged)
        return (B,) + staged

    def enqueue_gradients(self, B, obs_self_t, obs_self_v, obs_others, actions_prev, actions, goals, grid, vec, td, loss, q_tot,
                          stream=None):
        """Raw launches of cm3_qmix_learner_checkers_grad_f32 on contiguous device tensors: obs_self_t int8 or float64 [B, N, 75],
        obs_self_v / obs_others / vec float64, actions_prev / actions int32 [B, N], goals uint8 [B, N] or int64 [B, N, 2], grid int8 or
        float64 [B, 54], td float32 or float64 [B]; loss float32 [1], q_tot float32 [B]."""
        if (obs_self_t.dtype not in (torch.int8, torch.float64) or grid.dtype not in (torch.int8, torch.float64)
                or goals.dtype not in (torch.uint8, torch.int64)):
            raise Cm3Error("enqueue_gradients reads int8 or float64 windows and grids and uint8 index or int64 one-hot goals, not %s / %s "
                           "/ %s" % (obs_self_t.dtype, grid.dtype, goals.dtype))
        self._reserve(B)
        r = _lib.QmixLearnerCheckersRows()
        r.obs_self_t_f64 = 1 if obs_self_t.dtype == torch.float64 else 0
        r.grid_f64 = 1 if grid.dtype == torch.float64 else 0
        r.goals_onehot = 1 if goals.dtype == torch.int64 else 0
        r.td_f64 = 1 if td.dtype == torch.float64 else 0
        r.obs_self_t, r.obs_self_v, r.obs_others = _lib.ptr(obs_self_t), _lib.ptr(obs_self_v), _lib.ptr(obs_others)
        r.actions_prev, r.actions, r.goals, r.grid, r.vec = _lib.ptr(actions_prev), _lib.ptr(actions), _lib.ptr(goals), _lib.ptr(grid), _lib.ptr(vec)
        r.td, r.loss, r.q_tot = _lib.ptr(td), _lib.ptr(loss), _lib.ptr(q_tot)
        r.n_steps = int(B)
        d = self._desc()
        s = _lib.current_stream_handle(self.device) if stream is None else stream
        ws, ws_bytes = self._workspace_args()
        _lib.check(self._lib.cm3_qmix_learner_checkers_grad_f32(
            ctypes.byref(d), ctypes.byref(self.agent._wt), ctypes.byref(self.mixer._wt), ctypes.byref(self._agt), ctypes.byref(self._mgt),
            ctypes.byref(r), ws, ws_bytes, s))

    def train_step(self, cols, gamma, target_agent, target_mixer, tau, keep=None):
        """The whole of alg_qmix_checkers.train_step (alg_qmix_checkers.py:342-393) with no `run`.  The TD target is the reference
        graph's (:96-106): the target agents' argmax on the next_* columns with the `actions` column fed as actions_prev
        (target_agent.greedy_rows), agent_qs = the MAIN agent's Q at that argmax, the target mixer's q_tot on it
        (qmix_train_step_feeds(env="checkers", target_agent=, target_mixer=, mixer_q_agent=learner.agent) forms the same); then
        step() and the soft updates of both target networks (list_update_target_ops).  Returns the loss tensor."""
        vec = cols["vec"]
        B, N = vec.shape[0], vec.shape[1]
        rows = lambda x: x.reshape(B * N, *x.shape[2:])      # noqa: E731
        nxt = (rows(cols["next_obs_self_t"]), rows(cols["next_obs_self_v"]), rows(cols["next_obs_others"]), cols["actions"].reshape(B * N),
               rows(cols["goals"]))
        greedy = target_agent.greedy_rows(*nxt, onehot=False)
        q_main = self.agent.greedy_rows(*nxt, q=True, onehot=False)["q"]
        agent_qs = q_main.gather(1, greedy["argmax"].long().unsqueeze(1))
        td = target_mixer.q_tot(cols["next_grid"], cols["next_vec"], cols["goals"], agent_qs.reshape(B, N),
                                cols["local_rewards"].reshape(B, N), cols["done"], gamma, keep=keep)["td"]
        _keep(keep, q_main, agent_qs, *greedy.values())
        loss = self.step(cols, td, keep)
        target_agent.soft_update_from(self.agent, tau)
        target_mixer.soft_update_from(self.mixer, tau)
        return loss
