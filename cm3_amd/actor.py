"""ParticleActor -- the reference's particle policy evaluated on the device.

    reference                                                    here
    ---------------------------------------------------------   -----------------------------------------
    networks.actor_particle(obs_others, v_obs, v_goal, ...)      ParticleActor(weights, n_agents, stage)
      (networks.py:517-538)                                        weights: dict keyed by the TF variable names
    probs = (1-eps) probs + eps/l_action; multinomial            actor.act(env, epsilon) -> actions [E, N]
      (alg_credit.py:119-120)                                      (one launch: forward + mixing + sampling)
    alg.run_actor(local_others, local_self, goals, eps, sess)    ParticleRollout.collect(policy=actor, epsilon=..)
      (alg_credit.py:249-270, called at train_onpolicy.py:313)     step and actor launches alternate inside ONE
                                                                   hipGraph; nothing returns to the host

Weights stay float32 [in][out] as TensorFlow shapes them, so a checkpoint exported with
``{v.name: sess.run(v)}`` loads unchanged (names below; a "Policy_main/" prefix and ":0" suffix are ignored).

The actor reads float32 and float64 env buffers (VecParticleEnv(dtype=...)).  On a float64 env -- the reference-precision mode --
it rounds the observation to float32 as it stages its inputs, which is what the reference's tf.float32 placeholders do with its
float64 observations (alg_credit.py:96-111): the network itself is float32 either way.

Both actors derive from cm3_amd._net._DeviceNet, which loads the weights and has ``soft_update_from(main, tau)``: w <- tau * main.w +
(1 - tau) * w in float32, then repack() -- the actor half of list_update_target_ops (alg_credit.py:186-194, run at :775;
alg_credit_checkers.py:72, run at :773), for an actor holding the Policy_target weights.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import Cm3Error
from ._net import _DeviceNet, _keep, canon, sample_outputs, stage_particle_rows      # noqa: F401  (_keep: re-exported)


def _epsilon_args(epsilon):
    """(float for the descriptor, device pointer or 0): a float32 device tensor is read by the launch itself, so a
    captured hipGraph follows the annealed epsilon (train_onpolicy.py:369) without being re-captured."""
    if isinstance(epsilon, torch.Tensor):
        if epsilon.dtype != torch.float32 or epsilon.numel() != 1 or epsilon.device.type != "cuda":
            raise Cm3Error("a device epsilon must be one float32 element on the GPU")
        return 0.0, epsilon.data_ptr()
    return float(epsilon), 0


class RowsDrawCounter(object):
    """The draw counter of the rows sampling stream IN DEVICE MEMORY: two uint32 words {draw, arrivals} that a counted launch
    (cm3_actor_particle_rows_counted_f32 / cm3_actor_checkers_rows_counted_f32) reads and advances itself -- what
    ``sample_rows(..., draw=counter)`` takes, so that the launch can be captured into a hipGraph and still draw afresh on every
    replay.  One counter may serve any number of actors; the launches that share it must be ordered on the device (one stream, or
    the dependencies of one graph)."""

    def __init__(self, device, start=0):
        self.device = _lib.require_gpu(device)
        # (int32 storage: the launch reads the same 32 bits)
        self.state = torch.zeros(2, dtype=torch.int32, device=self.device)
        if self.state.data_ptr() % 8:
            raise Cm3Error("RowsDrawCounter: the allocator returned a tensor that is not 8-byte aligned")
        self.set(start)

    @staticmethod
    def _signed(v):
        v = int(v) & 0xFFFFFFFF
        return v - (1 << 32) if v >= (1 << 31) else v

    def set(self, v):
        """draw <- v (mod 2^32), arrivals <- 0, in stream order."""
        self.state.copy_(torch.tensor([self._signed(v), 0], dtype=torch.int32), non_blocking=False)
        return self

    def value(self):
        """The draw the NEXT counted launch will use (a synchronising read)."""
        return int(self.state[0].item()) & 0xFFFFFFFF

    def arrivals(self):
        """The ticket word (a synchronising read): 0 between launches."""
        return int(self.state[1].item()) & 0xFFFFFFFF

    def data_ptr(self):
        return self.state.data_ptr()


def _actor_entry(lib, dtype):
    """cm3_actor_particle_f32 / _f64 by the real of the env buffers the launch reads."""
    if dtype == torch.float32:
        return lib.cm3_actor_particle_f32
    if dtype == torch.float64:
        return lib.cm3_actor_particle_f64
    raise Cm3Error("the device actor reads float32 or float64 env buffers, not %s" % (dtype,))


H1_SELF, H1_OTHERS, H2, N_ACTIONS = 64, 128, 64, 5
PRECISIONS = {"f32": 0, "bf16": 1, "f16x3": 2}       # cm3_actor_particle_desc.precision
_NAMES = {
    "w_self": "actor_branch_self/kernel", "b_self": "actor_branch_self/bias", "w_self_h2": "W_branch_self_h2",
    "w_others": "stage-2/actor_others/kernel", "b_others": "stage-2/actor_others/bias",
    "w_others_h2": "stage-2/W_others_h2", "b_h2": "b", "w_out": "actor_out/kernel", "b_out": "actor_out/bias"}
_PREFIXES = ("Policy_main/", "Policy_target/")


def _canon(name):
    return canon(name, _PREFIXES)


def rows_id_base_i64(row_id_base):
    """row_id_base as cm3_actor_rows holds it: an int64_t (include/cm3_amd.h).  A value outside the field is refused -- a ctypes
    field would keep its low 64 bits without a word, and ids from 2^63 on would come back negative.  (cm3_actor_checkers_rows
    declares its base uint64_t and takes every 64-bit value.)"""
    base = int(row_id_base)
    if not -(1 << 63) <= base < (1 << 63):
        raise Cm3Error("row_id_base %d does not fit cm3_actor_rows.row_id_base (int64_t): -2^63 <= row_id_base < 2^63" % base)
    return base


class ParticleActor(_DeviceNet):
    _match = ("n", "stage")
    _refusal = "the main actor must be a ParticleActor for %(n)d agents at stage %(stage)d"

    def __init__(self, weights, n_agents, stage=2, device="cuda:0", seed=12341, env_id_base=0, precision="f32"):
        """precision of the 192 -> 64 second layer (87 % of the network's FLOPs):
        "f32"     exact float32 MFMA -- a k-ordered fmaf chain, the numerics of a plain float32 loop;
        "f16x3"   split float16: activations and weights as hi + lo float16 pairs, three f16 MFMA passes (hi hi + hi lo +
                  lo hi), float32 accumulation.  22 of the 24 significand bits per factor: probabilities within the same 2e-5
                  of the float64 oracle as "f32" (tests/test_gpu_actor.py), ~5x fewer matrix-core cycles.  First-layer
                  activations must stay below float16's 65504 (three orders of magnitude above a trained policy's).  With 5..9
                  agents (16..32 others inputs) actor_others runs in the same split float16 (csrc/actor.hip ActorFirstB::kF16Oth);
        "bf16"    plain bf16 operands: fastest, probabilities within ~1e-2 -- not a parity path."""
        self.device = _lib.require_gpu(device)
        if precision not in PRECISIONS:
            raise Cm3Error("precision must be one of %s" % sorted(PRECISIONS))
        self.precision = precision
        self.n = int(n_agents)
        self.stage = int(stage)
        self.L = 4 * max(self.n - 1, 1)
        self.seed = int(seed)
        self.env_id_base = int(env_id_base)
        self.rows_draw = 0          # launch counter of the rows stream (sample_rows)
        shapes = {"w_self": (6, H1_SELF), "b_self": (H1_SELF,), "w_self_h2": (H1_SELF, H2), "b_h2": (H2,),
                  "w_out": (H2, N_ACTIONS), "b_out": (N_ACTIONS,)}
        if self.stage > 1:
            shapes.update({"w_others": (self.L, H1_OTHERS), "b_others": (H1_OTHERS,), "w_others_h2": (H1_OTHERS, H2)})
        self._load(weights, _PREFIXES, _NAMES, shapes, "actor", lambda lib: lib.cm3_actor_particle_packed_bytes(self.n),
                   _lib.ActorParticleWeights())

    def repack(self):
        """Re-arrange the (possibly updated in place) TF-shaped weights into the forward kernel's layout."""
        d = self._desc(1, 0.0, 0)
        _lib.check(self._lib.cm3_actor_particle_pack(ctypes.byref(d), ctypes.byref(self._wt), self._packed.data_ptr(),
                                                     self._stream(None)))

    def _desc(self, n_envs, epsilon, env_id_base):
        d = _lib.ActorParticleDesc()
        d.n_envs, d.n_agents, d.stage = int(n_envs), self.n, self.stage
        d.n_h1_self, d.n_h1_others, d.n_h2, d.n_actions = H1_SELF, H1_OTHERS, H2, N_ACTIONS
        d.epsilon = float(epsilon)
        d.precision = PRECISIONS[self.precision]
        d.env_id_base = int(env_id_base)
        d.seed = self.seed & 0xFFFFFFFFFFFFFFFF
        return d

    def enqueue(self, n_envs, obs_others, state, goals, meta, episode, actions, epsilon, probs=None, stream=None,
                env_id_base=None, dtype=torch.float32):
        """Raw launch on device pointers/tensors; dtype: the real of obs_others / state / goals (torch.float32 or torch.float64 --
        cm3_actor_particle_f32 / _f64).  actions int32, probs float32 either way."""
        fn = _actor_entry(self._lib, dtype)
        b = _lib.ActorParticleBufs()
        b.obs_others, b.state, b.goals = _lib.ptr(obs_others), _lib.ptr(state), _lib.ptr(goals)
        b.meta, b.episode, b.actions, b.probs = _lib.ptr(meta), _lib.ptr(episode), _lib.ptr(actions), _lib.ptr(probs)
        epsilon, b.epsilon_dev = _epsilon_args(epsilon)
        d = self._desc(n_envs, epsilon, self.env_id_base if env_id_base is None else env_id_base)
        s = self._stream(stream)
        _lib.check(fn(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(b), s))

    def act(self, env, epsilon, return_probs=False):
        """Actions [E, N] int32 for the env's CURRENT observation (alg.run_actor); optionally the mixed
        probabilities [E, N, 5] (float32).  float32 and float64 envs alike."""
        if env.n != self.n:
            raise Cm3Error("actor built for %d agents, env has %d" % (self.n, env.n))
        cur = env._cur
        actions = torch.empty(env.E, env.n, dtype=torch.int32, device=self.device)
        probs = torch.empty(env.E, env.n, N_ACTIONS, dtype=torch.float32, device=self.device) if return_probs else None
        self.enqueue(env.E, env._obs_others[cur], env._state[cur], env._goals, env._meta, env._episode, actions,
                     epsilon, probs, env_id_base=env.env_id_base, dtype=env.dtype)
        return (actions, probs) if return_probs else actions

    # ---- the actor over the rows of a sampled batch (cm3_actor_particle_rows_f32): the two evaluations of alg_credit.train_step ----
    def enqueue_rows(self, n_rows, obs_others, v_obs, goals, epsilon, probs=None, actions=None, onehot=None, draw=0, row_id_base=0,
                     stream=None):
        """Raw launch of cm3_actor_particle_rows_f32 on contiguous float32 device tensors; every output is optional, one is
        required.  epsilon: a float, or a one-element float32 device tensor the launch reads itself.  (seed, row_id_base + row,
        draw) key the row's uniform; nothing is drawn when actions and onehot are both None.  row_id_base: an int64 (the ABI's
        field; Cm3Error outside it).  draw: an integer, or a RowsDrawCounter -- then the launch is
        cm3_actor_particle_rows_counted_f32, which reads the counter's device word and advances it itself."""
        r = _lib.ActorRows()
        r.obs_others, r.v_obs, r.goals = _lib.ptr(obs_others), _lib.ptr(v_obs), _lib.ptr(goals)
        r.probs, r.actions, r.onehot = _lib.ptr(probs), _lib.ptr(actions), _lib.ptr(onehot)
        epsilon, r.epsilon_dev = _epsilon_args(epsilon)
        counter = draw if isinstance(draw, RowsDrawCounter) else None
        r.n_rows, r.row_id_base, r.draw = int(n_rows), rows_id_base_i64(row_id_base), 0 if counter is not None else int(draw) & 0xFFFFFFFF
        d = self._desc(1, epsilon, 0)
        s = self._stream(stream)
        if counter is not None:
            _lib.check(self._lib.cm3_actor_particle_rows_counted_f32(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(r),
                                                                     counter.data_ptr(), s))
        else:
            _lib.check(self._lib.cm3_actor_particle_rows_f32(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(r), s))

    def probs_rows(self, obs_others, v_obs, goals, epsilon, keep=None):
        """The mixed probabilities float32 [R, 5] over the R = prod(leading shape) rows, ONE launch: the reference's
        sess.run(self.probs, ...) of train_step (alg_credit.py:121, fetched at :708 / :729) on the columns obs_others / v_local /
        goals of a sampled batch.  Nothing is drawn.  A row's probabilities are the bits act() computes for the same inputs.
        keep: an optional list that receives every tensor this call allocated and the launch touches (the output, the staged
        inputs) -- whoever captures the launch into a hipGraph holds them for as long as the graph is replayed."""
        rows, oo, vo, vg = stage_particle_rows("probs_rows", self.device, self.L, obs_others, v_obs, goals)
        probs = torch.empty(rows, N_ACTIONS, dtype=torch.float32, device=self.device)
        _keep(keep, oo, vo, vg, probs)
        self.enqueue_rows(rows, oo, vo, vg, epsilon, probs=probs)
        return probs

    def sample_rows(self, obs_others, v_obs, goals, epsilon, probs=False, onehot=False, draw=None, keep=None):
        """Actions sampled from the mixed probabilities over transition rows, ONE launch: with the Policy_target weights this is
        action_samples_target of train_step (alg_credit.py:128, run_actor_target :272-287) on obs_others_next / v_local_next /
        goals.  Returns a dict of device tensors: "actions" int32 [R] always; "probs" float32 [R, 5] and "onehot" int64 [R, 5] when
        asked for.  The uniforms are the build's own rows stream keyed (seed, row, draw): draw=None takes the actor's counter
        self.rows_draw and advances it, so successive calls draw afresh; an explicit draw reproduces a call (and leaves the
        counter alone); a RowsDrawCounter makes the launch read and advance that counter on the device (capturable: every
        replay draws afresh; self.rows_draw is left alone).  keep: as probs_rows."""
        rows, oo, vo, vg = stage_particle_rows("sample_rows", self.device, self.L, obs_others, v_obs, goals)
        out = sample_outputs(self.device, rows, probs, onehot)
        if draw is None:
            draw, self.rows_draw = self.rows_draw, (self.rows_draw + 1) & 0xFFFFFFFF
        _keep(keep, oo, vo, vg, *out.values())
        self.enqueue_rows(rows, oo, vo, vg, epsilon, draw=draw, **out)
        return out



_CK_NAMES = {
    "conv_w": "conv/Conv/weights", "conv_b": "conv/Conv/biases", "lin_w": "conv_linear/kernel",
    "lin_b": "conv_linear/bias", "self_w": "branch_self/kernel", "self_b": "branch_self/bias", "w_self_h2": "W_self_h2",
    "others_w": "stage-2/branch_others/kernel", "others_b": "stage-2/branch_others/bias",
    "w_others_h2": "stage-2/W_others_h2", "b_h2": "b", "out_w": "actor_out/kernel", "out_b": "actor_out/bias"}
CK_CONV_F, CK_CONV_LIN, CK_H1, CK_H2 = 6, 32, 256, 256


def checkers_policy_shapes(Lo):
    """short name -> shape of the thirteen TF variables of networks.actor_checkers / Qmix_single_checkers with Lo others inputs"""
    return {"conv_w": (3, 3, 3, CK_CONV_F), "conv_b": (CK_CONV_F,), "lin_w": (25 * CK_CONV_F, CK_CONV_LIN),
            "lin_b": (CK_CONV_LIN,), "self_w": (CK_CONV_LIN + 4 + N_ACTIONS + 2, CK_H1), "self_b": (CK_H1,),
            "w_self_h2": (CK_H1, CK_H2), "others_w": (Lo, CK_H1), "others_b": (CK_H1,), "w_others_h2": (CK_H1, CK_H2),
            "b_h2": (CK_H2,), "out_w": (CK_H2, N_ACTIONS), "out_b": (N_ACTIONS,)}


def stage_checkers_rows(what, device, Lo, obs_self_t, obs_self_v, obs_others, actions_prev, goals):
    """(rows, obs_self_t, obs_self_v, obs_others, actions_prev, goals) contiguous on `device`, in the forms the Checkers rows kernels
    read (cm3_actor_checkers_rows_f32, cm3_qmix_checkers_rows_f32), from inputs with equal leading shape [...]: obs_self_t
    [..., 5, 5, 3] or [..., 75]; obs_self_v [..., 4]; obs_others [..., Lo]; actions_prev [...] (0..4); goals a one-hot [..., 2] or an
    index [...].  int8 windows and uint8 index goals go in as they are (what the trajectory and the compact ring keep); everything
    else becomes float64 windows / int64 one-hot goals (no copy for the columns sample_batch returns)."""
    lead = tuple(obs_self_v.shape[:-1])
    win = tuple(obs_self_t.shape)
    index_goals = tuple(goals.shape) == lead
    if (win not in (lead + (5, 5, 3), lead + (75,)) or tuple(obs_self_v.shape) != lead + (4,)
            or tuple(obs_others.shape) != lead + (Lo,) or tuple(actions_prev.shape) != lead
            or not (index_goals or tuple(goals.shape) == lead + (2,))):
        raise Cm3Error("%s takes [..., 5, 5, 3] (or [..., 75]), [..., 4], [..., %d], [...] and [..., 2] (or [...]) with equal "
                       "leading shape, got %s, %s, %s, %s, %s" % (what, Lo, win, tuple(obs_self_v.shape), tuple(obs_others.shape),
                                                                  tuple(actions_prev.shape), tuple(goals.shape)))
    rows = int(np.prod(lead, dtype=np.int64))
    if rows <= 0:
        raise Cm3Error("%s needs at least one row" % what)
    stage = lambda t, dt: t.to(device=device, dtype=dt).contiguous()      # noqa: E731
    ot = stage(obs_self_t, torch.int8 if obs_self_t.dtype == torch.int8 else torch.float64)
    if index_goals:
        vg = (stage(goals, torch.uint8) if goals.dtype == torch.uint8
              else torch.nn.functional.one_hot(goals.to(device).long(), 2).contiguous())
    else:
        vg = stage(goals, torch.int64)
    return rows, ot, stage(obs_self_v, torch.float64), stage(obs_others, torch.float64), stage(actions_prev, torch.int32), vg


class _CheckersPolicyNet(_DeviceNet):
    """What CheckersActor and CheckersQmixAgent share: one network (cm3_actor_checkers_weights / _desc), two heads.  The launches are
    private here and take the library's entry point; each class publishes them under the hook names cm3_amd.rollout looks for."""
    _net_stage = 2          # cm3_actor_checkers_desc.stage (the QMIX network has the others branch at every agent count)

    def _desc(self, n_envs, epsilon, env_id_base, obst_stride):
        d = _lib.ActorCheckersDesc()
        d.n_envs, d.n_agents, d.stage, d.n_obs = int(n_envs), self.n, self._net_stage, 2
        d.conv_f, d.n_conv_linear, d.n_h1, d.n_h2, d.n_actions = CK_CONV_F, CK_CONV_LIN, CK_H1, CK_H2, N_ACTIONS
        d.epsilon = float(epsilon)
        d.precision = PRECISIONS[self.precision]
        d.obs_self_t_stride = int(obst_stride)
        d.env_id_base = int(env_id_base)
        d.seed = self.seed & 0xFFFFFFFFFFFFFFFF
        return d

    def _enqueue_tick(self, fn, n_envs, obs_self_t_raw, obst_stride, obs_self_v, obs_others, goals, actions_prev, steps, episode,
                      actions, epsilon, probs, stream, env_id_base, prev_done):
        b = _lib.ActorCheckersBufs()
        b.obs_self_t, b.obs_self_v, b.obs_others = _lib.ptr(obs_self_t_raw), _lib.ptr(obs_self_v), _lib.ptr(obs_others)
        b.goals, b.actions_prev, b.steps, b.episode = (_lib.ptr(goals), _lib.ptr(actions_prev), _lib.ptr(steps),
                                                       _lib.ptr(episode))
        b.actions, b.probs = _lib.ptr(actions), _lib.ptr(probs)
        b.prev_done = _lib.ptr(prev_done)
        epsilon, b.epsilon_dev = _epsilon_args(epsilon)
        d = self._desc(n_envs, epsilon, self.env_id_base if env_id_base is None else env_id_base, obst_stride)
        _lib.check(fn(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(b), self._stream(stream)))

    def _enqueue_whole(self, fn, env_desc, traj, n_envs, obst_stride, n_ticks, epsilon, prev0, probs, stream, final_obs, prev0_next):
        epsilon, eps_dev = _epsilon_args(epsilon)
        d = self._desc(n_envs, epsilon, env_desc.env_id_base, obst_stride)
        _lib.check(fn(
            ctypes.byref(env_desc), ctypes.byref(traj), ctypes.byref(d), ctypes.byref(self._wt), _lib.ptr(prev0), _lib.ptr(prev0_next),
            _lib.ptr(probs), 0 if probs is None else probs[0].numel() * probs.element_size(), eps_dev,
            None if final_obs is None else ctypes.byref(final_obs), int(n_ticks), self._stream(stream)))


class CheckersActor(_CheckersPolicyNet):
    """The reference's Checkers policy evaluated on the device.

        reference                                                        here
        -------------------------------------------------------------   ----------------------------------------
        networks.actor_checkers(a_prev, t_obs_self, v_obs_self,          CheckersActor(weights, n_agents, stage)
            v_obs_others, v_goal, f1=6, k1=[3,3], n_h1=256, n_h2=256)      weights: dict keyed by the TF variable names
            (networks.py:549-578; conv: convnet_1 :67-75)
        probs = (1-eps) probs + eps/5; multinomial                       actor.act(env, epsilon, actions_prev)
            (alg_credit_checkers.py:112-113)                               -> actions [E, N] (one launch)
        alg.run_actor(actions_prev, obs_others, obs_self_t, obs_self_v,  CheckersRollout.collect(goals, policy=actor,
            goals, eps, sess)  (alg_credit_checkers.py:229-253)            epsilon=..): actor and step launches alternate
                                                                           inside ONE hipGraph
    """
    _match = ("n", "stage")
    _refusal = "the main actor must be a CheckersActor for %(n)d agents at stage %(stage)d"

    def __init__(self, weights, n_agents, stage=2, device="cuda:0", seed=12341, env_id_base=0, precision="f32"):
        """precision: "f32" (default: every layer on the exact-f32 MFMA), "f16x3" (every layer in split float16: activations and
        weights as float16 hi + lo, three float16 MFMAs per product with float32 accumulation -- held to the same 2e-5 parity
        bound as "f32", half its time per launch), or "bf16" (the two 256x256 layers rounded to bf16; not a parity path:
        probabilities within ~1e-2 of the float32 ones)."""
        self.device = _lib.require_gpu(device)
        if precision not in PRECISIONS:
            raise Cm3Error("precision must be one of %s" % sorted(PRECISIONS))
        self.precision = precision
        self.n = int(n_agents)
        self.stage = self._net_stage = int(stage)
        self.Lo = 2 * max(self.n - 1, 1)
        self.seed = int(seed)
        self.env_id_base = int(env_id_base)
        self.rows_draw = 0          # launch counter of the rows stream (sample_rows)
        shapes = checkers_policy_shapes(self.Lo)
        if self.stage == 1:
            for short in ("others_w", "others_b", "w_others_h2"):
                del shapes[short]
        self._load(weights, _PREFIXES, _CK_NAMES, shapes, "actor", lambda lib: lib.cm3_actor_checkers_packed_bytes(),
                   _lib.ActorCheckersWeights())

    def repack(self):
        d = self._desc(1, 0.0, 0, 75 * self.n)
        _lib.check(self._lib.cm3_actor_checkers_pack(ctypes.byref(d), ctypes.byref(self._wt), self._packed.data_ptr(),
                                                     self._stream(None)))

    def enqueue(self, n_envs, obs_self_t_raw, obst_stride, obs_self_v, obs_others, goals, actions_prev, steps, episode,
                actions, epsilon, probs=None, stream=None, env_id_base=None, prev_done=None):
        """Raw launch on the env's device buffers (obs_self_t_raw: the int8 storage with obst_stride bytes per env).
        prev_done (uint8 [E], optional): envs that finished an episode on the previous tick see actions_prev = 0."""
        self._enqueue_tick(self._lib.cm3_actor_checkers_f32, n_envs, obs_self_t_raw, obst_stride, obs_self_v, obs_others, goals,
                           actions_prev, steps, episode, actions, epsilon, probs, stream, env_id_base, prev_done)

    def enqueue_rollout(self, env_desc, traj, n_envs, obst_stride, n_ticks, epsilon, prev0=None, probs=None, stream=None,
                        final_obs=None, prev0_next=None):
        """The whole policy-driven rollout in ONE launch (cm3_policy_rollout_checkers): env_desc / traj are the env's descriptor and
        the rollout's trajectory struct; probs: optional float32 [T, E, N, 5]; final_obs: optional _lib.CheckersBufs naming the env's
        current-observation buffers, which then receive the state the rollout leaves."""
        self._enqueue_whole(self._lib.cm3_policy_rollout_checkers, env_desc, traj, n_envs, obst_stride, n_ticks, epsilon, prev0,
                            probs, stream, final_obs, prev0_next)

    def fused_rollout_ok(self, env):
        """cm3_policy_rollout_checkers covers the reference's configurations: split-float16 actor, one agent at stage 1 or two at
        stage 2, the 3 x 8 band with n_obs 2 -- and actor and env must share seed and env_id_base (one Philox key; otherwise
        collect() falls back to a launch pair per tick, whose actor launch takes its own key)."""
        same_key = (self.seed & 0xFFFFFFFFFFFFFFFF) == int(env._desc.seed) and self.env_id_base == int(env._desc.env_id_base)
        return (self.precision == "f16x3" and same_key and env.n == self.n and env.n in (1, 2) and (self.stage > 1) == (env.n > 1)
                and env.K == 5 and env.R == 3 and env.C == 8 and env.grid_stride % 4 == 0 and env.obst_stride % 4 == 0)

    def act(self, env, epsilon, actions_prev=None, return_probs=False):
        """Actions [E, N] int32 for the env's CURRENT observation (alg.run_actor); actions_prev None = zeros
        (train_onpolicy.py:295)."""
        if env.n != self.n:
            raise Cm3Error("actor built for %d agents, env has %d" % (self.n, env.n))
        if env.K != 5:
            raise Cm3Error("the device actor reads 5x5 windows (n_obs = 2)")
        s = env._slots[env._cur]
        prev = None
        if actions_prev is not None:
            prev = torch.as_tensor(actions_prev, device=self.device).to(torch.int32).reshape(env.E, env.n).contiguous()
        actions = torch.empty(env.E, env.n, dtype=torch.int32, device=self.device)
        probs = torch.empty(env.E, env.n, N_ACTIONS, dtype=torch.float32, device=self.device) if return_probs else None
        self.enqueue(env.E, s["obs_self_t_raw"], env.obst_stride, s["obs_self_v"], s["obs_others"], env._goals, prev,
                     env._steps, env._episode, actions, epsilon, probs, env_id_base=env._desc.env_id_base)
        return (actions, probs) if return_probs else actions

    # ---- the actor over the rows of a sampled batch (cm3_actor_checkers_rows_f32): the two evaluations of
    # alg_credit_checkers.train_step ----
    def enqueue_rows(self, n_rows, obs_self_t, obs_self_v, obs_others, actions_prev, goals, epsilon, probs=None, actions=None,
                     onehot=None, draw=0, row_id_base=0, stream=None):
        """Raw launch of cm3_actor_checkers_rows_f32 on contiguous device tensors: obs_self_t int8 or float64 [R, 75], obs_self_v /
        obs_others float64, actions_prev int32 [R], goals uint8 [R] or int64 [R, 2]; every output is optional, one is required.
        epsilon: a float, or a one-element float32 device tensor the launch reads itself.  (seed, row_id_base + row, draw) key the
        row's uniform; nothing is drawn when actions and onehot are both None.  draw: an integer, or a RowsDrawCounter -- then the
        launch is cm3_actor_checkers_rows_counted_f32, which reads the counter's device word and advances it itself."""
        if obs_self_t.dtype not in (torch.int8, torch.float64) or goals.dtype not in (torch.uint8, torch.int64):
            raise Cm3Error("enqueue_rows reads int8 or float64 windows and uint8 index or int64 one-hot goals, not %s / %s"
                           % (obs_self_t.dtype, goals.dtype))
        r = _lib.ActorCheckersRows()
        r.obs_self_t, r.obs_self_v, r.obs_others = _lib.ptr(obs_self_t), _lib.ptr(obs_self_v), _lib.ptr(obs_others)
        r.actions_prev, r.goals = _lib.ptr(actions_prev), _lib.ptr(goals)
        r.obs_self_t_f64 = 1 if obs_self_t.dtype == torch.float64 else 0
        r.goals_onehot = 1 if goals.dtype == torch.int64 else 0
        r.probs, r.actions, r.onehot = _lib.ptr(probs), _lib.ptr(actions), _lib.ptr(onehot)
        epsilon, r.epsilon_dev = _epsilon_args(epsilon)
        counter = draw if isinstance(draw, RowsDrawCounter) else None
        r.n_rows, r.row_id_base = int(n_rows), int(row_id_base) & 0xFFFFFFFFFFFFFFFF
        r.draw = 0 if counter is not None else int(draw) & 0xFFFFFFFF
        d = self._desc(1, epsilon, 0, 75 * self.n)
        s = self._stream(stream)
        if counter is not None:
            _lib.check(self._lib.cm3_actor_checkers_rows_counted_f32(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(r),
                                                                     counter.data_ptr(), s))
        else:
            _lib.check(self._lib.cm3_actor_checkers_rows_f32(ctypes.byref(d), ctypes.byref(self._wt), ctypes.byref(r), s))

    def probs_rows(self, obs_self_t, obs_self_v, obs_others, actions_prev, goals, epsilon, keep=None):
        """The mixed probabilities float32 [R, 5] over the R = prod(leading shape) rows, ONE launch: the reference's
        sess.run(self.probs, ...) of train_step (alg_credit_checkers.py:107-113) on the columns obs_self_t / obs_self_v / obs_others /
        actions_prev / goals of a sampled batch (input forms: stage_checkers_rows).  Nothing is drawn.  At precision "f16x3" float64
        windows must hold float16-exact values (the env's are -1 / 0 / 1).  A row's probabilities are the bits act() computes for
        the same inputs at the same precision.  keep: an optional list that receives every tensor this call allocated and the launch
        touches (the output, the staged inputs) -- whoever captures the launch into a hipGraph holds them while it is replayed."""
        rows, ot, ov, oo, ap, vg = stage_checkers_rows("probs_rows", self.device, self.Lo, obs_self_t, obs_self_v, obs_others,
                                                       actions_prev, goals)
        probs = torch.empty(rows, N_ACTIONS, dtype=torch.float32, device=self.device)
        _keep(keep, ot, ov, oo, ap, vg, probs)
        self.enqueue_rows(rows, ot, ov, oo, ap, vg, epsilon, probs=probs)
        return probs

    def sample_rows(self, obs_self_t, obs_self_v, obs_others, actions_prev, goals, epsilon, probs=False, onehot=False, draw=None,
                    keep=None):
        """Actions sampled from the mixed probabilities over transition rows, ONE launch: with the Policy_target weights this is
        action_samples_target of train_step (alg_credit_checkers.py:117, run_actor_target :255-260, called at :551) on
        next_obs_self_t / next_obs_self_v / next_obs_others / actions / goals (the reference feeds the action just taken as
        actions_prev there).  Returns a dict of device tensors: "actions" int32 [R] always; "probs" float32 [R, 5] and "onehot" int64
        [R, 5] when asked for.  The uniforms are the build's own rows stream keyed (seed, row, draw): draw=None takes the actor's
        counter self.rows_draw and advances it, so successive calls draw afresh; an explicit draw reproduces a call (and leaves the
        counter alone); a RowsDrawCounter makes the launch read and advance that counter on the device (capturable: every replay
        draws afresh; self.rows_draw is left alone).  keep: as probs_rows."""
        rows, ot, ov, oo, ap, vg = stage_checkers_rows("sample_rows", self.device, self.Lo, obs_self_t, obs_self_v, obs_others,
                                                       actions_prev, goals)
        out = sample_outputs(self.device, rows, probs, onehot)
        if draw is None:
            draw, self.rows_draw = self.rows_draw, (self.rows_draw + 1) & 0xFFFFFFFF
        _keep(keep, ot, ov, oo, ap, vg, *out.values())
        self.enqueue_rows(rows, ot, ov, oo, ap, vg, epsilon, draw=draw, **out)
        return out

