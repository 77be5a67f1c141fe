"""ParticleQmixAgent -- the QMIX baseline's per-agent Q network and its epsilon-greedy choice, evaluated on the device.

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
np.random calls, not the same numbers.  The mixer and the learner stay on the reference's side.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import Cm3Error
from .actor import _epsilon_args

H, N_ACTIONS = 64, 5
# the six tensors of cm3_qmix_particle_pack, in its order
NAMES = ("h/kernel", "h/bias", "h2/kernel", "h2/bias", "out/kernel", "out/bias")


def _canon(name):
    name = name.split(":")[0]
    for prefix in ("Agent_main/", "Agent_target/"):
        if name.startswith(prefix):
            name = name[len(prefix):]
    return name


class ParticleQmixAgent(object):
    # the one-launch episode and fused per-tick kernels run the CM3 actor: ParticleRollout keeps this agent on launch pairs
    fused_kernels = False

    def __init__(self, weights, n_agents, device="cuda:0", seed=12341, env_id_base=0):
        self.device = _lib.require_gpu(device)
        self.n = int(n_agents)
        if not 1 <= self.n <= _lib.MAX_AGENTS:
            raise Cm3Error("n_agents must be in 1..%d" % _lib.MAX_AGENTS)
        self.L = 4 * max(self.n - 1, 1)
        self.seed = int(seed)
        self.env_id_base = int(env_id_base)
        src = {_canon(k): v for k, v in weights.items()}
        shapes = {"h/kernel": (self.L + 6, H), "h/bias": (H,), "h2/kernel": (H, H), "h2/bias": (H,),
                  "out/kernel": (H, N_ACTIONS), "out/bias": (N_ACTIONS,)}
        self.w = {}
        for name in NAMES:
            if name not in src:
                raise Cm3Error("missing QMIX weight %r" % name)
            t = torch.as_tensor(np.asarray(src[name]), dtype=torch.float32).contiguous()
            if tuple(t.shape) != shapes[name]:
                raise Cm3Error("QMIX weight %r has shape %s, expected %s" % (name, tuple(t.shape), shapes[name]))
            self.w[name] = t.to(self.device)
        self._lib = _lib.lib()
        self._tensors = (ctypes.c_void_p * 6)(*[self.w[k].data_ptr() for k in NAMES])
        nbytes = self._lib.cm3_qmix_particle_packed_bytes(self.n)
        self._packed = torch.zeros(nbytes // 4, dtype=torch.float32, device=self.device)
        self.repack()

    def repack(self):
        """Re-arrange the (possibly updated in place) TF-shaped weights into the forward kernel's layout: after every update."""
        d = self._desc(1, 0.0, 0)
        _lib.check(self._lib.cm3_qmix_particle_pack(ctypes.byref(d), self._tensors, self._packed.data_ptr(),
                                                    _lib.current_stream_handle(self.device)))

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
        s = _lib.current_stream_handle(self.device) if stream is None else stream
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
