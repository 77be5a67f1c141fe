"""What the twelve weight-holding classes share (ParticleActor / CheckersActor, ParticleCritic / CheckersCritic, ParticleQmixAgent /
CheckersQmixAgent, ParticleQmixMixer / CheckersQmixMixer, ParticleValue / ParticleComaCritic, CheckersValue / CheckersComaCritic): loading a dict of TF variables into ``self.w`` and the library's packed layout, the soft
update of a target copy, the stream default -- and the staging and output-allocation helpers more than one of them uses.

_DeviceNet defines NO launch hook: cm3_amd.rollout chooses its launch path by which of enqueue / act / enqueue_rollout /
enqueue_episode / stage / precision / fused_kernels / episode_kernel / seed a policy has, so those names stay with the classes that
have them (tests/test_device_net_hooks.py pins the table).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import Cm3Error

N_ACTIONS = 5


def _keep(keep, *tensors):
    """Appends the tensors a launch touches to the caller's keep list (None: nobody captures, nothing to do)."""
    if keep is not None:
        keep.extend(t for t in tensors if t is not None)


def canon(name, prefixes):
    """The TF variable name without its ":0" suffix and scope prefix."""
    name = name.split(":")[0]
    for prefix in prefixes:
        if name.startswith(prefix):
            name = name[len(prefix):]
    return name


class _DeviceNet(object):
    _match = ("n",)         # the attributes a soft_update_from partner must share
    _refusal = ""           # the words of the refusal, %-formatted with those attributes by name

    def _load(self, weights, prefixes, names, shapes, label, packed_bytes, wt=None, fields=None):
        """weights (keyed by TF variable names) -> ``self.w`` (float32 device tensors of `shapes`, under its short names; `names`
        maps a short name to the TF one), the pointers of the library's weights struct `wt` (fields: short name -> field, default
        the short names of `names`; a tensor the class does not have is a null pointer), ``self._packed`` of packed_bytes(lib)
        bytes, and the first repack().  wt=None: no struct -- ``self._tensors`` is the array of self.w's pointers, in order."""
        src = {canon(k, prefixes): v for k, v in weights.items()}
        self.w = {}
        for short, shape in shapes.items():
            name = names[short]
            if name not in src:
                raise Cm3Error("missing %s weight %r" % (label, name))
            t = torch.as_tensor(np.asarray(src[name]), dtype=torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise Cm3Error("%s weight %r has shape %s, expected %s" % (label, name, tuple(t.shape), shape))
            self.w[short] = t.to(self.device)
        if wt is None:
            self._tensors = (ctypes.c_void_p * len(self.w))(*[t.data_ptr() for t in self.w.values()])
        else:
            self._wt = wt
            for short, field in (fields or {s: s for s in names}).items():
                setattr(wt, field, _lib.ptr(self.w.get(short)))
        self._lib = _lib.lib()
        self._packed = torch.zeros(packed_bytes(self._lib) // 4, dtype=torch.float32, device=self.device)
        if wt is not None:
            wt.packed = self._packed.data_ptr()
        self.repack()

    def _stream(self, stream):
        return _lib.current_stream_handle(self.device) if stream is None else stream

    def soft_update_from(self, main, tau):
        """w <- tau * main.w + (1 - tau) * w on the TF-shaped float32 tensors in place, then repack(): this network's part of the
        reference's list_update_target_ops, for an object holding the target weights.  main: an object of the same class that
        agrees in self._match."""
        if not isinstance(main, type(self)) or any(getattr(main, a) != getattr(self, a) for a in self._match):
            raise Cm3Error("soft_update_from: " + self._refusal % {a: getattr(self, a) for a in self._match})
        tau = float(tau)
        for name in self.w:
            # float32 throughout, as TF evaluates tau * var + (1 - tau) * target with float32 constants
            self.w[name].copy_(tau * main.w[name].to(self.device) + (1.0 - tau) * self.w[name])
        self.repack()


def stage_particle_rows(what, device, L, obs_others, v_obs, goals):
    """(rows, obs_others, v_obs, goals) contiguous float32 on `device` from [..., L], [..., 4], [..., 2] with equal leading shape (a
    float64 column is rounded, as the reference's tf.float32 placeholders do)."""
    lead = tuple(v_obs.shape[:-1])
    if (tuple(obs_others.shape) != lead + (L,) or tuple(v_obs.shape) != lead + (4,)
            or tuple(goals.shape) != lead + (2,)):
        raise Cm3Error("%s takes [..., %d], [..., 4] and [..., 2] with equal leading shape, got %s, %s, %s"
                       % (what, L, tuple(obs_others.shape), tuple(v_obs.shape), tuple(goals.shape)))
    rows = int(np.prod(lead, dtype=np.int64))
    if rows <= 0:
        raise Cm3Error("%s needs at least one row" % what)
    stage = lambda t: t.to(device=device, dtype=torch.float32).contiguous()      # noqa: E731
    return rows, stage(obs_others), stage(v_obs), stage(goals)


def stage_td_cols(what, device, B, N, actions=None, reward=None, done=None, reward_name="reward"):
    """(actions, reward, done) of B time steps of N agents, contiguous on `device` in the forms the rows kernels read: actions [B, N]
    int32; reward [B, N] float32 or float64 (another dtype is widened to float64); done [B] uint8 (from bool or integers).  None
    stays None."""
    if actions is not None:
        if actions.numel() != B * N:
            raise Cm3Error("%s takes actions [B, %d] for %d time steps, got %s" % (what, N, B, tuple(actions.shape)))
        actions = actions.to(device=device, dtype=torch.int32).contiguous()
    if reward is not None:
        if reward.numel() != B * N:
            raise Cm3Error("%s takes %s [B, %d] for %d time steps, got %s" % (what, reward_name, N, B, tuple(reward.shape)))
        reward = reward.to(device=device, dtype=reward.dtype if reward.dtype == torch.float32 else torch.float64).contiguous()
    if done is not None:
        if done.numel() != B:
            raise Cm3Error("%s takes done [B] for %d time steps, got %s" % (what, B, tuple(done.shape)))
        done = done.reshape(-1).to(device)
        done = (done.contiguous().view(torch.uint8) if done.dtype == torch.bool else (done != 0).view(torch.uint8))
    return actions, reward, done


def td_given(what, reward_name, reward, done, gamma):
    """Whether a Q launch also computes the TD target: reward, done and gamma are all given (True) or all None (False)."""
    given = [x is not None for x in (reward, done, gamma)]
    if any(given) and not all(given):
        raise Cm3Error("%s: %s, done and gamma come together (the TD target) or not at all" % (what, reward_name))
    return all(given)


def td_outputs(device, rows, name, td):
    """The output dict of a Q launch over `rows` rows: `name` float32 [rows, 1], `name`64 float64 [rows, 1], with td "td" float64 [rows]."""
    out = {name: torch.empty(rows, 1, dtype=torch.float32, device=device),
           name + "64": torch.empty(rows, 1, dtype=torch.float64, device=device)}
    if td:
        out["td"] = torch.empty(rows, dtype=torch.float64, device=device)
    return out


def _rows_outputs(device, rows, always, optional):
    out = {always: torch.empty(rows, dtype=torch.int32, device=device)}
    for name, (asked, shape, dtype) in optional.items():
        if asked:
            out[name] = torch.empty((rows,) + shape, dtype=dtype, device=device)
    return out


def sample_outputs(device, rows, probs, onehot):
    """The output dict of sample_rows: "actions" int32 [rows]; "probs" float32 [rows, 5] and "onehot" int64 [rows, 5] when asked for."""
    return _rows_outputs(device, rows, "actions", {"probs": (probs, (N_ACTIONS,), torch.float32),
                                                   "onehot": (onehot, (N_ACTIONS,), torch.int64)})


def greedy_outputs(device, rows, q, onehot, q_max):
    """The output dict of greedy_rows: "argmax" int32 [rows]; "q" float32 [rows, 5], "onehot" int64 [rows, 5] and "q_max" float32
    [rows] when asked for."""
    return _rows_outputs(device, rows, "argmax", {"q": (q, (N_ACTIONS,), torch.float32), "onehot": (onehot, (N_ACTIONS,), torch.int64),
                                                  "q_max": (q_max, (), torch.float32)})
