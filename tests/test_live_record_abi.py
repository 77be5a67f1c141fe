"""CPU: the argument checks around cm3_particle_traj.live_record -- which descriptors packed live records apply to
(cm3_particle_live_record_applies) and that cm3_particle_rollout_* refuses a record for every other descriptor BEFORE it launches
anything, on the fused path too (no GPU needed: the checks come first)."""
import ctypes

import pytest

from cm3_amd import _lib

GEN, FUSED = _lib.FLAG_GEN_ACTIONS, _lib.FLAG_FUSED_TICKS
PAIR, AGENT, ENV = _lib.FLAG_KERNEL_LANE_PER_PAIR, _lib.FLAG_KERNEL_LANE_PER_AGENT, _lib.FLAG_KERNEL_LANE_PER_ENV


def _desc(n_agents, n_envs, flags):
    d = _lib.ParticleDesc()
    d.n_envs, d.n_agents, d.max_steps, d.flags = n_envs, n_agents, 33, flags
    return d


@pytest.mark.parametrize("n,e,flags,real,want", [
    (4, 4096, GEN, 4, 1), (2, 32768, GEN, 4, 1), (3, 24576, GEN, 4, 1), (4, 12288, GEN, 4, 1),
    (4, 12289, GEN, 4, 0), (4, 12289, GEN | PAIR, 4, 1),          # above the pair range: only a forced pair mapping
    (4, 4096, GEN, 8, 0), (5, 4096, GEN, 4, 0), (1, 4096, GEN, 4, 0),
    (4, 4096, 0, 4, 0), (4, 4096, GEN | FUSED, 4, 0), (4, 4096, GEN | AGENT, 4, 0), (4, 4096, GEN | ENV, 4, 0),
    (2, 1 << 25, GEN | PAIR, 4, 0),                               # 32-bit byte offsets into the record array
    # a forced pair mapping whose obs_others reaches 4 GiB (N = 4: from 22 369 622 envs): the record applies where every record
    # condition holds -- the launch then names the limit -- and nowhere else
    (4, 23000000, GEN | PAIR, 4, 1), (4, 23000000, PAIR, 4, 0), (4, 23000000, GEN | PAIR | FUSED, 4, 0), (4, 23000000, GEN | PAIR, 8, 0),
    (8, 23000000, GEN | PAIR, 4, 0), (5, 23000000, GEN | PAIR, 4, 0), (4, 34000000, GEN | PAIR, 4, 0), (3, 100000000, GEN | PAIR, 4, 0),
    (4, 23000000, GEN, 4, 0), (4, 4096, GEN | PAIR | ENV, 4, 0),
])
def test_live_record_applies(n, e, flags, real, want):
    assert _lib.lib().cm3_particle_live_record_applies(ctypes.byref(_desc(n, e, flags)), real) == want


@pytest.mark.parametrize("n,flags,fn", [(5, GEN, "cm3_particle_rollout_f32"), (4, GEN | FUSED, "cm3_particle_rollout_f32"),
                                        (4, GEN, "cm3_particle_rollout_f64"), (4, GEN | FUSED, "cm3_particle_rollout_f64")])
def test_rollout_refuses_a_record_it_cannot_use(n, flags, fn, e=64):
    h = _lib.lib()
    t = _lib.ParticleTraj()
    for name in ("state", "goals", "obs_others", "actions", "reward_n", "reward", "done", "meta", "episode", "state_live",
                 "goals_live", "live_record"):
        setattr(t, name, 0x1000)          # never dereferenced: the call fails on its arguments
    t.state_stride = t.goals_stride = 64
    rc = getattr(h, fn)(ctypes.byref(_desc(n, e, flags)), ctypes.byref(t), 2, None)
    assert rc == -1 and b"live_record" in h.cm3_last_error()
    assert e == 64 or b"live_record does not apply" in h.cm3_last_error()


@pytest.mark.parametrize("n,flags,fn", [(5, GEN, "cm3_particle_rollout_f32"), (4, GEN | FUSED, "cm3_particle_rollout_f32"),
                                        (4, GEN, "cm3_particle_rollout_f64"), (4, 0, "cm3_particle_rollout_f32"),
                                        (8, GEN, "cm3_particle_rollout_f32")])
def test_rollout_refuses_such_a_record_beyond_4_gib_before_any_launch_too(n, flags, fn):
    """a forced pair mapping whose obs_others reaches 4 GiB: the record is refused first, by name, not the size by the launch"""
    test_rollout_refuses_a_record_it_cannot_use(n, flags | PAIR, fn, e=23000000)
