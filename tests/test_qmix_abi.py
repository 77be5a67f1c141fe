"""CPU: the QMIX agent's C ABI (ABI 9) -- declared, exported, bound, and every invalid argument refused with a readable error
before anything touches a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cm3_qmix_particle_packed_bytes", "cm3_qmix_particle_pack", "cm3_qmix_particle_f32", "cm3_qmix_particle_f64")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    return _lib


def test_header_declares_and_library_exports_the_qmix_entries(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cm3_amd.h")).read(), flags=re.S)
    handle = built.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(handle, name), name
        assert name in built.SYMBOLS, name
    assert built.ABI_VERSION == 9 and handle.cm3_abi_version() == 9


def test_packed_size_per_agent_count(built):
    handle = built.lib()
    sizes = [handle.cm3_qmix_particle_packed_bytes(n) for n in range(1, 11)]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert handle.cm3_qmix_particle_packed_bytes(0) == 0 and handle.cm3_qmix_particle_packed_bytes(11) == 0


def _desc(built, **kw):
    d = built.ActorParticleDesc()
    d.n_envs, d.n_agents, d.stage = 16, 4, 2
    d.n_h1_self, d.n_h1_others, d.n_h2, d.n_actions = 64, 0, 64, 5
    d.epsilon, d.precision = 0.1, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _bufs(built, **kw):
    b = built.ActorParticleBufs()
    for name in ("obs_others", "state", "goals", "meta", "episode", "actions"):
        setattr(b, name, 0x1000)               # never dereferenced: validation fails first
    for k, v in kw.items():
        setattr(b, k, v)
    return b


FAKE = 0x1000


@pytest.mark.parametrize("entry", ["cm3_qmix_particle_f32", "cm3_qmix_particle_f64"])
@pytest.mark.parametrize("field,value,needle", [
    ("n_agents", 0, b"n_agents"), ("n_agents", 11, b"n_agents"), ("n_envs", 0, b"n_envs"),
    ("n_h1_self", 128, b"64/64/5"), ("n_h2", 32, b"64/64/5"), ("n_actions", 4, b"64/64/5"),
    ("precision", 2, b"precision"), ("epsilon", -0.1, b"epsilon"), ("epsilon", 1.5, b"epsilon")])
def test_invalid_descriptor_is_refused_without_a_gpu(built, entry, field, value, needle):
    handle = built.lib()
    fn = getattr(handle, entry)
    assert fn(ctypes.byref(_desc(built, **{field: value})), FAKE, ctypes.byref(_bufs(built)), None) == -1
    assert needle in handle.cm3_last_error()


@pytest.mark.parametrize("entry", ["cm3_qmix_particle_f32", "cm3_qmix_particle_f64"])
def test_missing_packed_or_buffers_is_refused(built, entry):
    handle = built.lib()
    fn = getattr(handle, entry)
    d = _desc(built)
    assert fn(ctypes.byref(d), None, ctypes.byref(_bufs(built)), None) == -1
    assert b"packed" in handle.cm3_last_error()
    assert fn(ctypes.byref(d), FAKE, None, None) == -1
    assert b"bufs" in handle.cm3_last_error()
    for name in ("obs_others", "state", "goals", "meta", "episode", "actions"):
        assert fn(ctypes.byref(d), FAKE, ctypes.byref(_bufs(built, **{name: None})), None) == -1, name
        assert b"missing buffers" in handle.cm3_last_error()


def test_pack_validates_before_launching(built):
    handle = built.lib()
    tensors = (ctypes.c_void_p * 6)(*([FAKE] * 6))
    assert handle.cm3_qmix_particle_pack(ctypes.byref(_desc(built, n_agents=12)), tensors, FAKE, None) == -1
    assert b"n_agents" in handle.cm3_last_error()
    assert handle.cm3_qmix_particle_pack(ctypes.byref(_desc(built, n_h2=128)), tensors, FAKE, None) == -1
    assert b"64/64/5" in handle.cm3_last_error()
    assert handle.cm3_qmix_particle_pack(ctypes.byref(_desc(built)), tensors, None, None) == -1
    assert b"packed" in handle.cm3_last_error()
    holes = (ctypes.c_void_p * 6)(FAKE, FAKE, FAKE, None, FAKE, FAKE)
    assert handle.cm3_qmix_particle_pack(ctypes.byref(_desc(built)), holes, FAKE, None) == -1
    assert b"missing QMIX weight 3" in handle.cm3_last_error()
    assert handle.cm3_qmix_particle_pack(None, tensors, FAKE, None) == -1
    assert b"null desc" in handle.cm3_last_error()


def test_agent_refuses_a_cpu_device():
    from cm3_amd import Cm3Error
    from cm3_amd.qmix import ParticleQmixAgent
    with pytest.raises(Cm3Error):
        ParticleQmixAgent({}, 4, device="cpu")
