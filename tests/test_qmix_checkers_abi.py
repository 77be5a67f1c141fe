"""CPU: the Checkers QMIX agent's C ABI (additive part of ABI 9) -- declared, exported, bound, and every invalid argument refused
with a readable error before anything touches a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cm3_qmix_checkers_pack", "cm3_qmix_checkers_f32")
FAKE = 0x1000                                   # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    return _lib


def test_header_declares_and_library_exports_the_entries(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cm3_amd.h")).read(), flags=re.S)
    handle = built.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(handle, name), name
        assert name in built.SYMBOLS, name
    assert built.ABI_VERSION == 9 and handle.cm3_abi_version() == 9


def _desc(built, **kw):
    d = built.ActorCheckersDesc()
    d.n_envs, d.n_agents, d.stage, d.n_obs = 16, 2, 2, 2
    d.conv_f, d.n_conv_linear, d.n_h1, d.n_h2, d.n_actions = 6, 32, 256, 256, 5
    d.epsilon, d.precision = 0.1, 0
    d.obs_self_t_stride = 152
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _weights(built, **kw):
    w = built.ActorCheckersWeights()
    for name, _ in w._fields_:
        setattr(w, name, FAKE)
    for k, v in kw.items():
        setattr(w, k, v)
    return w


BUFS = ("obs_self_t", "obs_self_v", "obs_others", "goals", "steps", "episode", "actions")


def _bufs(built, **kw):
    b = built.ActorCheckersBufs()
    for name in BUFS:
        setattr(b, name, FAKE)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


@pytest.mark.parametrize("field,value,needle", [
    ("n_agents", 0, b"n_agents"), ("n_agents", 9, b"n_agents"), ("n_envs", 0, b"n_envs"),
    ("conv_f", 3, b"widths"), ("n_conv_linear", 64, b"widths"), ("n_h1", 64, b"widths"), ("n_h2", 128, b"widths"),
    ("n_actions", 4, b"widths"), ("n_obs", 3, b"n_obs"),
    ("precision", 1, b"precision"), ("precision", 3, b"precision"), ("precision", -1, b"precision"),
    ("epsilon", -0.1, b"epsilon"), ("epsilon", 1.5, b"epsilon"),
    ("obs_self_t_stride", 149, b"obs_self_t_stride")])
def test_invalid_descriptor_is_refused_without_a_gpu(built, field, value, needle):
    handle = built.lib()
    rc = handle.cm3_qmix_checkers_f32(ctypes.byref(_desc(built, **{field: value})), ctypes.byref(_weights(built)),
                                      ctypes.byref(_bufs(built)), None)
    assert rc == -1
    assert needle in handle.cm3_last_error(), handle.cm3_last_error()


def test_bf16_is_refused_with_the_reason(built):
    handle = built.lib()
    assert handle.cm3_qmix_checkers_f32(ctypes.byref(_desc(built, precision=1)), ctypes.byref(_weights(built)),
                                        ctypes.byref(_bufs(built)), None) == -1
    assert b"argmax" in handle.cm3_last_error()


def test_missing_packed_or_buffers_is_refused(built):
    handle = built.lib()
    fn = handle.cm3_qmix_checkers_f32
    d = _desc(built)
    assert fn(ctypes.byref(d), ctypes.byref(_weights(built, packed=None)), ctypes.byref(_bufs(built)), None) == -1
    assert b"packed" in handle.cm3_last_error()
    assert fn(ctypes.byref(d), None, ctypes.byref(_bufs(built)), None) == -1
    assert b"null weights" in handle.cm3_last_error()
    assert fn(ctypes.byref(d), ctypes.byref(_weights(built)), None, None) == -1
    assert b"bufs" in handle.cm3_last_error()
    assert fn(None, ctypes.byref(_weights(built)), ctypes.byref(_bufs(built)), None) == -1
    assert b"null desc" in handle.cm3_last_error()
    for name in BUFS:
        assert fn(ctypes.byref(d), ctypes.byref(_weights(built)), ctypes.byref(_bufs(built, **{name: None})), None) == -1, name
        assert b"missing buffers" in handle.cm3_last_error()


@pytest.mark.parametrize("n_agents", [1, 2])
def test_pack_requires_the_others_branch_at_every_agent_count(built, n_agents):
    handle = built.lib()
    for name in ("others_w", "others_b", "w_others_h2"):
        for stage in (1, 2):                   # desc->stage is not read
            d = _desc(built, n_agents=n_agents, stage=stage)
            assert handle.cm3_qmix_checkers_pack(ctypes.byref(d), ctypes.byref(_weights(built, **{name: None})), FAKE, None) == -1
            assert b"others branch" in handle.cm3_last_error(), name


def test_pack_validates_before_launching(built):
    handle = built.lib()
    pack = handle.cm3_qmix_checkers_pack
    assert pack(ctypes.byref(_desc(built, n_agents=9)), ctypes.byref(_weights(built)), FAKE, None) == -1
    assert b"n_agents" in handle.cm3_last_error()
    assert pack(ctypes.byref(_desc(built, n_h1=64)), ctypes.byref(_weights(built)), FAKE, None) == -1
    assert b"widths" in handle.cm3_last_error()
    assert pack(ctypes.byref(_desc(built, n_obs=1)), ctypes.byref(_weights(built)), FAKE, None) == -1
    assert b"n_obs" in handle.cm3_last_error()
    assert pack(ctypes.byref(_desc(built)), ctypes.byref(_weights(built)), None, None) == -1
    assert b"packed" in handle.cm3_last_error()
    assert pack(ctypes.byref(_desc(built)), ctypes.byref(_weights(built, out_w=None)), FAKE, None) == -1
    assert b"missing weights" in handle.cm3_last_error()
    assert pack(None, ctypes.byref(_weights(built)), FAKE, None) == -1
    assert b"null desc" in handle.cm3_last_error()


@pytest.mark.parametrize("entry", ["cm3_qmix_checkers_pack", "cm3_actor_checkers_pack"])
@pytest.mark.parametrize("desc_kw,weights_kw,packed,needle", [
    ({"n_obs": 1}, {}, None, b"n_obs"),
    ({}, {"out_w": None}, None, b"null weights / packed buffer"),
    ({}, {"out_w": None, "others_w": None}, FAKE, b"missing weights")])
def test_pack_checks_fire_in_their_order(built, entry, desc_kw, weights_kw, packed, needle):
    """Two consecutive checks violated at once, in both Checkers pack entries: the earlier one's message is the one reported."""
    handle = built.lib()
    assert getattr(handle, entry)(ctypes.byref(_desc(built, **desc_kw)), ctypes.byref(_weights(built, **weights_kw)), packed, None) == -1
    assert needle in handle.cm3_last_error(), handle.cm3_last_error()


def test_agent_refuses_a_cpu_device_and_bf16():
    from cm3_amd import Cm3Error
    from cm3_amd.qmix import CheckersQmixAgent
    with pytest.raises(Cm3Error, match="no CPU fallback"):
        CheckersQmixAgent({}, 2, device="cpu")
    with pytest.raises(Cm3Error, match="bf16"):
        CheckersQmixAgent({}, 2, device="cpu", precision="bf16")


def test_agent_is_exported_lazily():
    import cm3_amd
    from cm3_amd.qmix import CheckersQmixAgent
    assert cm3_amd.CheckersQmixAgent is CheckersQmixAgent
    assert not hasattr(CheckersQmixAgent, "enqueue_rollout") and not hasattr(CheckersQmixAgent, "fused_rollout_ok")
