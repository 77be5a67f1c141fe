"""CPU: the float64 policy entry points (cm3_actor_particle_f64, cm3_policy_rollout_f64) are declared by include/cm3_amd.h,
exported by the library and bound by cm3_amd._lib with exactly the argument types of their float32 twins."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("cm3_actor_particle_f64", "cm3_actor_particle_f32"), ("cm3_policy_rollout_f64", "cm3_policy_rollout_f32")]


def _declaration(text, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text, flags=re.S)
    assert m, "include/cm3_amd.h does not declare %s" % name
    return " ".join(m.group(1).split())


@pytest.mark.parametrize("f64,f32", PAIRS)
def test_header_declares_the_f64_entry_with_the_f32_signature(f64, f32):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cm3_amd.h")).read(), flags=re.S)
    assert _declaration(text, f64) == _declaration(text, f32)


@pytest.mark.parametrize("f64,f32", PAIRS)
def test_binding_table_carries_the_f64_entry_like_its_twin(f64, f32):
    from cm3_amd import _lib
    assert f64 in _lib.SYMBOLS
    assert _lib.SYMBOLS[f64] == _lib.SYMBOLS[f32]


@pytest.mark.parametrize("f64,f32", PAIRS)
def test_library_exports_the_f64_entry(f64, f32):
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    handle = _lib.lib()
    assert hasattr(handle, f64) and hasattr(handle, f32)
    assert list(getattr(handle, f64).argtypes) == list(getattr(handle, f32).argtypes)
