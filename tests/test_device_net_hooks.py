"""CPU: cm3_amd.rollout chooses a policy's launch path by duck typing -- hasattr(policy, "enqueue" / "act" / "enqueue_rollout" /
"enqueue_episode" / "stage") and getattr(policy, "precision" / "fused_kernels" / "episode_kernel" / "seed", ...) -- so a shared base
class must not give any of the seven weight-holding classes one of those names it does not have by itself.  This pins, per class,
which of the names the class defines and which its __init__ sets (read from the source: no instance exists without a GPU)."""
import ast
import inspect
import textwrap

import pytest

HOOKS = ("enqueue", "act", "enqueue_rollout", "enqueue_episode", "fused_rollout_ok", "episode_ok", "stage", "precision", "fused_kernels",
         "episode_kernel", "seed", "rows_draw")
#                        on the class                                                      set by __init__
TABLE = {
    "actor.ParticleActor": ({"enqueue", "act"}, {"stage", "precision", "seed", "rows_draw"}),
    "actor.CheckersActor": ({"enqueue", "act", "enqueue_rollout", "fused_rollout_ok"}, {"stage", "precision", "seed", "rows_draw"}),
    "critic.ParticleCritic": ({"enqueue"}, {"stage"}),
    "critic.CheckersCritic": ({"enqueue"}, {"stage"}),
    "qmix.ParticleQmixAgent": ({"enqueue", "act", "enqueue_episode", "episode_ok", "fused_kernels"}, {"episode_kernel", "seed"}),
    "qmix.CheckersQmixAgent": ({"enqueue", "act", "enqueue_episode", "episode_ok"}, {"precision", "seed"}),
    "qmix.ParticleQmixMixer": ({"enqueue"}, set()),
}


def _self_attributes(fn):
    """the names `self.<name>` that fn's source assigns"""
    names = set()
    for node in ast.walk(ast.parse(textwrap.dedent(inspect.getsource(fn)))):
        targets = node.targets if isinstance(node, ast.Assign) else [node.target] if isinstance(node, (ast.AugAssign, ast.AnnAssign)) else []
        for target in targets:
            for t in ast.walk(target):
                if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == "self":
                    names.add(t.attr)
    return names


@pytest.mark.parametrize("path", sorted(TABLE))
def test_hook_names_are_those_of_the_class_itself(path):
    import importlib
    module, name = path.split(".")
    cls = getattr(importlib.import_module("cm3_amd." + module), name)
    on_class, in_init = TABLE[path]
    assert {h for h in HOOKS if hasattr(cls, h)} == on_class
    set_by_init = set()
    for c in cls.__mro__:
        if c is not object and "__init__" in vars(c):
            set_by_init |= _self_attributes(vars(c)["__init__"])
    assert set_by_init & set(HOOKS) == in_init
    from cm3_amd._net import _DeviceNet
    assert issubclass(cls, _DeviceNet) and not {h for h in HOOKS if hasattr(_DeviceNet, h)}
    # the names every one of them keeps: weights, the library, the device, the agent count
    assert {"device", "n"} <= set_by_init and {"w", "_packed", "_lib"} <= _self_attributes(_DeviceNet._load)
    assert callable(cls.repack) and cls.soft_update_from is _DeviceNet.soft_update_from
