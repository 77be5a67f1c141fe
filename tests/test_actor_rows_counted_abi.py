"""CPU: the C ABI of the COUNTED actor rows launches (part of ABI 9, additive) -- cm3_actor_particle_rows_counted_f32 and
cm3_actor_checkers_rows_counted_f32 declared, exported, bound; the ABI version and both rows structs unchanged; every check of the
uncounted entries fires first, in the same order and with the same message (the two-fault tables of tests/test_actor_rows_abi.py and
tests/test_actor_checkers_rows_abi.py, restated here), a null and then a misaligned draw_state rank last; nothing is launched on a
refusal (no GPU on the machine these run on: a launch would not return CM3_ERR_INVALID)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000                                      # 16-byte aligned, never dereferenced: validation fails first
STATE = 0x2000                                     # a well-formed draw_state, never dereferenced either
BIG = 64 * (2 ** 31 - 1) + 1
CK_INPUTS = ["obs_self_t", "obs_self_v", "obs_others", "actions_prev", "goals"]

# (desc fields, weights, rows fields or None for a null rows pointer, the message of the EARLIER of the two violated checks)
PARTICLE_TWO_FAULTS = [
    ({"n_h2": 32}, None, {}, b"64/128/64/5"),
    ({}, None, None, b"null weights"),
    ({"epsilon": 1.5}, "default", None, b"null rows"),
    ({"epsilon": 1.5, "precision": 3}, "default", {}, b"epsilon must be"),
    ({"precision": 3}, "unpacked", {}, b"precision must be"),
    ({}, "unpacked", {"goals": None}, b"weights->packed is NULL"),
    ({}, "default", {"goals": None, "actions": None}, b"missing inputs"),
    ({}, "default", {"actions": None, "n_rows": 0}, b"no output requested"),
    ({}, "default", {"n_rows": 0, "v_obs": FAKE + 4}, b"n_rows must be positive"),
    ({}, "default", {"n_rows": BIG, "v_obs": FAKE + 4}, b"more than a grid"),
    ({}, "default", {"v_obs": FAKE + 4, "onehot": FAKE + 8}, b"misaligned inputs")]
CHECKERS_TWO_FAULTS = [
    ({"n_agents": 0}, None, {}, b"n_agents"),
    ({}, None, None, b"null weights"),
    ({"precision": 3}, "default", None, b"null rows"),
    ({"precision": 3, "stage": 0}, "default", {}, b"precision must be"),
    ({"stage": 0, "epsilon": 1.5}, "default", {}, b"stage must be"),
    ({"epsilon": 1.5}, "unpacked", {}, b"epsilon must be"),
    ({}, "unpacked", {"goals": None}, b"weights->packed is NULL"),
    ({}, "default", {"goals": None, "actions": None}, b"missing inputs"),
    ({}, "default", {"actions": None, "n_rows": 0}, b"no output requested"),
    ({}, "default", {"n_rows": 0, "goals_onehot": 2}, b"n_rows must be positive"),
    ({}, "default", {"n_rows": BIG, "goals_onehot": 2}, b"more than a grid"),
    ({}, "default", {"goals_onehot": 2, "obs_self_v": FAKE + 8}, b"form flags"),
    ({}, "default", {"obs_self_v": FAKE + 8, "actions": FAKE + 2}, b"misaligned inputs")]
# the LAST check of each uncounted entry, violated alone: it still outranks a bad draw_state
LAST_UNCOUNTED = {"particle": ({"onehot": FAKE + 8}, b"misaligned onehot"), "checkers": ({"actions": FAKE + 2}, b"misaligned outputs")}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    return _lib


class _Env(object):
    """The two entries of one env and well-formed arguments for them."""

    def __init__(self, built, env):
        self.built, self.env = built, env
        self.counted = "cm3_actor_%s_rows_counted_f32" % env
        self.plain = "cm3_actor_%s_rows_f32" % env

    def desc(self, **kw):
        b = self.built
        if self.env == "particle":
            d = b.ActorParticleDesc()
            d.n_envs, d.n_agents, d.stage = 0, 4, 2
            d.n_h1_self, d.n_h1_others, d.n_h2, d.n_actions = 64, 128, 64, 5
        else:
            d = b.ActorCheckersDesc()
            d.n_envs, d.n_agents, d.stage, d.n_obs = 0, 2, 2, 2
            d.conv_f, d.n_conv_linear, d.n_h1, d.n_h2, d.n_actions = 6, 32, 256, 256, 5
        d.epsilon, d.precision, d.seed = 0.25, 0, 12341
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def weights(self, packed=FAKE):
        w = self.built.ActorParticleWeights() if self.env == "particle" else self.built.ActorCheckersWeights()
        w.packed = packed
        return w

    def rows(self, **kw):
        if self.env == "particle":
            r = self.built.ActorRows()
            r.obs_others, r.v_obs, r.goals = FAKE, FAKE, FAKE
        else:
            r = self.built.ActorCheckersRows()
            for name in CK_INPUTS:
                setattr(r, name, FAKE)
        r.actions, r.n_rows = FAKE, 100
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def call(self, entry, d, w, r, state):
        handle = self.built.lib()
        ref = lambda x: None if x is None else ctypes.byref(x)              # noqa: E731
        args = [ref(d), ref(w), ref(r)] + ([state] if entry == self.counted else []) + [None]
        rc = getattr(handle, entry)(*args)
        return rc, handle.cm3_last_error()


@pytest.fixture(params=["particle", "checkers"])
def env(request, built):
    return _Env(built, request.param)


def test_header_declares_and_library_exports_both_entries(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cm3_amd.h")).read(), flags=re.S)
    handle = built.lib()
    for entry in ("cm3_actor_particle_rows_counted_f32", "cm3_actor_checkers_rows_counted_f32"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % entry, text)
        assert m, entry
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == 5 and re.match(r"uint32_t\s*\*\s*draw_state$", params[3]) and re.match(r"void\s*\*\s*stream$", params[4]), params
        assert hasattr(handle, entry)
        assert entry in built.SYMBOLS and len(built.SYMBOLS[entry][1]) == 5


def test_abi_version_and_struct_sizes_are_unchanged(built):
    text = open(os.path.join(ROOT, "include", "cm3_amd.h")).read()
    assert built.ABI_VERSION == 9 and built.lib().cm3_abi_version() == 9
    assert re.search(r"#define\s+CM3_ABI_VERSION\s+9\b", text)
    assert ctypes.sizeof(built.ActorRows) == 80 and ctypes.sizeof(built.ActorCheckersRows) == 104


TWO_FAULTS = ([("particle",) + c for c in PARTICLE_TWO_FAULTS] + [("checkers",) + c for c in CHECKERS_TWO_FAULTS])


@pytest.mark.parametrize("state", [STATE, None, STATE + 4], ids=["state-ok", "state-null", "state-misaligned"])
@pytest.mark.parametrize("name,desc_kw,weights,rows_kw,needle", TWO_FAULTS,
                         ids=["%s-%d" % (c[0], i) for i, c in enumerate(TWO_FAULTS)])
def test_uncounted_checks_fire_first_in_their_order(built, name, desc_kw, weights, rows_kw, needle, state):
    """Every two-fault case of the uncounted entry: the same code and message through the counted entry as through the uncounted
    one, whatever draw_state is."""
    env = _Env(built, name)
    w = {None: None, "default": env.weights(), "unpacked": env.weights(packed=None)}[weights]
    r = None if rows_kw is None else env.rows(**rows_kw)
    rc_plain, msg_plain = env.call(env.plain, env.desc(**desc_kw), w, r, None)
    rc, msg = env.call(env.counted, env.desc(**desc_kw), w, r, state)
    assert rc == rc_plain == -1
    assert needle in msg and msg == msg_plain, (msg, msg_plain)


@pytest.mark.parametrize("state", [None, STATE + 4, STATE + 1], ids=["state-null", "state-plus-4", "state-plus-1"])
def test_last_uncounted_check_outranks_a_bad_draw_state(env, state):
    rows_kw, needle = LAST_UNCOUNTED[env.env]
    rc, msg = env.call(env.counted, env.desc(), env.weights(), env.rows(**rows_kw), state)
    assert rc == -1 and needle in msg, msg


def test_null_draw_state_is_refused_before_a_misaligned_one(env):
    """Everything else well-formed: NULL, then alignment (4-byte alignment is not enough: the words are an 8-byte pair).  On a
    machine without a GPU a launch would come back as CM3_ERR_HIP (-2), not as CM3_ERR_INVALID."""
    rc, msg = env.call(env.counted, env.desc(), env.weights(), env.rows(), None)
    assert rc == -1 and b"null draw_state" in msg, msg
    for off in (1, 2, 4, 12):
        rc, msg = env.call(env.counted, env.desc(), env.weights(), env.rows(), STATE + off)
        assert rc == -1 and b"misaligned draw_state" in msg and b"8-byte" in msg, (off, msg)


def test_probs_only_call_still_validates_draw_state(env):
    """(a probs-only launch does not touch the counter, but the entry's contract on its arguments does not depend on the outputs)"""
    rc, msg = env.call(env.counted, env.desc(), env.weights(), env.rows(actions=None, probs=FAKE), None)
    assert rc == -1 and b"null draw_state" in msg, msg


def test_python_side_takes_the_counter():
    import inspect
    from cm3_amd import actor, batch
    assert inspect.isclass(actor.RowsDrawCounter)
    for cls in (actor.ParticleActor, actor.CheckersActor):
        assert "keep" in inspect.signature(cls.sample_rows).parameters and "keep" in inspect.signature(cls.probs_rows).parameters
        assert "draw" in inspect.signature(cls.enqueue_rows).parameters
    p = inspect.signature(batch.train_step_feeds).parameters
    assert p["draw"].default is None and p["keep"].default is None
    p = inspect.signature(batch.OnPolicyPhasePlan.__init__).parameters
    assert [p[n].default for n in ("target_actor", "actor", "draw_counter")] == [None, None, None]
