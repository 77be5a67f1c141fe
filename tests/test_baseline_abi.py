"""CPU: the C ABI of the IAC / COMA baseline critics over transition rows (part of ABI 9, additive) -- cm3_value_particle_packed_bytes /
_pack / _rows_f32 and cm3_coma_particle_packed_bytes / _pack / _rows_f32 declared, exported, bound; the six structs' layout as a C
compiler sees it; every invalid argument refused with a readable error, in the stated order, before anything touches a GPU (fake
pointers: no launch happens)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cm3_value_particle_packed_bytes", "cm3_value_particle_pack", "cm3_value_particle_rows_f32",
           "cm3_coma_particle_packed_bytes", "cm3_coma_particle_pack", "cm3_coma_particle_rows_f32")
FAKE = 0x1000                                      # 16-byte aligned, never dereferenced: validation fails first
LOCAL, GLOBAL = 0, 1


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
    assert re.search(r"#define\s+CM3_ABI_VERSION\s+9\b", text)
    for name, value in (("CM3_VALUE_LOCAL", 0), ("CM3_VALUE_GLOBAL", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    assert (built.VALUE_LOCAL, built.VALUE_GLOBAL) == (0, 1)


def test_struct_layouts_match_the_header(built, tmp_path):
    structs = {"cm3_value_particle_desc": built.ValueParticleDesc, "cm3_value_particle_weights": built.ValueParticleWeights,
               "cm3_value_rows": built.ValueRows, "cm3_coma_particle_desc": built.ComaParticleDesc,
               "cm3_coma_particle_weights": built.ComaParticleWeights, "cm3_coma_rows": built.ComaRows}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cm3_amd.h"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        c, f, v = line.split()
        got[(c, f)] = int(v)
    for cname, cls in structs.items():
        assert ctypes.sizeof(cls) == got[(cname, "size")], cname
        for fname, _ in cls._fields_:
            assert getattr(cls, fname).offset == got[(cname, fname)], (cname, fname)
    assert [f for f, _ in built.ValueRows._fields_] == ["reward_f64", "reserved", "state", "obs_others", "goals", "reward", "done",
                                                         "gamma", "v", "v64", "td", "n_steps"]
    assert [f for f, _ in built.ComaRows._fields_] == ["reward_f64", "reserved", "state", "goals", "v_obs", "actions", "own_actions",
                                                        "reward", "done", "gamma", "q", "q_taken", "q_taken64", "td", "n_steps"]
    assert [f for f, _ in built.ComaParticleWeights._fields_] == ["w_h1", "b_h1", "w_h2", "b_h2", "w_out", "b_out", "packed"]


def test_packed_bytes(built):
    fv, fq = built.lib().cm3_value_particle_packed_bytes, built.lib().cm3_coma_particle_packed_bytes
    for n in range(1, 11):
        for kind in (LOCAL, GLOBAL):
            assert fv(n, kind) > 0 and fv(n, kind) % 16 == 0
        assert (fq(n) > 0) == (n > 1) and fq(n) % 16 == 0
    # branch 1 [4][64][4] + bias 64, h2 [4][64][16], out [64][16] at one agent -- either kind
    assert fv(1, LOCAL) == fv(1, GLOBAL) == 4 * (1024 + 64 + 4096 + 1024)
    # + branch 2 [4][2][64][S2P] + bias 128 and 48 k-steps of h2: local K2 = 12 -> 3 k-steps -> stride 4, global 18 -> 5 -> 8
    assert fv(4, LOCAL) == 4 * (1024 + 64 + 512 * 4 + 128 + 4 * 64 * 48 + 1024)
    assert fv(4, GLOBAL) == 4 * (1024 + 64 + 512 * 8 + 128 + 4 * 64 * 48 + 1024)
    # h1 [16][64][S0P] + 256, h2 [16][64][64] + 256, out [64][64] + 16: K = 47 -> 12 k-steps -> 12; K = 119 -> 30 -> 32
    assert fq(4) == 4 * (1024 * 12 + 256 + 65536 + 256 + 4096 + 16)
    assert fq(10) == 4 * (1024 * 32 + 256 + 65536 + 256 + 4096 + 16)
    for n, kind in ((0, LOCAL), (11, GLOBAL), (4, 2), (4, -1)):
        assert fv(n, kind) == 0
    for n in (-1, 0, 1, 11):
        assert fq(n) == 0


def _fill(struct, **kw):
    for k, v in kw.items():
        setattr(struct, k, v)
    return struct


def _vdesc(built, **kw):
    d = built.ValueParticleDesc()
    d.n_agents, d.stage, d.kind, d.n_h1, d.n_others, d.n_h2 = 4, 2, LOCAL, 64, 128, 64
    return _fill(d, **kw)


def _qdesc(built, **kw):
    d = built.ComaParticleDesc()
    d.n_agents, d.units = 4, 256
    return _fill(d, **kw)


def _weights(cls, **kw):
    w = cls()
    for f, _ in cls._fields_:
        setattr(w, f, FAKE)
    return _fill(w, **kw)


def _vrows(built, **kw):
    r = built.ValueRows()
    r.state, r.obs_others, r.goals, r.v, r.n_steps, r.gamma = FAKE, FAKE, FAKE, FAKE, 100, 0.99
    return _fill(r, **kw)


def _qrows(built, **kw):
    r = built.ComaRows()
    r.state, r.goals, r.v_obs, r.actions, r.q, r.n_steps, r.gamma = FAKE, FAKE, FAKE, FAKE, FAKE, 100, 0.99
    return _fill(r, **kw)


def _refused(built, needle, which, desc="default", weights="default", rows="default"):
    handle = built.lib()
    if which == "value":
        fn, d0, w0, r0 = handle.cm3_value_particle_rows_f32, _vdesc(built), _weights(built.ValueParticleWeights), _vrows(built)
    else:
        fn, d0, w0, r0 = handle.cm3_coma_particle_rows_f32, _qdesc(built), _weights(built.ComaParticleWeights), _qrows(built)
    d, w, r = (d0 if desc == "default" else desc), (w0 if weights == "default" else weights), (r0 if rows == "default" else rows)
    ref = lambda x: None if x is None else ctypes.byref(x)      # noqa: E731
    assert fn(ref(d), ref(w), ref(r), None) == -1
    assert needle in handle.cm3_last_error(), handle.cm3_last_error()


def test_null_arguments_are_refused(built):
    for which, wcls in (("value", built.ValueParticleWeights), ("coma", built.ComaParticleWeights)):
        _refused(built, b"null desc", which, desc=None)
        _refused(built, b"null weights", which, weights=None)
        _refused(built, b"null rows", which, rows=None)
        _refused(built, b"packed weights are NULL", which, weights=_weights(wcls, packed=None))


@pytest.mark.parametrize("kw,needle", [
    ({"n_agents": 0}, b"n_agents must be in 1..10"), ({"n_agents": 11}, b"n_agents must be in 1..10"),
    ({"kind": 2}, b"kind must be"), ({"kind": -1}, b"kind must be"), ({"stage": 0}, b"stage must be 1 or 2"),
    ({"stage": 3}, b"stage must be 1 or 2"),
    ({"stage": 1}, b"V_particle_local runs at stage 1 with one agent"),
    ({"kind": GLOBAL, "n_agents": 1}, b"V_particle_global runs at stage 1 with one agent"),
    ({"n_h1": 128}, b"64/128/64"), ({"n_others": 64}, b"64/128/64"), ({"n_h2": 32}, b"64/128/64")])
def test_invalid_value_descriptor_is_refused_without_a_gpu(built, kw, needle):
    _refused(built, needle, "value", desc=_vdesc(built, **kw))
    handle = built.lib()
    assert handle.cm3_value_particle_pack(ctypes.byref(_vdesc(built, **kw)), ctypes.byref(_weights(built.ValueParticleWeights)), FAKE,
                                          None) == -1
    assert needle in handle.cm3_last_error()


@pytest.mark.parametrize("kw,needle", [
    ({"n_agents": 1}, b"n_agents must be in 2..10"), ({"n_agents": 0}, b"n_agents must be in 2..10"),
    ({"n_agents": 11}, b"n_agents must be in 2..10"), ({"units": 128}, b"width is 256")])
def test_invalid_coma_descriptor_is_refused_without_a_gpu(built, kw, needle):
    _refused(built, needle, "coma", desc=_qdesc(built, **kw))
    handle = built.lib()
    assert handle.cm3_coma_particle_pack(ctypes.byref(_qdesc(built, **kw)), ctypes.byref(_weights(built.ComaParticleWeights)), FAKE,
                                         None) == -1
    assert needle in handle.cm3_last_error()


def test_the_descriptor_is_checked_before_the_other_arguments(built):
    _refused(built, b"n_agents must be in 1..10", "value", desc=_vdesc(built, n_agents=0), weights=None, rows=None)
    _refused(built, b"n_agents must be in 2..10", "coma", desc=_qdesc(built, n_agents=1), weights=None, rows=None)


@pytest.mark.parametrize("which,n_steps", [("value", 0), ("value", -5), ("value", (2 ** 31 - 1) // 4 + 1), ("value", 2 ** 40),
                                           ("coma", 0), ("coma", (2 ** 31 - 1) // 4 + 1)])
def test_row_count_out_of_range_is_refused(built, which, n_steps):
    rows = _vrows(built, n_steps=n_steps) if which == "value" else _qrows(built, n_steps=n_steps)
    _refused(built, b"n_steps", which, rows=rows)


def test_value_refusals_fire_in_the_stated_order(built):
    """n_steps, inputs, outputs, td's inputs, alignment of inputs / reward / outputs / packed: each call breaks one rule and every
    LATER one, and the earlier rule is the one reported"""
    bad_packed = _weights(built.ValueParticleWeights, packed=FAKE + 8)
    V = lambda **kw: _vrows(built, **kw)      # noqa: E731
    _refused(built, b"n_steps must be positive", "value", weights=bad_packed, rows=V(n_steps=0, state=None, v=None))
    for name in ("state", "goals"):
        _refused(built, b"missing inputs: state and goals", "value", weights=bad_packed, rows=V(v=None, **{name: None}))
    _refused(built, b"reads obs_others at stage 2", "value", weights=bad_packed, rows=V(obs_others=None, v=None))
    _refused(built, b"no output requested", "value", weights=bad_packed, rows=V(v=None, state=FAKE + 4))
    _refused(built, b"td needs reward and done", "value", weights=bad_packed, rows=V(td=FAKE, done=FAKE, state=FAKE + 4))
    _refused(built, b"td needs reward and done", "value", weights=bad_packed, rows=V(td=FAKE, reward=FAKE, state=FAKE + 4))
    for name, ptr in (("state", FAKE + 8), ("goals", FAKE + 4), ("obs_others", FAKE + 8)):
        _refused(built, b"misaligned inputs", "value", weights=bad_packed, rows=V(td=FAKE, done=FAKE, reward=FAKE + 2, **{name: ptr}))
    _refused(built, b"misaligned reward", "value", weights=bad_packed, rows=V(td=FAKE, done=FAKE, reward=FAKE + 2, v=FAKE + 2))
    _refused(built, b"misaligned reward", "value", rows=V(td=FAKE, done=FAKE, reward=FAKE + 4, reward_f64=1))
    for kw in ({"v": FAKE + 2}, {"v64": FAKE + 4}, {"td": FAKE + 4, "done": FAKE, "reward": FAKE}):
        _refused(built, b"misaligned outputs", "value", weights=bad_packed, rows=V(**kw))
    _refused(built, b"misaligned packed", "value", weights=bad_packed)
    # a global network reads no obs_others, a local one at stage 1 neither: without it they pass that check and fail a later one
    _refused(built, b"misaligned packed", "value", desc=_vdesc(built, kind=GLOBAL), weights=bad_packed, rows=V(obs_others=None))
    _refused(built, b"misaligned packed", "value", desc=_vdesc(built, n_agents=1, stage=1), weights=bad_packed,
             rows=V(obs_others=FAKE + 2))


def test_coma_refusals_fire_in_the_stated_order(built):
    bad_packed = _weights(built.ComaParticleWeights, packed=FAKE + 8)
    Q = lambda **kw: _qrows(built, **kw)      # noqa: E731
    _refused(built, b"n_steps must be positive", "coma", weights=bad_packed, rows=Q(n_steps=0, state=None, q=None))
    for name in ("state", "goals", "v_obs"):
        _refused(built, b"missing inputs: state, goals and v_obs", "coma", weights=bad_packed, rows=Q(actions=None, **{name: None}))
    _refused(built, b"reads the actions of the others", "coma", weights=bad_packed, rows=Q(actions=None, q=None))
    _refused(built, b"no output requested", "coma", weights=bad_packed, rows=Q(q=None, state=FAKE + 4))
    for out in ("q_taken", "q_taken64", "td"):
        _refused(built, b"need own_actions", "coma", weights=bad_packed, rows=Q(state=FAKE + 4, **{out: FAKE}))
    _refused(built, b"td needs reward and done", "coma", weights=bad_packed, rows=Q(td=FAKE, own_actions=FAKE, done=FAKE, state=FAKE + 4))
    _refused(built, b"td needs reward and done", "coma", weights=bad_packed, rows=Q(td=FAKE, own_actions=FAKE, reward=FAKE, state=FAKE + 4))
    for name, ptr in (("state", FAKE + 8), ("v_obs", FAKE + 8), ("goals", FAKE + 4), ("actions", FAKE + 2), ("own_actions", FAKE + 2)):
        _refused(built, b"misaligned inputs", "coma", weights=bad_packed, rows=Q(q=FAKE + 2, **{name: ptr}))
    _refused(built, b"misaligned reward", "coma", weights=bad_packed,
             rows=Q(td=FAKE, own_actions=FAKE, done=FAKE, reward=FAKE + 2, q=FAKE + 2))
    _refused(built, b"misaligned reward", "coma", rows=Q(td=FAKE, own_actions=FAKE, done=FAKE, reward=FAKE + 4, reward_f64=1))
    for kw in ({"q": FAKE + 2}, {"q_taken": FAKE + 2, "own_actions": FAKE}, {"q_taken64": FAKE + 4, "own_actions": FAKE},
               {"td": FAKE + 4, "own_actions": FAKE, "done": FAKE, "reward": FAKE}):
        _refused(built, b"misaligned outputs", "coma", weights=bad_packed, rows=Q(**kw))
    _refused(built, b"misaligned packed", "coma", weights=bad_packed)


def test_pack_validates_before_launching(built):
    handle = built.lib()
    for fn, d, wcls, stage2 in ((handle.cm3_value_particle_pack, _vdesc(built), built.ValueParticleWeights, True),
                                (handle.cm3_coma_particle_pack, _qdesc(built), built.ComaParticleWeights, False)):
        W = lambda **kw: ctypes.byref(_weights(wcls, **kw))      # noqa: E731
        assert fn(None, W(), FAKE, None) == -1 and b"null desc" in handle.cm3_last_error()
        assert fn(ctypes.byref(d), None, FAKE, None) == -1 and b"null weights" in handle.cm3_last_error()
        assert fn(ctypes.byref(d), W(), None, None) == -1 and b"packed is NULL" in handle.cm3_last_error()
        assert fn(ctypes.byref(d), W(w_out=None), FAKE, None) == -1 and b"missing weights" in handle.cm3_last_error()
        if stage2:
            assert fn(ctypes.byref(d), W(w_b2=None), FAKE, None) == -1 and b"missing stage-2 weights" in handle.cm3_last_error()
        assert fn(ctypes.byref(d), W(), FAKE + 4, None) == -1 and b"misaligned packed" in handle.cm3_last_error()


def test_the_unit_is_built_like_the_matrix_units_and_holds_no_inline_assembly():
    """baseline.hip is compiled beside build.sh's loop over the matrix units, with that loop's flags, and linked through OBJS (so the
    post-build lint sees it); it and every csrc file it includes hold no inline assembly but the two empty scalar-operand statements
    of common.h -- the rule tests/test_abi.py enforces on the units of the loop."""
    root = os.path.join(ROOT, "cm3_amd", "csrc")
    build = open(os.path.join(root, "build.sh")).read()
    loop = re.search(r"for f in [a-z_ ]+; do\s*\n\s*(\"\$\{HIPCC\}\" \$\{FLAGS\} \$\{PHYS\} \$\{MFMA_FORM\}[^\n]*)\n", build)
    assert loop, "build.sh: the loop that compiles the matrix translation units was not found"
    own = [line for line in build.splitlines() if '"${HERE}/baseline.hip"' in line]
    assert len(own) == 1 and own[0].strip() == loop.group(1).strip().replace("${f}", "baseline")
    objs = build[build.index("OBJS=("):]
    assert '"${OBJ}/baseline.o"' in objs[:objs.index(")")]
    todo, scanned = ["baseline.hip"], []
    while todo:
        name = todo.pop()
        if name in scanned:
            continue
        scanned.append(name)
        text = open(os.path.join(root, name)).read()
        todo += re.findall(r'^\s*#\s*include\s+"([^"/]+)"', text, flags=re.M)
        code = re.sub(r"//[^\n]*", "", text)          # (comments may talk about asm)
        code = re.sub(r'asm\s+volatile\s*\(\s*""\s*:\s*"\+s"\s*\(\w+\)\s*\)', "", code)
        code = re.sub(r'asm\s+volatile\s*\(\s*""\s*:\s*:\s*"s"\s*\(\w+\)\s*\)', "", code)
        assert not re.search(r"\basm\s*(volatile\s*)?\(", code), "%s: inline assembly in a matrix translation unit" % name
    assert {"critic_rows.h", "actor_common.h", "common.h", "philox.h"} <= set(scanned), scanned
