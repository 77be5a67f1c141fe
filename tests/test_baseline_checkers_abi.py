"""CPU: the C ABI of the Checkers IAC / COMA baseline critics over transition rows (part of ABI 9, additive) --
cm3_value_checkers_packed_bytes / _pack / _rows_f32 and cm3_coma_checkers_packed_bytes / _pack / _rows_f32 declared, exported, bound;
the six structs' layout as a C compiler sees it; every invalid argument refused with a readable error, in the stated order, before
anything touches a GPU (fake pointers: no launch happens); the unit's build line and its freedom from inline assembly."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cm3_value_checkers_packed_bytes", "cm3_value_checkers_pack", "cm3_value_checkers_rows_f32",
           "cm3_coma_checkers_packed_bytes", "cm3_coma_checkers_pack", "cm3_coma_checkers_rows_f32")
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


def test_struct_layouts_match_the_header(built, tmp_path):
    structs = {"cm3_value_checkers_desc": built.ValueCheckersDesc, "cm3_value_checkers_weights": built.ValueCheckersWeights,
               "cm3_value_checkers_rows": built.ValueCheckersRows, "cm3_coma_checkers_desc": built.ComaCheckersDesc,
               "cm3_coma_checkers_weights": built.ComaCheckersWeights, "cm3_coma_checkers_rows": built.ComaCheckersRows}
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


def test_packed_bytes(built):
    fv, fq = built.lib().cm3_value_checkers_packed_bytes, built.lib().cm3_coma_checkers_packed_bytes
    for n in range(1, 9):
        for kind in (LOCAL, GLOBAL):
            assert fv(n, kind) > 0 and fv(n, kind) % 16 == 0
        assert (fq(n) > 0) == (n > 1) and fq(n) % 16 == 0
    # Toeplitz [80 x 160] + 160, branch1 [176 x 256] + 256, h2 [256 x 256], out [256 x 16] + 16 at one agent (local) ...
    assert fv(1, LOCAL) == 4 * (80 * 160 + 160 + 176 * 256 + 256 + 256 * 256 + 256 * 16 + 16)
    # ... [64 x 112] + 112 and [128 x 256] (global); stage 2 adds branch2 [K2P x 32] + 32 and 32 rows of h2: K2 = 28 -> 32
    assert fv(1, GLOBAL) == 4 * (64 * 112 + 112 + 128 * 256 + 256 + 256 * 256 + 256 * 16 + 16)
    assert fv(8, GLOBAL) == 4 * (64 * 112 + 112 + 128 * 256 + 256 + 32 * 32 + 32 + 288 * 256 + 256 * 16 + 16)
    assert fv(8, LOCAL) == 4 * (80 * 160 + 160 + 176 * 256 + 256 + 16 * 32 + 32 + 288 * 256 + 256 * 16 + 16)
    # both Toeplitz matrices, h1 [(272 + pad16(12 N - 1)) x 256] + 256, h2 [256 x 256] + 256, out [256 x 16] + 16
    for n, tp in ((2, 32), (5, 64), (8, 96)):
        assert fq(n) == 4 * (64 * 112 + 112 + 80 * 160 + 160 + (272 + tp) * 256 + 256 + 256 * 256 + 256 + 256 * 16 + 16)
    for n, kind in ((0, LOCAL), (9, GLOBAL), (4, 2), (4, -1)):
        assert fv(n, kind) == 0
    for n in (-1, 0, 1, 9):
        assert fq(n) == 0


def _fill(struct, **kw):
    for k, v in kw.items():
        setattr(struct, k, v)
    return struct


def _vdesc(built, **kw):
    d = built.ValueCheckersDesc()
    d.n_agents, d.stage, d.kind, d.n_h1_1, d.n_h1_2, d.n_h2 = 4, 2, LOCAL, 256, 32, 256
    return _fill(d, **kw)


def _qdesc(built, **kw):
    d = built.ComaCheckersDesc()
    d.n_agents, d.units = 4, 256
    return _fill(d, **kw)


def _weights(cls, **kw):
    w = cls()
    for f, _ in cls._fields_:
        setattr(w, f, FAKE)
    return _fill(w, **kw)


def _vrows(built, **kw):
    r = built.ValueCheckersRows()
    r.grid_f64 = r.windows_f64 = r.goals_onehot = 1
    r.grid, r.vec, r.goals, r.windows, r.obs_self_v, r.obs_others, r.v, r.n_steps, r.gamma = FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 100, 0.99
    return _fill(r, **kw)


def _qrows(built, **kw):
    r = built.ComaCheckersRows()
    r.grid_f64 = r.windows_f64 = r.goals_onehot = 1
    r.grid, r.vec, r.goals, r.actions, r.windows, r.obs_self_v, r.q, r.n_steps, r.gamma = FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 100, 0.99
    return _fill(r, **kw)


def _refused(built, needle, which, desc="default", weights="default", rows="default"):
    handle = built.lib()
    if which == "value":
        fn, d0, w0, r0 = handle.cm3_value_checkers_rows_f32, _vdesc(built), _weights(built.ValueCheckersWeights), _vrows(built)
    else:
        fn, d0, w0, r0 = handle.cm3_coma_checkers_rows_f32, _qdesc(built), _weights(built.ComaCheckersWeights), _qrows(built)
    d, w, r = (d0 if desc == "default" else desc), (w0 if weights == "default" else weights), (r0 if rows == "default" else rows)
    ref = lambda x: None if x is None else ctypes.byref(x)      # noqa: E731
    assert fn(ref(d), ref(w), ref(r), None) == -1
    assert needle in handle.cm3_last_error(), handle.cm3_last_error()


def test_null_arguments_are_refused(built):
    for which, wcls in (("value", built.ValueCheckersWeights), ("coma", built.ComaCheckersWeights)):
        _refused(built, b"null desc", which, desc=None)
        _refused(built, b"null weights", which, weights=None)
        _refused(built, b"null rows", which, rows=None)
        _refused(built, b"packed weights are NULL", which, weights=_weights(wcls, packed=None))


@pytest.mark.parametrize("kw,needle", [
    ({"n_agents": 0}, b"n_agents must be in 1..8"), ({"n_agents": 9}, b"n_agents must be in 1..8"),
    ({"kind": 2}, b"kind must be"), ({"kind": -1}, b"kind must be"), ({"stage": 0}, b"stage must be 1 or 2"),
    ({"stage": 3}, b"stage must be 1 or 2"),
    ({"stage": 1}, b"V_checkers_local runs at stage 1 with one agent"),
    ({"kind": GLOBAL, "n_agents": 1}, b"V_checkers_global runs at stage 1 with one agent"),
    ({"n_h1_1": 128}, b"256/32/256"), ({"n_h1_2": 64}, b"256/32/256"), ({"n_h2": 32}, b"256/32/256")])
def test_invalid_value_descriptor_is_refused_without_a_gpu(built, kw, needle):
    _refused(built, needle, "value", desc=_vdesc(built, **kw))
    handle = built.lib()
    assert handle.cm3_value_checkers_pack(ctypes.byref(_vdesc(built, **kw)), ctypes.byref(_weights(built.ValueCheckersWeights)), FAKE,
                                          None) == -1
    assert needle in handle.cm3_last_error()


@pytest.mark.parametrize("kw,needle", [
    ({"n_agents": 1}, b"n_agents must be in 2..8"), ({"n_agents": 0}, b"n_agents must be in 2..8"),
    ({"n_agents": 9}, b"n_agents must be in 2..8"), ({"units": 128}, b"width is 256")])
def test_invalid_coma_descriptor_is_refused_without_a_gpu(built, kw, needle):
    _refused(built, needle, "coma", desc=_qdesc(built, **kw))
    handle = built.lib()
    assert handle.cm3_coma_checkers_pack(ctypes.byref(_qdesc(built, **kw)), ctypes.byref(_weights(built.ComaCheckersWeights)), FAKE,
                                         None) == -1
    assert needle in handle.cm3_last_error()


def test_the_descriptor_is_checked_before_the_other_arguments(built):
    _refused(built, b"n_agents must be in 1..8", "value", desc=_vdesc(built, n_agents=0), weights=None, rows=None)
    _refused(built, b"n_agents must be in 2..8", "coma", desc=_qdesc(built, n_agents=1), weights=None, rows=None)


@pytest.mark.parametrize("which,n_steps", [("value", 0), ("value", -5), ("value", (2 ** 31 - 1) // 4 + 1), ("value", 2 ** 40),
                                           ("coma", 0), ("coma", (2 ** 31 - 1) // 4 + 1)])
def test_row_count_out_of_range_is_refused(built, which, n_steps):
    rows = _vrows(built, n_steps=n_steps) if which == "value" else _qrows(built, n_steps=n_steps)
    _refused(built, b"n_steps", which, rows=rows)


def test_value_refusals_fire_in_the_stated_order(built):
    """n_steps, inputs, outputs, td's inputs, alignment of inputs / reward / outputs / packed (the order of critic_rows::check_rows):
    each call breaks one rule and every LATER one, and the earlier rule is the one reported"""
    bad_packed = _weights(built.ValueCheckersWeights, packed=FAKE + 8)
    V = lambda **kw: _vrows(built, **kw)      # noqa: E731
    G = _vdesc(built, kind=GLOBAL)
    _refused(built, b"n_steps must be positive", "value", weights=bad_packed, rows=V(n_steps=0, goals=None, v=None))
    for name in ("goals", "windows", "obs_self_v"):
        _refused(built, b"missing inputs: goals", "value", weights=bad_packed, rows=V(v=None, **{name: None}))
    for name in ("goals", "grid", "vec"):
        _refused(built, b"missing inputs: goals", "value", desc=G, weights=bad_packed, rows=V(v=None, **{name: None}))
    _refused(built, b"reads obs_others at stage 2", "value", weights=bad_packed, rows=V(obs_others=None, v=None))
    _refused(built, b"no output requested", "value", weights=bad_packed, rows=V(v=None, obs_self_v=FAKE + 4))
    _refused(built, b"td needs reward and done", "value", weights=bad_packed, rows=V(td=FAKE, done=FAKE, obs_self_v=FAKE + 4))
    _refused(built, b"td needs reward and done", "value", weights=bad_packed, rows=V(td=FAKE, reward=FAKE, obs_self_v=FAKE + 4))
    for name in ("obs_self_v", "windows", "obs_others", "goals"):
        _refused(built, b"misaligned inputs", "value", weights=bad_packed, rows=V(td=FAKE, done=FAKE, reward=FAKE + 2, **{name: FAKE + 4}))
    for name in ("vec", "grid", "goals"):
        _refused(built, b"misaligned inputs", "value", desc=G, weights=bad_packed, rows=V(v=FAKE + 2, **{name: FAKE + 4}))
    _refused(built, b"misaligned reward", "value", weights=bad_packed, rows=V(td=FAKE, done=FAKE, reward=FAKE + 2, v=FAKE + 2))
    _refused(built, b"misaligned reward", "value", rows=V(td=FAKE, done=FAKE, reward=FAKE + 4, reward_f64=1))
    for kw in ({"v": FAKE + 2}, {"v64": FAKE + 4}, {"td": FAKE + 4, "done": FAKE, "reward": FAKE}):
        _refused(built, b"misaligned outputs", "value", weights=bad_packed, rows=V(**kw))
    _refused(built, b"misaligned packed", "value", weights=bad_packed)
    # a network reads only its own kind's columns, int8 windows / grids and index goals need no alignment: without / off the 8-byte
    # grid they pass those checks and fail a later one
    _refused(built, b"misaligned packed", "value", desc=G, weights=bad_packed, rows=V(obs_others=None, windows=None, obs_self_v=FAKE + 2))
    _refused(built, b"misaligned packed", "value", weights=bad_packed, rows=V(grid=None, vec=FAKE + 2))
    _refused(built, b"misaligned packed", "value", desc=_vdesc(built, n_agents=1, stage=1), weights=bad_packed, rows=V(obs_others=FAKE + 2))
    _refused(built, b"misaligned packed", "value", weights=bad_packed, rows=V(windows=FAKE + 1, windows_f64=0, goals=FAKE + 1, goals_onehot=0))


def test_coma_refusals_fire_in_the_stated_order(built):
    bad_packed = _weights(built.ComaCheckersWeights, packed=FAKE + 8)
    Q = lambda **kw: _qrows(built, **kw)      # noqa: E731
    _refused(built, b"n_steps must be positive", "coma", weights=bad_packed, rows=Q(n_steps=0, vec=None, q=None))
    for name in ("grid", "vec", "goals", "windows", "obs_self_v"):
        _refused(built, b"missing inputs: grid, vec, goals, windows and obs_self_v", "coma", weights=bad_packed,
                 rows=Q(actions=None, **{name: None}))
    _refused(built, b"reads the actions of the others", "coma", weights=bad_packed, rows=Q(actions=None, q=None))
    _refused(built, b"no output requested", "coma", weights=bad_packed, rows=Q(q=None, vec=FAKE + 4))
    for out in ("q_taken", "q_taken64", "td"):
        _refused(built, b"need own_actions", "coma", weights=bad_packed, rows=Q(vec=FAKE + 4, **{out: FAKE}))
    _refused(built, b"td needs reward and done", "coma", weights=bad_packed, rows=Q(td=FAKE, own_actions=FAKE, done=FAKE, vec=FAKE + 4))
    _refused(built, b"td needs reward and done", "coma", weights=bad_packed, rows=Q(td=FAKE, own_actions=FAKE, reward=FAKE, vec=FAKE + 4))
    for name, ptr in (("vec", FAKE + 4), ("obs_self_v", FAKE + 4), ("grid", FAKE + 4), ("windows", FAKE + 4), ("goals", FAKE + 4),
                      ("actions", FAKE + 2), ("own_actions", FAKE + 2)):
        _refused(built, b"misaligned inputs", "coma", weights=bad_packed, rows=Q(q=FAKE + 2, **{name: ptr}))
    _refused(built, b"misaligned reward", "coma", weights=bad_packed,
             rows=Q(td=FAKE, own_actions=FAKE, done=FAKE, reward=FAKE + 2, q=FAKE + 2))
    _refused(built, b"misaligned reward", "coma", rows=Q(td=FAKE, own_actions=FAKE, done=FAKE, reward=FAKE + 4, reward_f64=1))
    for kw in ({"q": FAKE + 2}, {"q_taken": FAKE + 2, "own_actions": FAKE}, {"q_taken64": FAKE + 4, "own_actions": FAKE},
               {"td": FAKE + 4, "own_actions": FAKE, "done": FAKE, "reward": FAKE}):
        _refused(built, b"misaligned outputs", "coma", weights=bad_packed, rows=Q(**kw))
    _refused(built, b"misaligned packed", "coma", weights=bad_packed)
    _refused(built, b"misaligned packed", "coma", weights=bad_packed,
             rows=Q(grid=FAKE + 1, grid_f64=0, windows=FAKE + 1, windows_f64=0, goals=FAKE + 1, goals_onehot=0))


def test_pack_validates_before_launching(built):
    handle = built.lib()
    for fn, d, wcls, stage2 in ((handle.cm3_value_checkers_pack, _vdesc(built), built.ValueCheckersWeights, True),
                                (handle.cm3_coma_checkers_pack, _qdesc(built), built.ComaCheckersWeights, False)):
        W = lambda **kw: ctypes.byref(_weights(wcls, **kw))      # noqa: E731
        assert fn(None, W(), FAKE, None) == -1 and b"null desc" in handle.cm3_last_error()
        assert fn(ctypes.byref(d), None, FAKE, None) == -1 and b"null weights" in handle.cm3_last_error()
        assert fn(ctypes.byref(d), W(), None, None) == -1 and b"packed is NULL" in handle.cm3_last_error()
        assert fn(ctypes.byref(d), W(w_out=None), FAKE, None) == -1 and b"missing weights" in handle.cm3_last_error()
        assert fn(ctypes.byref(d), W(b_out=None), FAKE, None) == -1 and b"missing weights" in handle.cm3_last_error()
        if stage2:
            assert fn(ctypes.byref(d), W(w_b2=None), FAKE, None) == -1 and b"missing stage-2 weights" in handle.cm3_last_error()
        assert fn(ctypes.byref(d), W(), FAKE + 4, None) == -1 and b"misaligned packed" in handle.cm3_last_error()


def test_the_unit_is_built_like_the_matrix_units_and_holds_no_inline_assembly():
    """baseline_checkers.hip is compiled beside build.sh's loop over the matrix units, with exactly that loop's command line, linked
    through OBJS (so the post-build lint sees it) and named in the diagnostics loop; it and every csrc file it includes hold no inline
    assembly but the two empty scalar-operand statements of common.h -- the scan tests/test_baseline_abi.py applies to baseline.hip."""
    root = os.path.join(ROOT, "cm3_amd", "csrc")
    build = open(os.path.join(root, "build.sh")).read()
    loop = re.search(r"for f in [a-z_ ]+; do\s*\n\s*(\"\$\{HIPCC\}\" \$\{FLAGS\} \$\{PHYS\} \$\{MFMA_FORM\}[^\n]*)\n", build)
    assert loop, "build.sh: the loop that compiles the matrix translation units was not found"
    own = [line for line in build.splitlines() if '"${HERE}/baseline_checkers.hip"' in line]
    assert len(own) == 1 and own[0].strip() == loop.group(1).strip().replace("${f}", "baseline_checkers")
    objs = build[build.index("OBJS=("):]
    assert '"${OBJ}/baseline_checkers.o"' in objs[:objs.index(")")]
    diag = re.search(r"for f in ([a-z_0-9 ]+); do grep -v \"remark:\"", build)
    assert diag and "baseline_checkers" in diag.group(1).split()
    todo, scanned = ["baseline_checkers.hip"], []
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
    assert {"ck_tiles.h", "critic_rows.h", "actor_common.h", "common.h", "philox.h"} <= set(scanned), scanned
