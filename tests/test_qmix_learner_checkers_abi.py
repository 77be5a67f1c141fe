"""CPU: the C ABI of the Checkers QMIX learner (part of ABI 9, additive) -- cm3_qmix_learner_checkers_workspace_bytes / _grad_f32
declared, exported, bound; the structs' layout as a C compiler sees it; the workspace size; every invalid argument refused in the
stated order (descriptor, pointers, row counts) before anything touches a GPU; how the unit is built and what it shares with the
particle learner's; the refusals of CheckersQmixLearner and of qmix_train_step_feeds(env="checkers", learner=)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cm3_qmix_learner_checkers_workspace_bytes", "cm3_qmix_learner_checkers_grad_f32")
FAKE = 0x1000                                      # 16-byte aligned, never dereferenced: validation fails first
AGENT = ["conv_w", "conv_b", "lin_w", "lin_b", "self_w", "self_b", "w_self_h2", "others_w", "others_b", "w_others_h2", "b_h2", "out_w",
         "out_b"]
MIXER = ["conv_w", "conv_b", "hyper_w_1", "hyper_w_final", "hyper_b_1", "hyper_b_final_l1", "hyper_b_final"]
INPUTS = ["obs_self_t", "obs_self_v", "obs_others", "actions_prev", "actions", "goals", "grid", "vec", "td"]
MAX_STEPS = (2 ** 31 - 1) // 216


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    return _lib


def test_header_declares_and_library_exports_the_entries(built):
    raw = open(os.path.join(ROOT, "include", "cm3_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    handle = built.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(handle, name), name
        assert name in built.SYMBOLS, name
    assert built.ABI_VERSION == 9 and handle.cm3_abi_version() == 9
    for name in ("cm3_qmix_learner_checkers_desc", "cm3_qmix_learner_checkers_rows"):
        assert re.search(r"\}\s*%s\s*;" % name, text) and not re.search(r"typedef struct %s\b" % name, text), name
    # weights and gradients go in as the existing structs: no third weights struct
    grad = text[text.index("int cm3_qmix_learner_checkers_grad_f32"):]
    grad = grad[:grad.index(";")]
    assert grad.count("const cm3_actor_checkers_weights *") == 2 and grad.count("const cm3_qmix_mixer_checkers_weights *") == 2


def test_struct_layouts_match_the_header(built, tmp_path):
    structs = {"cm3_qmix_learner_checkers_desc": built.QmixLearnerCheckersDesc, "cm3_qmix_learner_checkers_rows": built.QmixLearnerCheckersRows}
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
    assert [f for f, _ in built.QmixLearnerCheckersDesc._fields_] == ["n_agents", "conv_f", "n_conv_linear", "n_h1", "n_h2", "n_actions",
                                                                      "embed_dim", "mixer_conv_f"]
    assert [f for f, _ in built.QmixLearnerCheckersRows._fields_] == (["obs_self_t_f64", "grid_f64", "goals_onehot", "td_f64"] + INPUTS
                                                                      + ["loss", "q_tot", "n_steps"])


def workspace_floats(N, B):
    """csrc/learner_checkers.hip's ws_layout: per agent row the window [80], its patches [25][27], c1 [160], xs [48], obs_others [16],
    hs / ho / h2 and their three deltas [256], Q and d Q [16], d lin [32], d c1 [25][16]; per transition the grid [64], its patches
    [27][30], xm (padded to whole k groups), the hyper pre-activations [128 (N + 3)], the delta rows [128 (N + 4)], d conv [27][16],
    err2; one partial gradient per 256 rows with one more row tile for the bias sums, nine jobs"""
    up4 = lambda x: (x + 3) // 4 * 4      # noqa: E731
    R, Lo, KM = B * N, 2 * max(N - 1, 1), 108 + 6 * N
    KP = (KM + 15) // 16 * 16
    chunks = lambda rows: (rows + 255) // 256      # noqa: E731
    part = lambda rows, Kx, ldd: up4(chunks(rows) * ((Kx + 15) // 16 + 1) * 16 * ldd)      # noqa: E731
    rows = sum(up4(R * k) for k in (80, 25 * 27, 160, 48, 16, 256, 256, 256, 16, 16, 256, 256, 256, 32, 25 * 16))
    steps = sum(up4(B * k) for k in (64, 27 * 30, KP, 128 * (N + 3), 128 * (N + 4), 27 * 16, 1))
    partial = (part(25 * R, 27, 16) + part(R, 150, 32) + part(R, 43, 256) + part(R, Lo, 256) + 2 * part(R, 256, 256) + part(R, 256, 16)
               + part(27 * B, 30, 16) + part(B, KM, 128 * (N + 4)))
    return rows + steps + partial


def test_workspace_bytes(built):
    fn = built.lib().cm3_qmix_learner_checkers_workspace_bytes
    for n in range(1, 9):
        for B in (1, 3, 37, 128, 256, 257, 4096):
            assert fn(n, B) == 4 * workspace_floats(n, B), (n, B)
            assert fn(n, B) % 16 == 0
    for n in (0, 9, 10, -1):
        assert fn(n, 128) == 0
    for B in (0, -1, MAX_STEPS + 1, 2 ** 40):
        assert fn(2, B) == 0
    assert fn(8, MAX_STEPS) > 0


def _desc(built, **kw):
    d = built.QmixLearnerCheckersDesc()
    d.n_agents, d.conv_f, d.n_conv_linear, d.n_h1, d.n_h2, d.n_actions, d.embed_dim, d.mixer_conv_f = 2, 6, 32, 256, 256, 5, 128, 4
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _tensors(cls, fields, **kw):
    t = cls()
    for f in fields:
        setattr(t, f, FAKE)
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _agent(built, **kw):
    return _tensors(built.ActorCheckersWeights, AGENT, **kw)


def _mixer(built, **kw):
    return _tensors(built.QmixMixerCheckersWeights, MIXER, **kw)


def _rows(built, **kw):
    r = built.QmixLearnerCheckersRows()
    r.obs_self_t_f64, r.grid_f64, r.goals_onehot, r.td_f64 = 1, 1, 1, 1
    for f in INPUTS + ["loss", "q_tot"]:
        setattr(r, f, FAKE)
    r.n_steps = 128
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _refused(built, needle, desc="default", aw="default", mw="default", ag="default", mg="default", rows="default", workspace=FAKE,
             nbytes=1 << 40):
    handle = built.lib()
    d = _desc(built) if desc == "default" else desc
    aw = _agent(built) if aw == "default" else aw
    ag = _agent(built) if ag == "default" else ag
    mw = _mixer(built) if mw == "default" else mw
    mg = _mixer(built) if mg == "default" else mg
    r = _rows(built) if rows == "default" else rows
    ref = lambda x: None if x is None else ctypes.byref(x)      # noqa: E731
    rc = handle.cm3_qmix_learner_checkers_grad_f32(ref(d), ref(aw), ref(mw), ref(ag), ref(mg), ref(r), workspace, nbytes, None)
    assert rc == -1                                              # CM3_ERR_INVALID
    assert needle in handle.cm3_last_error(), handle.cm3_last_error()


def test_null_arguments_are_refused(built):
    _refused(built, b"null desc", desc=None)
    _refused(built, b"null weights", aw=None)
    _refused(built, b"null weights", mw=None)
    _refused(built, b"null grads", ag=None)
    _refused(built, b"null grads", mg=None)
    _refused(built, b"null rows", rows=None)
    _refused(built, b"workspace is NULL", workspace=None)


@pytest.mark.parametrize("kw,needle", [
    ({"n_agents": 0}, b"n_agents must be in 1..8"), ({"n_agents": 9}, b"n_agents must be in 1..8"), ({"n_agents": -3}, b"n_agents must be in 1..8"),
    ({"conv_f": 4}, b"6/32/256/256/5"), ({"n_conv_linear": 64}, b"6/32/256/256/5"), ({"n_h1": 64}, b"6/32/256/256/5"),
    ({"n_h2": 128}, b"6/32/256/256/5"), ({"n_actions": 4}, b"6/32/256/256/5"), ({"embed_dim": 64}, b"embedding width"),
    ({"mixer_conv_f": 6}, b"embedding width")])
def test_invalid_descriptor_is_refused_first(built, kw, needle):
    _refused(built, needle, desc=_desc(built, **kw))
    # ... before the pointers and before the row count
    _refused(built, needle, desc=_desc(built, **kw), aw=None, rows=_rows(built, n_steps=0))


def test_missing_and_misaligned_pointers_are_refused_before_the_row_count(built):
    bad = _rows(built, n_steps=0)
    for name in AGENT:
        _refused(built, b"missing weights", aw=_agent(built, **{name: None}), rows=bad)
        _refused(built, b"missing gradients", ag=_agent(built, **{name: None}), rows=bad)
    for name in MIXER:
        _refused(built, b"missing weights", mw=_mixer(built, **{name: None}), rows=bad)
        _refused(built, b"missing gradients", mg=_mixer(built, **{name: None}), rows=bad)
    for name in INPUTS:
        _refused(built, b"missing inputs", rows=_rows(built, n_steps=0, **{name: None}))
    for name in ("loss", "q_tot"):
        _refused(built, b"missing outputs", rows=_rows(built, n_steps=0, **{name: None}))
    _refused(built, b"misaligned weights or gradients", aw=_agent(built, lin_w=FAKE + 2), rows=bad)
    _refused(built, b"misaligned weights or gradients", mg=_mixer(built, hyper_w_1=FAKE + 1), rows=bad)
    for kw in ({"obs_self_t": FAKE + 4}, {"obs_self_v": FAKE + 4}, {"obs_others": FAKE + 4}, {"vec": FAKE + 4}, {"grid": FAKE + 4},
               {"goals": FAKE + 4}, {"actions_prev": FAKE + 2}, {"actions": FAKE + 2}, {"td": FAKE + 4}):
        _refused(built, b"misaligned inputs", rows=_rows(built, n_steps=0, **kw))
    _refused(built, b"misaligned outputs", rows=_rows(built, n_steps=0, loss=FAKE + 2))
    _refused(built, b"misaligned workspace", rows=bad, workspace=FAKE + 8)
    # the narrow forms need no alignment, a float32 td 4 bytes: the call goes on to the row count
    _refused(built, b"n_steps must be positive",
             rows=_rows(built, n_steps=0, obs_self_t=FAKE + 1, obs_self_t_f64=0, grid=FAKE + 3, grid_f64=0, goals=FAKE + 1, goals_onehot=0,
                        td=FAKE + 4, td_f64=0))


@pytest.mark.parametrize("n_steps", [0, -5, MAX_STEPS + 1, 2 ** 40])
def test_row_count_out_of_range_is_refused(built, n_steps):
    _refused(built, b"n_steps", rows=_rows(built, n_steps=n_steps))


def test_a_small_workspace_is_refused(built):
    need = built.lib().cm3_qmix_learner_checkers_workspace_bytes(2, 128)
    _refused(built, b"too small", nbytes=need - 4)
    _refused(built, b"too small", nbytes=0)


def test_the_unit_is_built_like_the_matrix_units_and_shares_the_particle_learners_kernels():
    """learner_checkers.hip is compiled beside build.sh's loop over the matrix units, with that loop's flags, linked through OBJS (so the
    post-build lint sees it) and named on the diagnostics line; it and every csrc file it includes hold no inline assembly but the two
    empty scalar-operand statements of common.h.  The X^T . Delta and reduce kernels live in learner_common.h, which both learners
    include; neither unit defines them or includes another unit."""
    root = os.path.join(ROOT, "cm3_amd", "csrc")
    build = open(os.path.join(root, "build.sh")).read()
    loop = re.search(r"for f in [a-z_ ]+; do\s*\n\s*(\"\$\{HIPCC\}\" \$\{FLAGS\} \$\{PHYS\} \$\{MFMA_FORM\}[^\n]*)\n", build)
    assert loop, "build.sh: the loop that compiles the matrix translation units was not found"
    own = [line for line in build.splitlines() if '"${HERE}/learner_checkers.hip"' in line]
    assert len(own) == 1 and own[0].strip() == loop.group(1).strip().replace("${f}", "learner_checkers")
    objs = build[build.index("OBJS=("):]
    assert '"${OBJ}/learner_checkers.o"' in objs[:objs.index(")")]
    diag = [line for line in build.splitlines() if "resource_usage.txt" in line and line.startswith("for f in")]
    assert len(diag) == 1 and " learner_checkers " in diag[0]
    todo, scanned = ["learner_checkers.hip"], []
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
    assert {"actor_common.h", "common.h", "ck_tiles.h", "learner_common.h"} <= set(scanned), scanned
    assert not [n for n in scanned[1:] if n.endswith(".hip")], scanned
    text = open(os.path.join(root, "learner_checkers.hip")).read()
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in text and "atomicAdd" not in text and "unsafeAtomicAdd" not in text
    common = open(os.path.join(root, "learner_common.h")).read()
    particle = open(os.path.join(root, "learner.hip")).read()
    for unit in (text, particle):
        assert '#include "learner_common.h"' in unit
        assert not re.search(r"__global__[^\n]*k_learner_(xtd|reduce)", unit)
    assert len(re.findall(r"__global__[^\n]*k_learner_xtd", common)) == 1 and len(re.findall(r"__global__[^\n]*k_learner_reduce", common)) == 1
    assert "k_learner_xtd<9>" in text and "k_learner_xtd<4>" in particle


# ---- the Python layer's refusals (no GPU: bare objects, the refusal comes before any launch) ----
def _bare(cls_name, n, device="cuda:0"):
    import torch
    from cm3_amd import qmix
    cls = getattr(qmix, cls_name)
    obj = cls.__new__(cls)
    obj.n, obj.device = n, torch.device(device)
    return obj


def test_the_learner_refuses_networks_it_cannot_train():
    from cm3_amd import Cm3Error
    from cm3_amd.qmix import CheckersQmixLearner
    with pytest.raises(Cm3Error, match="takes the main CheckersQmixAgent and the main CheckersQmixMixer, got object"):
        CheckersQmixLearner(object(), _bare("CheckersQmixMixer", 2))
    with pytest.raises(Cm3Error, match="got CheckersQmixAgent and ParticleQmixMixer"):
        CheckersQmixLearner(_bare("CheckersQmixAgent", 2), _bare("ParticleQmixMixer", 2))
    with pytest.raises(Cm3Error, match="got ParticleQmixAgent and CheckersQmixMixer"):
        CheckersQmixLearner(_bare("ParticleQmixAgent", 2), _bare("CheckersQmixMixer", 2))
    with pytest.raises(Cm3Error, match="the agent is built for 2 agents, the mixer for 3; build both for one agent count"):
        CheckersQmixLearner(_bare("CheckersQmixAgent", 2), _bare("CheckersQmixMixer", 3))
    with pytest.raises(Cm3Error, match="build both on one device"):
        CheckersQmixLearner(_bare("CheckersQmixAgent", 2), _bare("CheckersQmixMixer", 2, "cuda:1"))


def test_the_learner_is_exported_shares_its_base_and_has_no_launch_hook():
    import cm3_amd
    from cm3_amd import qmix
    from cm3_amd._net import _DeviceNet
    from tests.test_device_net_hooks import HOOKS
    assert cm3_amd.CheckersQmixLearner is qmix.CheckersQmixLearner
    assert not issubclass(qmix.CheckersQmixLearner, _DeviceNet)
    assert not [h for h in HOOKS if hasattr(qmix.CheckersQmixLearner, h)]
    # the gradient store, the segment table, Adam and _reserve are one text for both learners
    for name in ("__init__", "_reserve", "enqueue_adam", "gradients", "step", "workspace_floats"):
        assert getattr(qmix.CheckersQmixLearner, name) is getattr(qmix.ParticleQmixLearner, name), name
    for name in ("enqueue_gradients", "train_step", "_stage"):
        assert getattr(qmix.CheckersQmixLearner, name) is not getattr(qmix.ParticleQmixLearner, name), name


def _never(ops, feed):
    raise AssertionError("run was called: the refusal must come first")


def test_train_step_feeds_refuses_a_learner_it_cannot_use():
    import torch
    from cm3_amd.batch import qmix_train_step_feeds

    class L(object):
        agent = _bare("CheckersQmixAgent", 4)
    # anything but a CheckersQmixLearner, before a column is read
    for bad in (L(), _bare("ParticleQmixLearner", 2), object()):
        with pytest.raises(ValueError, match="takes a CheckersQmixLearner as learner, got %s: the Checkers learner is not built from another "
                                             "network's weights" % type(bad).__name__):
            qmix_train_step_feeds({}, _never, 0.99, env="checkers", learner=bad)
    learner = _bare("CheckersQmixLearner", 4)
    learner.agent = _bare("CheckersQmixAgent", 4)
    with pytest.raises(ValueError, match="pass target_agent and target_mixer"):
        qmix_train_step_feeds({}, _never, 0.99, env="checkers", learner=learner)
    with pytest.raises(ValueError, match="pass target_agent and target_mixer"):
        qmix_train_step_feeds({}, _never, 0.99, env="checkers", target_agent=_bare("CheckersQmixAgent", 2), learner=learner)
    cols = {"vec": torch.zeros(3, 2, 4, dtype=torch.float64)}
    with pytest.raises(ValueError, match="learner is built for 4 agents, the batch has 2"):
        qmix_train_step_feeds(cols, _never, 0.99, env="checkers", target_agent=_bare("CheckersQmixAgent", 2),
                              target_mixer=_bare("CheckersQmixMixer", 2), learner=learner)
