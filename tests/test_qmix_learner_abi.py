"""CPU: the C ABI of the particle QMIX learner (part of ABI 9, additive) -- cm3_qmix_learner_particle_workspace_bytes / _grad_f32 and
cm3_adam_step_f32 declared, exported, bound; the structs' layout as a C compiler sees it; the workspace size; every invalid argument
refused in the stated order (descriptor, pointers, row counts) before anything touches a GPU; how the unit is built; the refusals of
ParticleQmixLearner and of qmix_train_step_feeds(learner=)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cm3_qmix_learner_particle_workspace_bytes", "cm3_qmix_learner_particle_grad_f32", "cm3_adam_step_f32")
FAKE = 0x1000                                      # 16-byte aligned, never dereferenced: validation fails first
TENSORS = ["h_kernel", "h_bias", "h2_kernel", "h2_bias", "out_kernel", "out_bias", "hyper_w_1", "hyper_w_final", "hyper_b_1",
           "hyper_b_final_l1", "hyper_b_final"]


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
    assert re.search(r"#define\s+CM3_ABI_VERSION\s+9\b", text)
    for name in ("cm3_qmix_learner_particle_desc", "cm3_qmix_learner_tensors", "cm3_qmix_learner_rows", "cm3_adam_segment", "cm3_adam_desc"):
        assert re.search(r"\}\s*%s\s*;" % name, text) and not re.search(r"typedef struct %s\b" % name, text), name


def test_struct_layouts_match_the_header(built, tmp_path):
    structs = {"cm3_qmix_learner_particle_desc": built.QmixLearnerParticleDesc, "cm3_qmix_learner_tensors": built.QmixLearnerTensors,
               "cm3_qmix_learner_rows": built.QmixLearnerRows, "cm3_adam_segment": built.AdamSegment, "cm3_adam_desc": built.AdamDesc}
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
    assert [f for f, _ in built.QmixLearnerParticleDesc._fields_] == ["n_agents", "n_h", "n_actions", "embed_dim"]
    assert [f for f, _ in built.QmixLearnerTensors._fields_] == TENSORS
    assert [f for f, _ in built.QmixLearnerRows._fields_] == ["td_f64", "reserved", "obs_others", "v_obs", "goals", "actions", "state", "td",
                                                               "loss", "q_tot", "n_steps"]
    assert [f for f, _ in built.AdamSegment._fields_] == ["var", "grad", "m", "v", "count"] and ctypes.sizeof(built.AdamSegment) == 40
    assert [f for f, _ in built.AdamDesc._fields_] == ["lr", "beta1", "beta2", "epsilon", "n_segments", "reserved", "total"]


def workspace_floats(N, B):
    """csrc/learner.hip's ws_layout: the rows' inputs (padded to L + 8), h1, h2, q_sel, d q_sel, d Q [16], d h2, d h1; the mixer's
    inputs (padded to whole k-steps), its delta rows [64 (N + 4)], err2; one partial gradient per 256 rows with one more row tile for
    the bias sums"""
    up4 = lambda x: (x + 3) // 4 * 4      # noqa: E731
    L = 4 * max(N - 1, 1)
    K1, K1P, KM = L + 6, L + 8, 6 * N
    KMP, MD = up4(KM), 64 * (N + 4)
    R = B * N
    ca, cm = (R + 255) // 256, (B + 255) // 256
    rows = up4(R * K1P) + 2 * R * 64 + 2 * up4(R) + R * 16 + 2 * R * 64
    mixer = B * KMP + B * MD + up4(B)
    partial = ca * (((K1 + 15) // 16 + 1) * 16 * 64 + 5 * 16 * 64 + 5 * 16 * 16) + cm * ((KM + 15) // 16 + 1) * 16 * MD
    return rows + mixer + partial


def test_workspace_bytes(built):
    fn = built.lib().cm3_qmix_learner_particle_workspace_bytes
    for n in range(1, 11):
        for B in (1, 3, 37, 128, 256, 257, 16384):
            assert fn(n, B) == 4 * workspace_floats(n, B), (n, B)
            assert fn(n, B) % 16 == 0
    assert fn(4, 128) == 4 * workspace_floats(4, 128) == 1051136
    for n in (0, 11, -1):
        assert fn(n, 128) == 0
    for B in (0, -1, (2 ** 31 - 1) // 10 + 1, 2 ** 40):
        assert fn(4, B) == 0
    assert fn(10, (2 ** 31 - 1) // 10) > 0


def _desc(built, **kw):
    d = built.QmixLearnerParticleDesc()
    d.n_agents, d.n_h, d.n_actions, d.embed_dim = 4, 64, 5, 64
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _tensors(built, **kw):
    t = built.QmixLearnerTensors()
    for f in TENSORS:
        setattr(t, f, FAKE)
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _rows(built, **kw):
    r = built.QmixLearnerRows()
    r.td_f64 = 1
    for f in ("obs_others", "v_obs", "goals", "actions", "state", "td", "loss", "q_tot"):
        setattr(r, f, FAKE)
    r.n_steps = 128
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _refused(built, needle, desc="default", weights="default", grads="default", rows="default", workspace=FAKE, nbytes=1 << 40):
    handle = built.lib()
    d = _desc(built) if desc == "default" else desc
    w = _tensors(built) if weights == "default" else weights
    g = _tensors(built) if grads == "default" else grads
    r = _rows(built) if rows == "default" else rows
    ref = lambda x: None if x is None else ctypes.byref(x)      # noqa: E731
    rc = handle.cm3_qmix_learner_particle_grad_f32(ref(d), ref(w), ref(g), ref(r), workspace, nbytes, None)
    assert rc == -1                                              # CM3_ERR_INVALID
    assert needle in handle.cm3_last_error(), handle.cm3_last_error()


def test_null_arguments_are_refused(built):
    _refused(built, b"null desc", desc=None)
    _refused(built, b"null weights", weights=None)
    _refused(built, b"null grads", grads=None)
    _refused(built, b"null rows", rows=None)
    _refused(built, b"workspace is NULL", workspace=None)


@pytest.mark.parametrize("kw,needle", [
    ({"n_agents": 0}, b"n_agents must be in 1..10"), ({"n_agents": 11}, b"n_agents must be in 1..10"), ({"n_agents": -3}, b"n_agents must be in 1..10"),
    ({"n_h": 128}, b"64/64/5"), ({"n_actions": 4}, b"64/64/5"), ({"embed_dim": 128}, b"embedding width"), ({"embed_dim": 0}, b"embedding width")])
def test_invalid_descriptor_is_refused_first(built, kw, needle):
    _refused(built, needle, desc=_desc(built, **kw))
    # ... before the pointers and before the row count
    _refused(built, needle, desc=_desc(built, **kw), weights=None, rows=_rows(built, n_steps=0))


def test_missing_pointers_are_refused_before_the_row_count(built):
    bad = _rows(built, n_steps=0)
    for name in TENSORS:
        _refused(built, b"missing weights", weights=_tensors(built, **{name: None}), rows=bad)
        _refused(built, b"missing gradients", grads=_tensors(built, **{name: None}), rows=bad)
    for name in ("obs_others", "v_obs", "goals", "actions", "state", "td"):
        _refused(built, b"missing inputs", rows=_rows(built, n_steps=0, **{name: None}))
    for name in ("loss", "q_tot"):
        _refused(built, b"missing outputs", rows=_rows(built, n_steps=0, **{name: None}))
    for kw in ({"obs_others": FAKE + 8}, {"v_obs": FAKE + 4}, {"state": FAKE + 8}, {"goals": FAKE + 4}, {"actions": FAKE + 2}, {"td": FAKE + 4}):
        _refused(built, b"misaligned inputs", rows=_rows(built, n_steps=0, **kw))
    _refused(built, b"misaligned outputs", rows=_rows(built, n_steps=0, loss=FAKE + 2))
    _refused(built, b"misaligned workspace", rows=bad, workspace=FAKE + 8)
    # a float32 td needs 4-byte alignment only: the call goes on to the row count
    _refused(built, b"n_steps must be positive", rows=_rows(built, n_steps=0, td=FAKE + 4, td_f64=0))


@pytest.mark.parametrize("n_steps", [0, -5, (2 ** 31 - 1) // 10 + 1, 2 ** 40])
def test_row_count_out_of_range_is_refused(built, n_steps):
    _refused(built, b"n_steps", rows=_rows(built, n_steps=n_steps))


def test_a_small_workspace_is_refused(built):
    need = built.lib().cm3_qmix_learner_particle_workspace_bytes(4, 128)
    _refused(built, b"too small", nbytes=need - 4)
    _refused(built, b"too small", nbytes=0)


def _adam(built, **kw):
    d = built.AdamDesc()
    d.lr, d.beta1, d.beta2, d.epsilon, d.n_segments, d.total = 1e-3, 0.9, 0.999, 1e-8, 11, 1000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_adam_validates_before_launching(built):
    handle = built.lib()
    fn = handle.cm3_adam_step_f32

    def refused(needle, desc, segments=FAKE, state=FAKE):
        assert fn(None if desc is None else ctypes.byref(desc), segments, state, None) == -1
        assert needle in handle.cm3_last_error(), handle.cm3_last_error()
    refused(b"null desc", None)
    for kw in ({"lr": float("nan")}, {"beta1": 1.0}, {"beta1": -0.1}, {"beta2": 1.5}, {"epsilon": 0.0}, {"epsilon": -1e-8}):
        refused(b"Adam takes", _adam(built, **kw), segments=None)          # the descriptor first
    refused(b"n_segments must be positive", _adam(built, n_segments=0), segments=None)
    refused(b"segments is NULL", _adam(built, total=0), segments=None)      # pointers before counts
    refused(b"state is NULL", _adam(built, total=0), state=None)
    refused(b"misaligned", _adam(built, total=0), segments=FAKE + 4)
    refused(b"misaligned", _adam(built, total=0), state=FAKE + 4)
    refused(b"total must be positive", _adam(built, total=0))
    refused(b"total must be positive", _adam(built, total=-3))


def test_the_unit_is_built_like_the_matrix_units_and_holds_no_inline_assembly():
    """learner.hip is compiled beside build.sh's loop over the matrix units, with that loop's flags (-ffp-contract=off among them), and
    linked through OBJS (so the post-build lint sees it) and named on the diagnostics line; it and every csrc file it includes hold no
    inline assembly but the two empty scalar-operand statements of common.h."""
    root = os.path.join(ROOT, "cm3_amd", "csrc")
    build = open(os.path.join(root, "build.sh")).read()
    loop = re.search(r"for f in [a-z_ ]+; do\s*\n\s*(\"\$\{HIPCC\}\" \$\{FLAGS\} \$\{PHYS\} \$\{MFMA_FORM\}[^\n]*)\n", build)
    assert loop, "build.sh: the loop that compiles the matrix translation units was not found"
    own = [line for line in build.splitlines() if '"${HERE}/learner.hip"' in line]
    assert len(own) == 1 and own[0].strip() == loop.group(1).strip().replace("${f}", "learner")
    assert re.search(r'^FLAGS="[^"\n]*-ffp-contract=off', build, flags=re.M)
    objs = build[build.index("OBJS=("):]
    assert '"${OBJ}/learner.o"' in objs[:objs.index(")")]
    diag = [line for line in build.splitlines() if "resource_usage.txt" in line and line.startswith("for f in")]
    assert len(diag) == 1 and " learner " in diag[0]
    todo, scanned = ["learner.hip"], []
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
    assert {"actor_common.h", "common.h", "philox.h"} <= set(scanned), scanned
    text = open(os.path.join(root, "learner.hip")).read()
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in text and "atomicAdd" not in text and "unsafeAtomicAdd" not in text


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
    from cm3_amd.qmix import ParticleQmixLearner
    with pytest.raises(Cm3Error, match="takes the main ParticleQmixAgent and the main ParticleQmixMixer, got object"):
        ParticleQmixLearner(object(), _bare("ParticleQmixMixer", 2))
    with pytest.raises(Cm3Error, match="got ParticleQmixAgent and CheckersQmixMixer"):
        ParticleQmixLearner(_bare("ParticleQmixAgent", 2), _bare("CheckersQmixMixer", 2))
    with pytest.raises(Cm3Error, match="the agent is built for 2 agents, the mixer for 3; build both for one agent count"):
        ParticleQmixLearner(_bare("ParticleQmixAgent", 2), _bare("ParticleQmixMixer", 3))
    with pytest.raises(Cm3Error, match="build both on one device"):
        ParticleQmixLearner(_bare("ParticleQmixAgent", 2), _bare("ParticleQmixMixer", 2, "cuda:1"))


def test_the_learner_is_no_device_net_and_has_no_launch_hook():
    import cm3_amd
    from cm3_amd._net import _DeviceNet
    from cm3_amd.qmix import ParticleQmixLearner
    from tests.test_device_net_hooks import HOOKS
    assert cm3_amd.ParticleQmixLearner is ParticleQmixLearner
    assert not issubclass(ParticleQmixLearner, _DeviceNet)
    assert not [h for h in HOOKS if hasattr(ParticleQmixLearner, h)]


def _never(ops, feed):
    raise AssertionError("run was called: the refusal must come first")


def test_train_step_feeds_refuses_a_learner_it_cannot_use():
    from cm3_amd.batch import qmix_train_step_feeds
    from tests.test_qmix_mixer_abi import _host_cols

    class L(object):
        agent = _bare("ParticleQmixAgent", 4)
    cols = _host_cols()
    with pytest.raises(ValueError, match="the Checkers learner is not built"):
        qmix_train_step_feeds({}, _never, 0.99, env="checkers", learner=L())
    with pytest.raises(ValueError, match="pass target_agent and target_mixer"):
        qmix_train_step_feeds(cols, _never, 0.99, learner=L())
    with pytest.raises(ValueError, match="pass target_agent and target_mixer"):
        qmix_train_step_feeds(cols, _never, 0.99, target_agent=_bare("ParticleQmixAgent", 2), learner=L())
    with pytest.raises(ValueError, match="learner is built for 4 agents, the batch has 2"):
        qmix_train_step_feeds(cols, _never, 0.99, target_agent=_bare("ParticleQmixAgent", 2), target_mixer=_bare("ParticleQmixMixer", 2),
                              learner=L())
