"""GPU: the advantage-normalisation kernels (cm3_amd/csrc/advantage.hip) against the NumPy oracle oracle/advantage_oracle.py.

Every case drives the raw C ABI on host-generated inputs (seeded NumPy) and asserts
  - layer (a): returns and normalised values bit for bit equal to the working-precision restatement (given the kernel's own
    statistics), and the statistics equal to the kernels' expressions over the kernel's own moments;
  - layer (b): moments, mean / sd and normalised values within bounds derived per case from a float64 / exact reference;
  - identical moment bits from cm3_returns_moments_*, cm3_returns_normalize_* and the segmented entry, and the arrival counter
    of cm3_returns_moments_* back at 0 after every call (the zero-once scratch contract of include/cm3_amd.h);
  - the launch path the case is named for (cm3_last_kernel_variant: launch A's build and its number of partial blocks).
The matrix is a covering set over T, the column count (block and path edges), C, done / valid patterns, gamma, segments,
n_parts, a misaligned / odd-length output and the copy shift -- the largest column counts at small T, the longest T at few
columns.  Set CM3_ADVANTAGE_ERRORS=<file> to write the worst observed errors (per dtype and path) as JSON."""
import ctypes
import json
import os
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import advantage_oracle as ao

pytestmark = pytest.mark.gpu

EPS = 1e-8
Case = namedtuple("Case", "T K E C done valid gamma shift misalign n_parts offset const")
CASES = {
    # name: T per segment, K segments, E, C, done, valid, gamma, copy shift region bytes, misaligned out, n_parts, offset, constant x
    "t1_one_column":        Case(1, 1, 1, 1, "random", "none", 0.99, (), False, (), 0.0, False),
    "t7_odd_misaligned":    Case(7, 1, 63, 1, "all", "random", 0.0, (), True, (), 0.0, False),
    "t8_count0":            Case(8, 1, 16, 4, "none", "zero", 1.0, (), False, (2,), 0.0, False),
    "t9_count1_last_done":  Case(9, 1, 65, 1, "last", "one", 0.97, (), False, (), 0.0, False),
    "t33_constant":         Case(33, 1, 255, 1, "all", "all", 0.99, (), False, (), 0.0, True),
    "t40_shift_padded":     Case(40, 1, 257, 1, "random", "random", 0.99, (1048576 + 4112,), False, (), 2.0, False),
    "t41_walk_shift4":      Case(41, 1, 128, 2, "random", "random", 0.97, (16, 4096, 48, 2097168), False, (), 0.0, False),
    "t64_walk_constant":    Case(64, 1, 1, 1, "none", "none", 0.0, (), False, (), 0.0, True),
    "t330_walk_k2":         Case(330, 2, 16, 4, "sparse", "random", 0.99, (), False, (), 1.0, False),
    "t330_walk_gamma1":     Case(330, 1, 7, 8, "sparse", "none", 1.0, (), True, (), 0.0, False),
    "c4_k10_mask_shift3":   Case(33, 10, 4096, 4, "random", "random", 0.99, (65536, 16, 4096), False, (), 0.0, False),
    "keep_262144_cols":     Case(1, 1, 32768, 8, "random", "random", 0.97, (), False, (), 0.0, False),
    "walk_262145_cols_k2":  Case(2, 2, 262145, 1, "random", "random", 0.99, (), False, (), 0.0, False),
    "walk_560008_cols":     Case(1, 1, 70001, 8, "none", "none", 0.97, (), True, (), 0.0, False),
    "k4096_mask":           Case(2, 4096, 16, 4, "random", "random", 0.99, (), False, (), 0.0, False),
    "parts_k1":             Case(9, 1, 100, 2, "random", "random", 0.97, (), False, (1, 2, 8), 3.0, False),
    "parts_k5":             Case(33, 5, 50, 4, "random", "random", 0.99, (), False, (1, 2, 8), 3.0, False),
}
REALS = {"f32": np.float32, "f64": np.float64}
WORST = {}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    yield _lib
    path = os.environ.get("CM3_ADVANTAGE_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def moments_scratch(lib):
    """ONE scratch for every cm3_returns_moments_* call of the module, zeroed once: the kernel must leave its counter at 0."""
    return torch.zeros(lib.lib().cm3_returns_scratch_bytes() // 8, dtype=torch.float64, device="cuda")


def _note(sfx, path, what, err, bound):
    """Worst |kernel - exact| of this dtype / path / quantity (with the bound at that element) and the worst err / bound."""
    err, bound = np.atleast_1d(np.asarray(err, np.float64)), np.atleast_1d(np.asarray(bound, np.float64))
    w = WORST.setdefault("%s/%s/%s" % (sfx, path, what), {"err": 0.0, "bound_at_err": 0.0, "err_over_bound": 0.0})
    i = int(np.argmax(err))
    if err[i] >= w["err"]:
        w["err"], w["bound_at_err"] = float(err[i]), float(bound[i])
    pos = bound > 0
    if pos.any():
        w["err_over_bound"] = max(w["err_over_bound"], float((err[pos] / bound[pos]).max()))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _inputs(case, real, seed):
    rng = np.random.default_rng(seed)
    TT, E, C = case.T * case.K, case.E, case.C
    if case.const:
        x = np.full((TT, E, C), 0.75, np.float32)
    else:
        x = (rng.standard_normal((TT, E, C)) * 2.0 + case.offset).astype(np.float32)
        x[rng.random(x.shape) < 0.01] = -0.0                 # the sign of zero counts (x = -0 at a done tick gives +0)
    done = {"random": lambda: rng.random((TT, E)) < 0.1, "sparse": lambda: rng.random((TT, E)) < 0.01,
            "none": lambda: np.zeros((TT, E), bool), "all": lambda: np.ones((TT, E), bool),
            "last": lambda: np.tile(np.arange(TT)[:, None] % case.T == case.T - 1, (1, E))}[case.done]()
    valid = None
    if case.valid != "none":
        valid = {"random": lambda: rng.random((TT, E)) < 0.8, "zero": lambda: np.zeros((TT, E), bool),
                 "all": lambda: np.ones((TT, E), bool), "one": lambda: np.zeros((TT, E), bool)}[case.valid]()
        if case.valid == "one":
            valid[TT // 2, E // 3] = True
        valid = valid.astype(np.uint8)
    return x.astype(real), done.astype(np.uint8), valid


def _expected_path(case):
    cols = case.E * case.C
    blocks = (cols + 255) // 256
    if case.T <= 40 and blocks <= 1024:
        return "k_returns_partials_keep", (256 if case.shift and blocks < 256 else blocks)
    return "k_returns_partials", min(blocks, 1024)


def _device_out(n, dtype, misalign):
    """n elements; misalign: a view one element (4 / 8 bytes) past the allocation's 16-byte boundary (float32 then takes the
    scalar fold path)."""
    if not misalign:
        return torch.empty(n, dtype=dtype, device="cuda")
    return torch.empty(n + 1, dtype=dtype, device="cuda")[1:]


def _stats_checks(sfx, path, mom_k, st_k, vals, ds, ds2):
    """Layer (a) statistics from the kernel's moments + layer (b) bounds; returns (mean_x, sd_x, dmean, dsd)."""
    mean_w, sd_w, n_w = ao.stats_from_moments(mom_k)
    assert st_k[0] == mean_w and st_k[2] == n_w
    assert abs(st_k[1] - sd_w) <= np.spacing(sd_w)
    mean_x, sd_x = ao.stats_exact(vals)
    dmean, dsd = ao.stats_bound(mom_k, st_k, ds, ds2, mean_x, sd_x)
    em, es = abs(st_k[0] - mean_x), abs(st_k[1] - sd_x)
    assert em <= dmean and es <= dsd, (em, dmean, es, dsd)
    _note(sfx, path, "mean", em, dmean)
    _note(sfx, path, "sd", es, dsd)
    return mean_x, sd_x, dmean, dsd


def _normalized_checks(sfx, path, real, y_seg, g_seg, v_seg, st_k, mean_x, sd_x, dmean, dsd):
    g = g_seg.astype(np.float64)
    ye = (g - mean_x) / (sd_x + EPS)
    nb = ao.normalized_bound(g, ye, float(st_k[0]), float(st_k[1]), EPS, real, dmean, dsd, mean_x, sd_x)
    sel = np.ones(g.shape, bool) if v_seg is None else np.broadcast_to(v_seg.astype(bool)[..., None], g.shape)
    if sel.any():
        e = np.abs(y_seg.astype(np.float64) - ye)[sel]
        b = nb[sel]
        assert (e <= b).all(), float((e / b).max())
        _note(sfx, path, "normalized", e, b)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_advantage_kernels_against_the_oracle(lib, moments_scratch, name, sfx):
    case = CASES[name]
    real = REALS[sfx]
    dtype = torch.float32 if sfx == "f32" else torch.float64
    L = lib.lib()
    T, K, E, C = case.T, case.K, case.E, case.C
    TT, cols = T * K, E * C
    n_elem = T * cols
    x_h, done_h, valid_h = _inputs(case, real, seed=zlib.crc32(name.encode()) + len(sfx))
    x = torch.from_numpy(x_h).cuda()
    done = torch.from_numpy(done_h).cuda()
    valid = None if valid_h is None else torch.from_numpy(valid_h).cuda()
    stream = lib.current_stream_handle(x.device)
    kern, n_partials = _expected_path(case)
    path = kern.replace("k_returns_partials_keep", "keep").replace("k_returns_partials", "walk")

    # ---- the segmented entry: apply = 0 (raw returns + copy shift), then apply = 1 ----
    out = _device_out(TT * cols, dtype, case.misalign)
    scratch = torch.zeros(L.cm3_returns_segments_scratch_bytes(K) // 8, dtype=torch.float64, device="cuda")
    buf = torch.zeros(4, K, 3, dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(len(name))
    regions = [(torch.zeros(b // 4, device="cuda"), torch.randn(b // 4, generator=g, device="cuda"),
                torch.randn(b // 4, generator=g, device="cuda")) for b in case.shift]
    m0 = [m.clone() for _, m, _ in regions]
    c0 = [c.clone() for _, _, c in regions]
    cs = lib.CopyShift()
    cs.n = len(regions)
    for r, (a, m, c) in enumerate(regions):
        cs.first_dst[r], cs.mid[r], cs.last_src[r], cs.bytes[r] = a.data_ptr(), m.data_ptr(), c.data_ptr(), case.shift[r]
    seg = getattr(L, "cm3_returns_normalize_segments_" + sfx)

    def seg_call(o, apply, mom, st, shift):
        lib.check(seg(x.data_ptr(), done.data_ptr(), lib.ptr(valid), o.data_ptr(), scratch.data_ptr(), mom.data_ptr(),
                      st.data_ptr(), T, K, E, C, case.gamma, EPS, apply, ctypes.byref(shift) if shift is not None else None,
                      stream))
    seg_call(out, 0, buf[0], buf[1], cs)
    assert lib.last_kernel_variant().startswith("%s<%s,N=%d," % (kern, sfx, n_partials)), lib.last_kernel_variant()
    torch.cuda.synchronize()
    ret = out.cpu().numpy().reshape(x_h.shape)
    for (a, m, c), mm, cc in zip(regions, m0, c0):        # first_dst <- mid, then mid <- last_src; last_src untouched
        assert torch.equal(a, mm) and torch.equal(m, cc) and torch.equal(c, cc)
    seg_call(out, 1, buf[2], buf[3], None)
    torch.cuda.synchronize()
    y = out.cpu().numpy().reshape(x_h.shape)
    bh = buf.cpu().numpy()
    mom, st = bh[0], bh[1]
    assert np.array_equal(_bits(bh[2]), _bits(mom)) and np.array_equal(_bits(bh[3]), _bits(st))

    # ---- layer (a): bit for bit ----
    want = ao.returns_working(x_h, done_h, case.gamma, real, valid_h, K)
    assert np.array_equal(_bits(ret), _bits(want)), np.argwhere(_bits(ret) != _bits(want))[:5]
    want_y = ao.normalize_working(ret, st, EPS, real, valid_h, K)
    assert np.array_equal(_bits(y), _bits(want_y)), np.argwhere(_bits(y) != _bits(want_y))[:5]

    # ---- layer (b): bounds ----
    gw = ao.returns_working(x_h, done_h, case.gamma, real, None, K, masked=False)
    ge = ao.returns_exact(x_h, done_h, case.gamma, K)
    rb = ao.returns_bound(gw, ge, done_h, case.gamma, real, K)
    sel = np.ones(ret.shape, bool) if valid_h is None else np.broadcast_to(valid_h.astype(bool)[..., None], ret.shape)
    if sel.any():
        e = np.abs(ret.astype(np.float64) - ge)[sel]
        assert (e <= rb[sel]).all()
        _note(sfx, path, "returns", e, rb[sel])
    exact = ao.moments_exact(ret, valid_h, K)
    rs, ys = ret.reshape(K, T, E, C), y.reshape(K, T, E, C)
    vs = None if valid_h is None else valid_h.reshape(K, T, E)
    for k, m in enumerate(exact):
        assert mom[k, 2] == m["n"] and st[k, 2] == m["n"]
        ds, ds2 = ao.moments_bound(m)
        assert abs(mom[k, 0] - m["s"]) <= ds and abs(mom[k, 1] - m["s2"]) <= ds2
        _note(sfx, path, "sum", abs(mom[k, 0] - m["s"]), ds)
        mean_x, sd_x, dmean, dsd = _stats_checks(sfx, path, mom[k], st[k], m["vals"], ds, ds2)
        _normalized_checks(sfx, path, real, ys[k], rs[k], None if vs is None else vs[k], st[k], mean_x, sd_x, dmean, dsd)

    # ---- the other entry points: same moment bits, same returns / normalised bits, counter back at 0 ----
    ks = range(K) if K <= 10 else (0, K // 2, K - 1)
    counter = moments_scratch.view(torch.int32)[3 * 1024 * 2]
    for k in ks:
        xk, dk = x[k * T:(k + 1) * T], done[k * T:(k + 1) * T]
        vk = None if valid is None else valid[k * T:(k + 1) * T]
        o2 = torch.empty(n_elem, dtype=dtype, device="cuda")
        b2 = torch.zeros(4, 3, dtype=torch.float64, device="cuda")
        lib.check(getattr(L, "cm3_returns_moments_" + sfx)(
            xk.data_ptr(), dk.data_ptr(), lib.ptr(vk), o2.data_ptr(), moments_scratch.data_ptr(), b2[0].data_ptr(),
            T, E, C, case.gamma, stream))
        torch.cuda.synchronize()
        assert int(counter) == 0
        assert np.array_equal(_bits(o2.cpu().numpy()), _bits(rs[k].ravel()))
        lib.check(getattr(L, "cm3_normalize_" + sfx)(o2.data_ptr(), lib.ptr(vk), b2[0].data_ptr(), 1, b2[1].data_ptr(), n_elem, C,
                                                   EPS, 1, stream))
        o3 = _device_out(n_elem, dtype, case.misalign)
        s3 = torch.zeros(L.cm3_returns_scratch_bytes() // 8, dtype=torch.float64, device="cuda")
        lib.check(getattr(L, "cm3_returns_normalize_" + sfx)(
            xk.data_ptr(), dk.data_ptr(), lib.ptr(vk), o3.data_ptr(), s3.data_ptr(), b2[2].data_ptr(), b2[3].data_ptr(),
            T, E, C, case.gamma, EPS, 1, None, stream))
        kern1, np1 = _expected_path(case._replace(shift=()))
        assert lib.last_kernel_variant().startswith("%s<%s,N=%d," % (kern1, sfx, np1)), lib.last_kernel_variant()
        torch.cuda.synchronize()
        b2h = b2.cpu().numpy()
        for row in (b2h[0], b2h[2]):
            assert np.array_equal(_bits(row), _bits(mom[k]))
        for row in (b2h[1], b2h[3]):
            assert np.array_equal(_bits(row), _bits(st[k]))
        assert np.array_equal(_bits(o2.cpu().numpy()), _bits(ys[k].ravel()))
        assert np.array_equal(_bits(o3.cpu().numpy()), _bits(ys[k].ravel()))

    # ---- several ranks: cm3_normalize_segments_* over [ranks][K][3] parts of exact per-shard moments ----
    for n_parts in case.n_parts:
        parts_h, abs_h = ao.shard_moments(ret, valid_h, K, n_parts)
        parts = torch.from_numpy(parts_h).cuda()
        z = torch.from_numpy(ret.copy()).cuda()
        st4 = torch.zeros(K, 3, dtype=torch.float64, device="cuda")
        lib.check(getattr(L, "cm3_normalize_segments_" + sfx)(z.data_ptr(), lib.ptr(valid), parts.data_ptr(), n_parts, K,
                                                            st4.data_ptr(), n_elem, C, EPS, 1, stream))
        torch.cuda.synchronize()
        st4h, zh = st4.cpu().numpy(), z.cpu().numpy()
        assert np.array_equal(_bits(zh), _bits(ao.normalize_working(ret, st4h, EPS, real, valid_h, K)))
        for k, m in enumerate(exact):
            tot = ao.fold_parts(parts_h, k)
            assert tot[2] == m["n"]
            # each part is correctly rounded (u64 |part|), the rank-ordered fold adds (n_parts - 1) u64 sum|part|
            ds = (n_parts * ao.U64) * float(abs_h[:, k, 0].sum()) + ao.U64 * abs(m["s"])
            ds2 = (n_parts * ao.U64) * float(abs_h[:, k, 1].sum()) + ao.U64 * abs(m["s2"])
            mean_x, sd_x, dmean, dsd = _stats_checks(sfx, "parts%d" % n_parts, tot, st4h[k], m["vals"], ds, ds2)
            _normalized_checks(sfx, "parts%d" % n_parts, real, zh.reshape(K, T, E, C)[k], rs[k], None if vs is None else vs[k],
                               st4h[k], mean_x, sd_x, dmean, dsd)

    # ---- the Python front ends: normalized_returns (one segment, with the mask), ReturnsNormalizer (segments, no mask) ----
    from cm3_amd.shard import ReturnsNormalizer, normalized_returns
    if K == 1:
        xt = x[..., 0] if C == 1 else x
        yt, (mean_t, sd_t, n_t) = normalized_returns(xt, done, valid, gamma=case.gamma, eps=EPS)
        assert np.array_equal(_bits(yt.cpu().numpy().reshape(y.shape)), _bits(y))
        assert (float(mean_t), float(sd_t), float(n_t)) == tuple(st[0])
    if valid_h is None:
        rn = ReturnsNormalizer(x, done, case.gamma, EPS, True, segments=K)
        rn.enqueue_fused(stream)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(rn.out.cpu().numpy()), _bits(y))
        assert np.array_equal(_bits(rn.buf.cpu().numpy().reshape(2, K, 3)), _bits(bh[:2]))


@pytest.mark.parametrize("sizes", [(16,), (0, 16), (4096, 0, 8 * 2 ** 20 + 4112), (48, 16, 32, 2 ** 20, 0, 64, 4096, 8 * 2 ** 20 + 16)])
def test_copy_list_equals_torch_copies(lib, sizes):
    """cm3_copy_list against torch copies: 1..8 regions of 0, 16 bytes .. > 8 MiB (more than 2048 blocks x 4 KiB, so the loop
    strides); the bytes behind every region stay untouched."""
    g = torch.Generator(device="cuda").manual_seed(len(sizes))
    guard = 256
    srcs = [torch.randint(0, 255, (b + guard,), generator=g, device="cuda", dtype=torch.uint8) for b in sizes]
    dsts = [torch.randint(0, 255, (b + guard,), generator=g, device="cuda", dtype=torch.uint8) for b in sizes]
    before = [d.clone() for d in dsts]
    n = len(sizes)
    dp = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dsts])
    sp = (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs])
    nb = (ctypes.c_size_t * n)(*sizes)
    lib.check(lib.lib().cm3_copy_list(n, dp, sp, nb, lib.current_stream_handle(torch.device("cuda"))))
    torch.cuda.synchronize()
    for b, s, d, d0 in zip(sizes, srcs, dsts, before):
        want = torch.cat([s[:b], d0[b:]])
        assert torch.equal(d, want), b
