"""CPU: the advantage-normalisation oracle (oracle/advantage_oracle.py) -- its working-precision layer against exact rational
arithmetic, its float64 layer's error bounds (they hold, and they are tight enough to catch a wrong result), its agreement
with the host helpers of cm3_amd/shard.py -- and the argument checks of every advantage / copy entry point, which refuse
before any HIP call and so run without a GPU."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import advantage_oracle as ao

REALS = [np.float32, np.float64]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _returns_fraction(x, done, gamma):
    T = len(x)
    out = [Fraction(0)] * T
    g = Fraction(0)
    for t in range(T - 1, -1, -1):
        g = Fraction(x[t]) + (0 if done[t] else Fraction(gamma) * g)
        out[t] = g
    return out


@pytest.mark.parametrize("real", REALS)
def test_hand_computed_returns_and_statistics(real):
    """Dyadic inputs and gamma: every intermediate is exact in float32, so layer (a) must equal rational arithmetic."""
    x = [1.0, 2.0, -3.0, 0.5, 4.0, -1.25]
    done = [0, 1, 0, 0, 1, 0]
    for gamma in (0.5, 0.75, 1.0, 0.0):
        want = _returns_fraction(x, done, gamma)
        got = ao.returns_working(np.array(x, real)[:, None], np.array(done, np.uint8)[:, None], gamma, real)
        assert [Fraction(float(v)) for v in got[:, 0]] == want, gamma
        assert got.dtype == real
    # G = [1 + .5 * 2, 2, -3 + .5 * (.5 + .5 * 4), .5 + .5 * 4, 4, -1.25] at gamma = .5
    assert ao.returns_working(np.array(x, real)[:, None], np.array(done, np.uint8)[:, None], 0.5, real)[:, 0].tolist() == \
        [2.0, 2.0, -1.75, 2.5, 4.0, -1.25]
    # masked entries are +0 and leave the recurrence alone
    valid = np.array([1, 0, 1, 1, 0, 1], np.uint8)[:, None]
    got = ao.returns_working(np.array(x, real)[:, None], np.array(done, np.uint8)[:, None], 0.5, real, valid)[:, 0]
    assert got.tolist() == [2.0, 0.0, -1.75, 2.5, 0.0, -1.25]
    # statistics: (mean, sd) from the moments against exact rationals
    vals = [Fraction(v) for v in (2.0, -1.75, 2.5, -1.25)]
    n = len(vals)
    mean = sum(vals) / n
    var = sum(v * v for v in vals) / n - mean * mean
    m = ao.moments_exact(got[:, None], valid)[0]
    assert (m["s"], m["s2"], m["n"]) == (float(sum(vals)), float(sum(v * v for v in vals)), 4.0)
    mk, sk, nk = ao.stats_from_moments((m["s"], m["s2"], m["n"]))
    assert mk == float(mean) and nk == 4.0
    assert abs(sk - math.sqrt(float(var))) <= 1e-15 * sk
    assert ao.stats_exact(m["vals"]) == (mk, sk)


def test_count_zero_and_one_and_constant_statistics():
    assert ao.stats_from_moments((0.0, 0.0, 0.0)) == (0.0, 0.0, 0.0)
    assert ao.stats_from_moments((-2.5, 6.25, 1.0)) == (-2.5, 0.0, 1.0)
    # constant column: s2 / n - mean^2 may round below zero; the clamp gives sd = 0
    v = np.full(7, 0.1)
    m = ao.moments_exact(v[:, None, None])[0]
    mean, sd, n = ao.stats_from_moments((m["s"], m["s2"], m["n"]))
    assert n == 7.0 and sd >= 0.0 and sd < 1e-8
    # count 0 normalises nothing: every entry is masked -> +0
    y = ao.normalize_working(np.ones((3, 2), np.float32), [(0.0, 0.0, 0.0)], 1e-8, np.float32, np.zeros((3, 2), np.uint8))
    assert (_bits(y) == 0).all()


@pytest.mark.parametrize("real", REALS)
def test_sign_of_zero(real):
    """x = -0 at a done tick gives +0 (x + 0), not x; a masked entry is +0; a normalised zero is +0."""
    x = np.array([[-0.0], [-1.0]], real)
    done = np.array([[1], [0]], np.uint8)
    g = ao.returns_working(x, done, 0.99, real)
    assert _bits(g)[0, 0] == 0 and g[1, 0] == -1.0
    g = ao.returns_working(np.array([[-0.0]], real), np.array([[0]], np.uint8), 0.99, real)      # -0 + gamma * (+0) = +0
    assert _bits(g)[0, 0] == 0
    g = ao.returns_working(np.array([[-0.0], [-0.0]], real), np.array([[0], [1]], np.uint8), 1.0, real)
    assert (_bits(g) == 0).all()
    y = ao.normalize_working(np.array([[-0.0], [2.0]], real), [(2.0, 0.0, 2.0)], 1.0, real, np.array([[0], [1]], np.uint8))
    assert (_bits(y) == 0).all()


def _random_case(rng, real, T, E, C, gamma, offset=0.0, p_done=0.1, p_valid=0.8, K=1):
    x = (rng.standard_normal((K * T, E, C)) + offset).astype(np.float32).astype(real)
    done = (rng.random((K * T, E)) < p_done).astype(np.uint8)
    valid = (rng.random((K * T, E)) < p_valid).astype(np.uint8)
    return x, done, valid


def _check_against_exact(x, done, valid, gamma, real, eps, K, moments_sum):
    """Layer (a) as the 'kernel', layer (b) as the judge; moments_sum(values) stands for the kernel's summation order.
    Returns the worst err / bound ratios."""
    gw = ao.returns_working(x, done, gamma, real, None, K, masked=False)
    ge = ao.returns_exact(x, done, gamma, K)
    b = ao.returns_bound(gw, ge, done, gamma, real, K)
    err = np.abs(gw.astype(np.float64) - ge)
    assert (err <= b).all(), float((err / b).max())
    ratios = {"returns": float((err / b).max())}
    g = ao.returns_working(x, done, gamma, real, valid, K)
    worst_norm = 0.0
    for k, m in enumerate(ao.moments_exact(g, valid, K)):
        s, s2 = moments_sum(m["vals"]), moments_sum(m["vals"] * m["vals"])
        ds, ds2 = ao.moments_bound(m)
        assert abs(s - m["s"]) <= ds and abs(s2 - m["s2"]) <= ds2
        mean_k, sd_k, n_k = ao.stats_from_moments((s, s2, m["n"]))
        mean_x, sd_x = ao.stats_exact(m["vals"])
        dmean, dsd = ao.stats_bound((s, s2, m["n"]), (mean_k, sd_k), ds, ds2, mean_x, sd_x)
        assert abs(mean_k - mean_x) <= dmean and abs(sd_k - sd_x) <= dsd
        ratios["sd"] = max(ratios.get("sd", 0.0), abs(sd_k - sd_x) / dsd)
        y = ao.normalize_working(g, np.array([(mean_k, sd_k, n_k)] * K), eps, real, valid, K)
        yk = y.reshape(K, -1, *y.shape[1:])[k]
        gk = g.reshape(K, -1, *g.shape[1:])[k].astype(np.float64)
        ye = (gk - mean_x) / (sd_x + eps)
        nb = ao.normalized_bound(gk, ye, mean_k, sd_k, eps, real, dmean, dsd, mean_x, sd_x)
        vk = valid.reshape(K, -1, valid.shape[1])[k].astype(bool)[..., None]
        vk = np.broadcast_to(vk, yk.shape)
        e = np.abs(yk.astype(np.float64) - ye)[vk]
        assert (e <= nb[vk]).all()
        if e.size:
            worst_norm = max(worst_norm, float((e / nb[vk]).max()))
    ratios["normalized"] = worst_norm
    return ratios


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("gamma", [0.0, 0.97, 0.99, 1.0])
def test_bounds_hold_on_random_inputs(real, gamma):
    rng = np.random.default_rng(int(gamma * 100) + (7 if real == np.float32 else 0))
    for (T, E, C, K, offset) in [(1, 5, 1, 1, 0.0), (41, 7, 2, 1, 0.0), (9, 6, 4, 3, 3.0), (130, 3, 1, 2, 20.0)]:
        x, done, valid = _random_case(rng, real, T, E, C, gamma, offset, K=K)
        _check_against_exact(x, done, valid, gamma, real, 1e-8, K, lambda v: float(np.cumsum(v)[-1]) if v.size else 0.0)


@pytest.mark.parametrize("real", REALS)
def test_bounds_are_not_vacuous(real):
    """The bounds are a handful of roundings wide: a gamma off by a few ulps of float32, a dropped done flag, a sum missing
    one term or a statistic off by the float32 rounding of the mean all fall outside them."""
    rng = np.random.default_rng(3)
    u = ao.unit_roundoff(real)
    T, E, C, gamma = 64, 9, 2, 0.97
    x, done, valid = _random_case(rng, real, T, E, C, gamma, offset=1.0, p_done=0.05)
    gw = ao.returns_working(x, done, gamma, real, None, 1, masked=False)
    ge = ao.returns_exact(x, done, gamma)
    b = ao.returns_bound(gw, ge, done, gamma, real)
    assert float((b / np.maximum(np.abs(ge), 1.0)).max()) < 8 * T * u
    # a wrong gamma is caught (float64: off by 64 ulps; float32: 0.9699 for 0.97) ...
    g_bad = gamma * (1 - 64 * u) if real == np.float64 else 0.9699
    bad = ao.returns_working(x, done, g_bad, real, None, 1, masked=False)
    assert (np.abs(bad.astype(np.float64) - ge) > b).any()
    # ... and so is one ignored done flag
    d2 = done.copy()
    t, e = np.argwhere(done[1:] != 0)[0]
    d2[t + 1, e] = 0
    bad = ao.returns_working(x, d2, gamma, real, None, 1, masked=False)
    assert (np.abs(bad.astype(np.float64) - ge) > b).any()
    # moments: one element left out of the sum is caught
    g = ao.returns_working(x, done, gamma, real, valid)
    m = ao.moments_exact(g, valid)[0]
    ds, ds2 = ao.moments_bound(m)
    assert abs(math.fsum(m["vals"][1:]) - m["s"]) > ds
    # the sd bound stays far below the spread: a relative error of 1e-3 is caught (with mean^2 / var ~ 1)
    mean_x, sd_x = ao.stats_exact(m["vals"])
    mean_k, sd_k, _ = ao.stats_from_moments((m["s"], m["s2"], m["n"]))
    dmean, dsd = ao.stats_bound((m["s"], m["s2"], m["n"]), (mean_k, sd_k), ds, ds2, mean_x, sd_x)
    assert dsd < 1e-10 * sd_x and dmean < 1e-10 * max(abs(mean_x), sd_x)
    # the normalised values: using the float32-rounded sd in the float64 computation is caught
    if real == np.float64:
        gk = g.astype(np.float64)
        ye = (gk - mean_x) / (sd_x + 1e-8)
        nb = ao.normalized_bound(gk, ye, mean_k, sd_k, 1e-8, real, dmean, dsd, mean_x, sd_x)
        y_bad = (gk - mean_k) / (float(np.float32(sd_k)) + 1e-8)
        assert (np.abs(y_bad - ye) > nb).any()


def test_sd_bound_grows_with_mean_squared_over_variance():
    """Returns with a large common offset: the one-pass formula loses about u64 mean^2 / sd of the sd; the bound covers it
    and says so (it is far wider than at offset 0)."""
    rng = np.random.default_rng(5)
    widths = []
    for offset in (0.0, 1e4):
        v = rng.standard_normal(4000) * 0.01 + offset
        m = ao.moments_exact(v[:, None, None])[0]
        s, s2 = float(np.cumsum(v)[-1]), float(np.cumsum(v * v)[-1])
        ds, ds2 = ao.moments_bound(m)
        mean_k, sd_k, _ = ao.stats_from_moments((s, s2, m["n"]))
        mean_x, sd_x = ao.stats_exact(m["vals"])
        dmean, dsd = ao.stats_bound((s, s2, m["n"]), (mean_k, sd_k), ds, ds2, mean_x, sd_x)
        assert abs(sd_k - sd_x) <= dsd and abs(mean_k - mean_x) <= dmean
        widths.append(dsd / sd_x)
    assert widths[1] > 1e6 * widths[0]


def test_parts_from_shards_layout_and_fold():
    rng = np.random.default_rng(11)
    g = rng.standard_normal((2 * 5, 13, 2))
    valid = (rng.random((10, 13)) < 0.7).astype(np.uint8)
    parts, abs_ = ao.shard_moments(g, valid, 2, 3)
    assert parts.shape == (3, 2, 3) and parts.flags.c_contiguous and abs_.shape == (3, 2, 2)
    whole = ao.moments_exact(g, valid, 2)
    for k in range(2):
        tot = ao.fold_parts(parts, k)
        assert tot[2] == whole[k]["n"]
        assert abs(tot[0] - whole[k]["s"]) <= 3 * ao.U64 * whole[k]["abs_s"]
    with pytest.raises(ValueError):
        ao.parts_from_shards(np.zeros((2, 3)))


# ---- agreement with the host helpers of cm3_amd/shard.py (CPU tensors) ----

@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("C", [1, 3])
def test_host_helpers_agree_with_the_oracle(real, C):
    torch = pytest.importorskip("torch")
    from cm3_amd.shard import global_moments, normalize_advantages, returns_to_go
    rng = np.random.default_rng(C)
    T, E, gamma = 33, 50, 0.97
    x, done, valid = _random_case(rng, real, T, E, C, gamma, offset=0.5)
    x = np.abs(x) + real(0.25)        # no -0 inputs: returns_to_go multiplies by (1 - done), -0 + (-0) stays -0 there
    xs = x if C > 1 else x[..., 0]
    tx = torch.from_numpy(xs.copy())
    # returns: the helper is the same recurrence in the same precision (gamma rounded to the tensor's real) -> same bits
    want = ao.returns_working(xs, done, gamma, real)
    got = returns_to_go(tx, torch.from_numpy(done), gamma=gamma).numpy()
    assert np.array_equal(_bits(got), _bits(want))
    # statistics: the count is exact, mean / sd within the oracle's bounds (torch sums in its own order)
    g = ao.returns_working(xs, done, gamma, real, valid)
    tg, tv = torch.from_numpy(g.copy()), torch.from_numpy(valid.astype(bool))
    mean_t, sd_t, n_t = (float(v) for v in global_moments(tg, tv))
    m = ao.moments_exact(g, valid)[0]
    assert n_t == m["n"]
    ds, ds2 = ao.moments_bound(m)
    mean_x, sd_x = ao.stats_exact(m["vals"])
    s_t, s2_t = mean_t * m["n"], (sd_t * sd_t + mean_t * mean_t) * m["n"]
    dmean, dsd = ao.stats_bound((s_t, s2_t, m["n"]), (mean_t, sd_t), ds, ds2, mean_x, sd_x)
    assert abs(mean_t - mean_x) <= dmean and abs(sd_t - sd_x) <= 2 * dsd
    # normalisation: the helper's expression is layer (a)'s, bit for bit, given the same statistics
    y = normalize_advantages(tg, tv, eps=1e-8).numpy()
    want = ao.normalize_working(g, [(mean_t, sd_t, n_t)], 1e-8, real, valid)
    assert np.array_equal(_bits(y), _bits(want))


# ---- argument checks of advantage.hip and cm3_copy_list (refused before any HIP call) ----

@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from cm3_amd import _lib
    return _lib


FAKE = 0x10000      # non-NULL, 16-byte aligned placeholder: never dereferenced on a refused call


def _refused(built, rc, text):
    assert rc == -1, rc
    assert text.encode() in built.lib().cm3_last_error(), built.lib().cm3_last_error()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_advantage_entry_points_refuse_bad_shapes(built, sfx):
    lib = built.lib()
    f = FAKE
    for T, E, C in [(0, 4, 1), (4, 0, 1), (4, 4, 0), (-1, 4, 1)]:
        _refused(built, getattr(lib, "cm3_returns_moments_" + sfx)(f, f, 0, f, f, f, T, E, C, 0.99, None), "must be positive")
        _refused(built, getattr(lib, "cm3_returns_normalize_" + sfx)(f, f, 0, f, f, f, f, T, E, C, 0.99, 1e-8, 1, None, None),
                 "must be positive")
        _refused(built, getattr(lib, "cm3_returns_normalize_segments_" + sfx)(f, f, 0, f, f, f, f, T, 2, E, C, 0.99, 1e-8, 1,
                                                                                None, None), "must be positive")
    for K in (0, 4097, -1):
        _refused(built, getattr(lib, "cm3_returns_normalize_segments_" + sfx)(f, f, 0, f, f, f, f, 4, K, 4, 1, 0.99, 1e-8, 1,
                                                                                None, None), "n_segments")
        _refused(built, getattr(lib, "cm3_normalize_segments_" + sfx)(f, 0, f, 1, K, 0, 16, 1, 1e-8, 1, None), "n_segments")
    _refused(built, getattr(lib, "cm3_returns_moments_" + sfx)(0, f, 0, f, f, f, 4, 4, 1, 0.99, None), "null pointer")
    _refused(built, getattr(lib, "cm3_returns_normalize_" + sfx)(f, f, 0, f, 0, f, f, 4, 4, 1, 0.99, 1e-8, 1, None, None),
             "null pointer")
    # cm3_normalize_*: n_parts, n_elem, C and -- new -- n_elem a multiple of C (the mask is [n_elem / C] per segment)
    _refused(built, getattr(lib, "cm3_normalize_" + sfx)(f, 0, f, 0, 0, 16, 1, 1e-8, 1, None), "n_parts")
    _refused(built, getattr(lib, "cm3_normalize_" + sfx)(f, 0, 0, 1, 0, 16, 1, 1e-8, 1, None), "n_parts")
    _refused(built, getattr(lib, "cm3_normalize_" + sfx)(0, 0, f, 1, 0, 16, 1, 1e-8, 1, None), "null pointer")
    _refused(built, getattr(lib, "cm3_normalize_" + sfx)(f, 0, f, 1, 0, 0, 1, 1e-8, 1, None), "must be positive")
    _refused(built, getattr(lib, "cm3_normalize_" + sfx)(f, 0, f, 1, 0, 16, 0, 1e-8, 1, None), "must be positive")
    for n_elem, C in [(15, 4), (7, 2), (65, 8)]:
        _refused(built, getattr(lib, "cm3_normalize_" + sfx)(f, f, f, 1, 0, n_elem, C, 1e-8, 1, None), "multiple of C")
        _refused(built, getattr(lib, "cm3_normalize_segments_" + sfx)(f, f, f, 2, 3, 0, n_elem, C, 1e-8, 1, None),
                 "multiple of C")


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_copy_shift_is_refused_unless_aligned_and_sized(built, sfx):
    lib = built.lib()
    f = FAKE

    def call(cs):
        return getattr(lib, "cm3_returns_normalize_" + sfx)(f, f, 0, f, f, f, f, 4, 4, 1, 0.99, 1e-8, 1, ctypes.byref(cs), None)

    def shift(n, over=None):
        cs = built.CopyShift()
        cs.n = n
        for r in range(min(max(n, 0), 4)):
            cs.first_dst[r], cs.mid[r], cs.last_src[r], cs.bytes[r] = f + 0x1000 * r, f + 0x10000, f + 0x20000, 64
        for (field, r), v in (over or {}).items():
            getattr(cs, field)[r] = v
        return cs
    _refused(built, call(shift(5)), "0..4 regions")
    _refused(built, call(shift(-1)), "0..4 regions")
    _refused(built, call(shift(2, {("bytes", 1): 40})), "region 1 is not 16-byte aligned")
    _refused(built, call(shift(3, {("first_dst", 2): f + 4})), "region 2 is not 16-byte aligned")
    _refused(built, call(shift(1, {("mid", 0): f + 8})), "region 0 is not 16-byte aligned")
    _refused(built, call(shift(4, {("last_src", 3): f + 12})), "region 3 is not 16-byte aligned")
    _refused(built, call(shift(2, {("mid", 1): 0})), "null region 1")
    seg = getattr(lib, "cm3_returns_normalize_segments_" + sfx)(f, f, 0, f, f, f, f, 4, 2, 4, 1, 0.99, 1e-8, 1,
                                                               ctypes.byref(shift(1, {("bytes", 0): 8})), None)
    _refused(built, seg, "region 0 is not 16-byte aligned")


def test_copy_list_is_refused_unless_one_to_eight_aligned_regions(built):
    from ctypes import c_size_t, c_void_p
    lib = built.lib()

    def call(n, dst, src, nb):
        k = max(len(dst), 1)
        return lib.cm3_copy_list(n, (c_void_p * k)(*dst), (c_void_p * k)(*src), (c_size_t * k)(*nb), None)
    regions = lambda n: ([FAKE + 0x1000 * r for r in range(n)], [FAKE + 0x100000 + 0x1000 * r for r in range(n)], [16] * n)  # noqa: E731
    _refused(built, call(0, *regions(1)), "1..8 regions")
    _refused(built, call(9, *regions(9)), "1..8 regions")
    _refused(built, call(-1, *regions(1)), "1..8 regions")
    d, s, nb = regions(3)
    nb[2] = 24
    _refused(built, call(3, d, s, nb), "region 2 is not 16-byte aligned")
    d, s, nb = regions(2)
    d[1] += 4
    _refused(built, call(2, d, s, nb), "region 1 is not 16-byte aligned")
    d, s, nb = regions(8)
    s[7] += 8
    _refused(built, call(8, d, s, nb), "region 7 is not 16-byte aligned")
    d, s, nb = regions(2)
    s[0] = 0
    _refused(built, call(2, d, s, nb), "null region 0")
    assert lib.cm3_copy_list(2, None, None, None, None) == -1
