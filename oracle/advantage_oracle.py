"""TEST INFRASTRUCTURE ONLY -- NumPy reference of the advantage-normalisation kernels (cm3_amd/csrc/advantage.hip).

Two layers.

(a) A working-precision restatement: the spec the kernels implement, operation for operation, in the working real R
    (np.float32 / np.float64).  Per segment of T ticks and per (env, channel) column
        G[t] = x[t] + (0 if done[t] else R(gamma) * G[t+1]),   G[T] = 0
    (exactly this form: x = -0.0 with done gives +0.0), invalid entries -> +0; the statistics come from the float64 moments
    (sum, sum of squares, count) as the kernels derive them, and the normalisation is (x - R(mean)) / R(sd + eps) in R.
    The library is built with -ffp-contract=off, so -- given the kernel's own statistics -- returns and normalised values match
    this layer bit for bit.

(b) An exact / float64 reference with error bounds derived per case: float64 returns with the UNROUNDED gamma and a running
    forward-error bound (one product and one sum per step, plus the systematic |R(gamma) - gamma| |G[t+1]| term of a float32
    gamma); math.fsum moments over the kernel's own returns with the summation bound (n - 1) u64 sum|.|; exact two-pass mean /
    sd with the bound of the one-pass formula s2 / n - mean^2 (which grows with mean^2 / var); normalised values against the
    exact statistics within the bound those errors imply.

Arrays are time-major: x [K*T, E] or [K*T, E, C], done / valid [K*T, E]; K = number of segments (consecutive rollouts).
"""
import math

import numpy as np

U64 = 2.0 ** -53


def unit_roundoff(real):
    return 2.0 ** -24 if np.dtype(real) == np.float32 else U64


def _split(x, done, valid, segments):
    """-> x [K, T, E, C], done [K, T, E] bool, valid [K, T, E] bool or None, and the caller's shape."""
    shape = x.shape
    K = int(segments)
    if shape[0] % K:
        raise ValueError("segments must divide the ticks")
    T, E = shape[0] // K, shape[1]
    C = 1 if x.ndim == 2 else shape[2]
    x4 = x.reshape(K, T, E, C)
    d3 = np.asarray(done).reshape(K, T, E) != 0
    v3 = None if valid is None else np.asarray(valid).reshape(K, T, E) != 0
    return x4, d3, v3, shape


# ---------------------------------------------------------------- (a) working precision ----------------------------------------

def returns_working(x, done, gamma, real, valid=None, segments=1, masked=True):
    """The kernels' returns in `real`, bit for bit.  masked=False keeps the recurrence's values at invalid entries (the bound
    of layer (b) needs them)."""
    real = np.dtype(real).type
    x4, d3, v3, shape = _split(np.asarray(x).astype(real), done, valid, segments)
    K, T, E, C = x4.shape
    g_r = real(gamma)
    zero = real(0)
    out = np.empty_like(x4)
    g = np.zeros((K, E, C), real)
    for t in range(T - 1, -1, -1):
        g = x4[:, t] + np.where(d3[:, t, :, None], zero, g_r * g)
        out[:, t] = g
    if masked and v3 is not None:
        out = np.where(v3[..., None], out, zero)
    return out.reshape(shape)


def stats_from_moments(tot):
    """(mean, sd, count) from the float64 (sum, sum of squares, count), with the kernels' expressions."""
    s, s2, n = float(tot[0]), float(tot[1]), float(tot[2])
    cnt = n if n > 1.0 else 1.0
    mean = s / cnt
    var = s2 / cnt - mean * mean
    var = var if var > 0.0 else 0.0
    return mean, math.sqrt(var), n


def fold_parts(parts, seg=0):
    """Rank-ordered sum of the [ranks][K][3] triples of segment `seg` (k_normalize's fold)."""
    p = np.asarray(parts, np.float64)
    tot = [float(v) for v in p[0, seg]]
    for r in range(1, p.shape[0]):
        tot = [tot[i] + float(p[r, seg, i]) for i in range(3)]
    return tot


def normalize_working(x, stats, eps, real, valid=None, segments=1):
    """(x - R(mean)) / R(sd + eps) in `real` per segment; stats [K][3] = (mean, sd, count); invalid entries -> +0."""
    real = np.dtype(real).type
    x4, _, v3, shape = _split(np.asarray(x).astype(real), np.zeros(x.shape[:2], np.uint8), valid, segments)
    st = np.asarray(stats, np.float64).reshape(-1, 3)
    out = np.empty_like(x4)
    for k in range(x4.shape[0]):
        m = real(st[k, 0])
        den = real(float(st[k, 1]) + eps)
        out[k] = (x4[k] - m) / den
    if v3 is not None:
        out = np.where(v3[..., None], out, real(0))
    return out.reshape(shape)


# ---------------------------------------------------------------- (b) exact / float64 reference ----------------------------------

def returns_exact(x, done, gamma, segments=1):
    """Float64 returns with the unrounded gamma (unmasked)."""
    return returns_working(np.asarray(x, np.float64), done, float(gamma), np.float64, None, segments)


def returns_bound(g_work, g_ref, done, gamma, real, segments=1):
    """Elementwise bound on |G_kernel - G_exact| (real numbers, not just the float64 reference), from the kernel's unmasked
    values g_work (= returns_working(..., masked=False), which layer (a) pins bit for bit) and the float64 reference g_ref:
        b[t] = nd * (gamma b[t+1] + |R(gamma) - gamma| |G^[t+1]| + u_R |R(gamma) G^[t+1]| + u64 |gamma G64[t+1]|)
               + u_R |G^[t]| + u64 |G64[t]|
    (the kernel's product and sum, the float32 gamma's systematic term, and the reference's own two roundings)."""
    real = np.dtype(real).type
    u = unit_roundoff(real)
    gk, d3, _, shape = _split(np.asarray(g_work, np.float64), done, None, segments)
    gr = np.asarray(g_ref, np.float64).reshape(gk.shape)
    K, T, E, C = gk.shape
    g_r = float(real(gamma))
    dg = abs(g_r - float(gamma))
    b = np.empty_like(gk)
    prev = np.zeros((K, E, C))
    for t in range(T - 1, -1, -1):
        nd = ~d3[:, t, :, None]
        if t + 1 < T:
            carry = dg * np.abs(gk[:, t + 1]) + u * np.abs(g_r * gk[:, t + 1]) + U64 * np.abs(gamma * gr[:, t + 1])
            step = np.where(nd, abs(gamma) * prev + carry, 0.0)
        else:
            step = np.zeros_like(prev)
        prev = step + u * np.abs(gk[:, t]) + U64 * np.abs(gr[:, t])
        b[:, t] = prev
    return (b * (1.0 + 1e-6)).reshape(shape)


def masked_values(g, valid=None, segments=1):
    """Per segment: the float64 values of the valid entries, in memory order."""
    x4, _, v3, _ = _split(np.asarray(g, np.float64), np.zeros(np.asarray(g).shape[:2], np.uint8), valid, segments)
    out = []
    for k in range(x4.shape[0]):
        vals = x4[k]
        if v3 is not None:
            vals = vals[np.broadcast_to(v3[k][..., None], vals.shape)]
        out.append(vals.ravel())
    return out


def moments_exact(g, valid=None, segments=1):
    """Per segment: dict(s, s2, n, abs_s, abs_s2, vals) -- math.fsum (correctly rounded) over the given returns' valid entries;
    the squares are the float64 products the kernels form."""
    out = []
    for v in masked_values(g, valid, segments):
        sq = v * v
        out.append(dict(s=math.fsum(v), s2=math.fsum(sq), n=float(v.size), abs_s=math.fsum(np.abs(v)), abs_s2=math.fsum(sq),
                        vals=v))
    return out


def moments_bound(m, terms=None):
    """|S_kernel - S_exact|, |S2_kernel - S2_exact| for a recursive / tree sum of `terms` (default: n) float64 summands (the
    fsum reference itself is within u64 |S| of the exact sum)."""
    n = m["n"] if terms is None else terms
    k = max(n - 1.0, 0.0) * U64 * (1.0 + 1e-6)
    return k * m["abs_s"] + U64 * abs(m["s"]), k * m["abs_s2"] + U64 * abs(m["s2"])


def stats_exact(vals):
    """Two-pass (mean, sd) of the valid returns (math.fsum both passes; sd = 0 for an empty selection)."""
    n = vals.size
    if n == 0:
        return 0.0, 0.0
    mean = math.fsum(vals) / n
    var = math.fsum((vals - mean) ** 2) / n
    return mean, math.sqrt(var)


def stats_bound(mom_k, stats_k, ds, ds2, mean_x, sd_x):
    """Bounds on |mean_k - mean_x| and |sd_k - sd_x| for the one-pass mean = S / n, var = S2 / n - mean^2, sd = sqrt(var) in
    float64 from the kernel's moments mom_k = (S, S2, n) and statistics stats_k = (mean, sd), given the sums' errors ds / ds2
    (moments_bound) and the exact two-pass values (whose own float64 rounding is included).  The mean^2 terms make the sd bound grow with mean^2 / var."""
    u = U64
    mean_k, sd_k = float(stats_k[0]), float(stats_k[1])
    cnt = max(float(mom_k[2]), 1.0)
    dmean = ds / cnt + u * abs(mean_k) + 2 * u * abs(mean_x)
    dq = ds2 / cnt + u * abs(float(mom_k[1]) / cnt)
    dp = dmean * (2 * abs(mean_k) + dmean) + u * mean_k * mean_k
    dvar = (dq + dp + u * sd_k * sd_k + 4 * u * sd_x * sd_x) * (1 + 1e-6)
    dsd = min(math.sqrt(dvar), dvar / (sd_k + sd_x) if sd_k + sd_x > 0 else math.inf) + 2 * u * sd_k + 4 * u * sd_x
    return dmean * (1 + 1e-6), dsd * (1 + 1e-6)


def normalized_bound(g, y_exact, mean_k, sd_k, eps, real, dmean, dsd, mean_x, sd_x):
    """Elementwise bound on |y_kernel - (g - mean_x) / (sd_x + eps)| for y_kernel = (g - R(mean_k)) / R(sd_k + eps) in R."""
    real = np.dtype(real).type
    u = unit_roundoff(real)
    m_r = float(real(mean_k))
    den_r = float(real(sd_k + eps))
    d_exact = sd_x + eps
    dm = u * abs(m_r) + dmean
    num = np.abs(np.asarray(g, np.float64) - m_r)
    dnum = dm + u * num
    dden = u * den_r + U64 * (sd_k + eps) + dsd
    lo = min(den_r, d_exact)
    if lo <= 0:
        return np.full(np.shape(g), np.inf)
    ay = np.abs(y_exact)
    b = dnum / lo + ay * dden / lo + u * (ay + dnum / lo + ay * dden / lo) + 3 * U64 * ay
    return b * (1.0 + 1e-3) + 1e-300


def parts_from_shards(shard_moments):
    """[ranks][K][3] float64 parts (what one all-gather of every rank's moments[K][3] delivers) from per-rank, per-segment
    (sum, sum of squares, count) triples: shard_moments[r][k] = (s, s2, n)."""
    p = np.asarray(shard_moments, np.float64)
    if p.ndim != 3 or p.shape[2] != 3:
        raise ValueError("shard moments must be [ranks][K][3]")
    return np.ascontiguousarray(p)


def shard_moments(g, valid, segments, n_ranks):
    """Exact (fsum) moments of each rank's share of every segment -- the envs split into n_ranks contiguous blocks, as
    cm3_amd.shard.shard_range does -- -> ([ranks][K][3] parts, per-part abs sums [ranks][K][2])."""
    x4, _, v3, _ = _split(np.asarray(g, np.float64), np.zeros(np.asarray(g).shape[:2], np.uint8), valid, segments)
    K, T, E, C = x4.shape
    q, rem = divmod(E, n_ranks)
    parts = np.zeros((n_ranks, K, 3))
    abs_ = np.zeros((n_ranks, K, 2))
    for r in range(n_ranks):
        base = r * q + min(r, rem)
        cnt = q + (1 if r < rem else 0)
        for k in range(K):
            v = x4[k, :, base:base + cnt]
            if v3 is not None:
                v = v[np.broadcast_to(v3[k, :, base:base + cnt, None], v.shape)]
            v = v.ravel()
            parts[r, k] = (math.fsum(v), math.fsum(v * v), float(v.size))
            abs_[r, k] = (math.fsum(np.abs(v)), math.fsum(v * v))
    return parts_from_shards(parts), abs_
