"""Numpy restatement of the policy normaliser (tsidb_policy_norm_update, the map of tsidb_policy_actor_norm), written from their
description in include/tsidb.h: the batch mean and biased variance of each column in float64 - two passes per segment of
SEG_ROWS rows, the segments merged in their order by Chan's formula - rsl_rl's running update, the float32 affine pair and the
float32 map with its clamp.  No torch, no library.

Beside the values it carries the EXACT result (rational arithmetic, rounded once) and a worst-case FORWARD ERROR BOUND for any
float64 evaluation of it, derived here and computed in float64.  u = 2^-53, g(k) = k u / (1 - k u).  Per column, for N rows
in S segments (S = 1: one plain sum), with A = max |x|, m the exact batch mean, R = max |x - m|:

    a mean of n <= N values, any order    |err| <= g(n + 1) A              (n - 1 additions, the division, one to spare)
    one Chan merge of two means           mean_a + (mean_b - mean_a) w, 0 < w <= 1: the inputs' errors enter as a convex
                                          combination (<= their maximum); the difference, w, the product and the sum round
                                          once each on magnitudes <= 2 A, 2 A, 2 A, A: + 7 u A per merge
    =>  B_mb  = g(N + 1 + 7 S) A                                            (every partial mean too)
    a deviation from any computed partial mean is at most D = 2 R + B_mb    (|x - m_s| <= |x - m| + |m - m_s| <= 2 R)
    the centred squares of a segment      sum (x - m^)^2 = sum (x - m_s)^2 + n_s (m^ - m_s)^2 exactly (the cross term vanishes);
                                          the difference, the square (2 roundings) and the n_s - 1 additions: relative
                                          g(n_s + 2) on a sum of non-negative terms <= n_s D^2
    =>  per row of the segment            g(N + 2) D^2 + B_mb^2
    the merge's d^2 n_a n_s / (n_a + n_s) d carries e_d = 2 B_mb + 2 u D, the products and the quotient 6 roundings; the weights
                                          n_a n_s / (n_a + n_s) <= n_s sum to <= N over the merges; two additions per merge
                                          on M2 <= N D^2
    =>  per row                           2 (2 D) e_d + e_d^2 + 6 u (2 D)^2 + 2 S u D^2
    var_b = M2 / N                        + u D^2
    =>  B_vb  = (g(N + 2) + (24 + 2 S + 1) u) D^2 + B_mb^2 + 4 D e_d + e_d^2

and for the running update from a given (mean, var, count), rate = N / count' <= 1, delta = mean_b - mean:
    e_delta = B_mb + u |delta|
    B_mean' = rate (e_delta + 3 u |delta|) + u |mean'|                      (rate, the product, the sum; fused or not)
    q = mean_b - mean':  e_q = B_mb + B_mean' + u |q|
    p = delta q:         e_p = |delta| e_q + |q| e_delta + e_delta e_q + u |delta q|
    inner = var_b - var + p:  e_i = B_vb + e_p + 2 u (|var_b| + |var| + |p|)
    B_var'  = rate (e_i + 2 u |inner|) + u |var'|
Each bound finally takes u |exact| more for the one rounding of the exact value itself.
tests/test_policy_norm_reference.py shows that float64 evaluations in several orders stay inside it."""
from fractions import Fraction

import numpy as np

U64 = 2.0 ** -53
SEG_ROWS = 256
EPS = 1e-2


def g(k):
    return k * U64 / (1.0 - k * U64)


def seen(block):
    """the values the device works on: float64 of the float32 cast of the block"""
    return np.asarray(block).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------- the batch statistics in float64
def _two_pass(x):
    """(mean, M2) of the rows of x, each a plain left-to-right sum in float64"""
    n = x.shape[0]
    s = np.zeros(x.shape[1])
    for row in x:
        s = s + row
    m = s / n
    q = np.zeros(x.shape[1])
    for row in x:
        d = row - m
        q = q + d * d
    return m, q


def batch_stats(x, order="segments", seg=SEG_ROWS):
    """(mean_b, var_b) [K] of the rows x [N, K] in float64; order: "sequential" / "reversed" - one two-pass sum over all rows,
    first to last / last to first - or "segments": two passes per segment of `seg` rows, merged in segment order by Chan"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    if order == "sequential":
        m, q = _two_pass(x)
        return m, q / n
    if order == "reversed":
        m, q = _two_pass(x[::-1])
        return m, q / n
    assert order == "segments"
    na, mean, m2 = 0.0, np.zeros(x.shape[1]), np.zeros(x.shape[1])
    for r0 in range(0, n, seg):
        ms, qs = _two_pass(x[r0:r0 + seg])
        ns = float(min(seg, n - r0))
        nab = na + ns
        d = ms - mean
        t = d * (ns / nab)
        mean = mean + t
        m2 = m2 + qs + d * t * na
        na = nab
    return mean, m2 / n


def running(mean_b, var_b, n, mean, var, count):
    """rsl_rl's EmpiricalNormalization.update, the five lines: (mean', var', count')"""
    count1 = count + n
    rate = n / count1
    delta = mean_b - mean
    mean1 = mean + rate * delta
    var1 = var + rate * (var_b - var + delta * (mean_b - mean1))
    return mean1, var1, count1


def update(x, mean, var, count, until=None, order="segments", seg=SEG_ROWS):
    """one tsidb_policy_norm_update on the rows x [N, K] (the values the device sees: seen(block)): (mean', var', count')"""
    if until is not None and count >= until:
        return np.array(mean, dtype=np.float64), np.array(var, dtype=np.float64), count
    mb, vb = batch_stats(x, order, seg)
    return running(mb, vb, x.shape[0], np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64), count)


def initial(K):
    return np.zeros(K), np.ones(K), 0


# ---------------------------------------------------------------------------- the float32 side
def affine32(mean, var, eps=EPS):
    """[2, K] float32: shift = (float)mean, scale = (float)(1 / (sqrt(var) + eps)), float64 until the cast"""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    return np.stack([mean.astype(np.float32), (1.0 / (np.sqrt(var) + eps)).astype(np.float32)])


def normalise32(block, affine, clip=None):
    """the rows the actor's layers see, float32: ((float)x - shift) * scale, one subtraction and one product, then the clamp"""
    x = np.asarray(block).astype(np.float32)
    a = np.asarray(affine, dtype=np.float32)
    v = ((x - a[0]).astype(np.float32) * a[1]).astype(np.float32)
    if clip is not None:
        c = np.float32(clip)
        v = np.minimum(np.maximum(v, -c), c)
    return v


# ---------------------------------------------------------------------------- the exact values and the bound
def exact_and_bound(x, mean, var, count, segments=None):
    """dict(mean_b, var_b, mean, var: the exact values rounded once to float64; b_mean_b, b_var_b, b_mean, b_var: the bound of a
    float64 evaluation in at most `segments` segments (None = ceil(N / SEG_ROWS)); count) for one update of (mean, var, count)
    [K] with the rows x [N, K]"""
    x = np.asarray(x, dtype=np.float64)
    n, K = x.shape
    S = segments if segments is not None else (n + SEG_ROWS - 1) // SEG_ROWS
    count1 = count + n
    rate_q = Fraction(n, count1)
    out = {k: np.zeros(K) for k in ("mean_b", "var_b", "mean", "var", "b_mean_b", "b_var_b", "b_mean", "b_var")}
    for c in range(K):
        col = [Fraction(float(v)) for v in x[:, c]]
        mb = sum(col) / n
        vb = sum(v * v for v in col) / n - mb * mb
        m0, v0 = Fraction(float(mean[c])), Fraction(float(var[c]))
        delta = mb - m0
        m1 = m0 + rate_q * delta
        q = mb - m1
        inner = vb - v0 + delta * q
        v1 = v0 + rate_q * inner
        A = float(np.abs(x[:, c]).max())
        R = float(max(abs(v - mb) for v in col))
        u, rate = U64, float(rate_q)
        b_mb = g(n + 1 + 7 * S) * A
        D = 2.0 * R + b_mb
        e_d = 2.0 * b_mb + 2.0 * u * D
        b_vb = (g(n + 2) + (25 + 2 * S) * u) * D * D + b_mb * b_mb + 4.0 * D * e_d + e_d * e_d
        ad, aq = abs(float(delta)), abs(float(q))
        e_delta = b_mb + u * ad
        b_m1 = rate * (e_delta + 3.0 * u * ad) + u * abs(float(m1))
        e_q = b_mb + b_m1 + u * aq
        e_p = ad * e_q + aq * e_delta + e_delta * e_q + u * ad * aq
        e_i = b_vb + e_p + 2.0 * u * (abs(float(vb)) + abs(float(v0)) + ad * aq)
        b_v1 = rate * (e_i + 2.0 * u * abs(float(inner))) + u * abs(float(v1))
        for k, val, b in (("mean_b", mb, b_mb), ("var_b", vb, b_vb), ("mean", m1, b_m1), ("var", v1, b_v1)):
            out[k][c] = float(val)
            out["b_" + k][c] = b + u * abs(float(val))
    out["count"] = count1
    return out


# ---------------------------------------------------------------------------- the cases the tests share
ENVS = (1, 17, 33, SEG_ROWS + 33)


def case_rows(n, K, seed):
    """[N, K] float64 rows of mixed scale, as a policy's input has them: column 0 with mean 1e3 and std 1e-2 (a one-pass sum of
    squares loses its variance), column 1 constant, then joint velocities of a few rad/s, unit vectors, and 0 - 1 cm heights"""
    rng = np.random.default_rng(seed)
    x = np.empty((n, K))
    x[:, 0] = 1e3 + 1e-2 * rng.standard_normal(n)
    x[:, 1] = 0.7
    for c in range(2, K):
        kind = c % 3
        x[:, c] = (rng.normal(0.3 * (c % 5), 4.0, n) if kind == 0 else rng.uniform(-1.0, 1.0, n) if kind == 1 else rng.uniform(0.0, 0.01, n))
    return x
