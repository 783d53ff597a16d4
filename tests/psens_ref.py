"""Float64 numpy restatement of power-scaling sensitivity as include/autoreparam.h (arp_element_order, arp_cjs_sums,
arp_loglik_total) and diagnostics.psens_summary define it: a stable argsort on the uint32 key, the weighted ECDF from a
longdouble cumulative sum, every sum by math.fsum, and the summary.  Test infrastructure: nothing here imports the package."""
import math

import numpy as np

DELTA = 0.01
THRESHOLD = 0.05
LN2 = math.log(2.0)


def key_of(x):
    """The order-preserving uint32 key of float32 values: negative values bit-inverted, the others with the sign bit set;
    -0 is +0."""
    x = np.ascontiguousarray(x, np.float32)
    u = np.where(x == 0, np.uint32(0), x.view(np.uint32)).astype(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def value_of(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def element_order(x):
    """(order [D, N] uint32, sorted [D, N] float32) of pooled draws x [N, D] float32 (row r = s C + c)."""
    key = key_of(x).T                                                    # [D, N]
    order = np.argsort(key, axis=1, kind="stable").astype(np.uint32)
    return order, value_of(np.take_along_axis(key, order.astype(np.int64), axis=1))


def _log2_or_zero(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(v == 0, 0.0, np.log2(np.where(v == 0, 1.0, v)))


def cjs_row(xs, order, lw, shift=0.0):
    """(sums [8], magnitude [8]) of one (row, element): xs [N] the sorted values, order [N] their draw indices, lw [N] the
    log weights by draw.  magnitude: per column, the sum of absolute terms that the header's bound multiplies (0 for the
    exact count)."""
    lws = np.asarray(lw, np.float64)[np.asarray(order, np.int64)]
    kept = ~np.isneginf(lws)
    x = np.asarray(xs, np.float64)[kept]
    W = np.exp(lws[kept])
    n = int(x.size)
    u = x - float(shift)
    S = math.fsum(W)
    sums = [float(n), S, math.fsum(W * u), math.fsum(W * u * u)]
    mag = [0.0, S, math.fsum(np.abs(W * u)), sums[3]]
    if n < 2:
        return np.array(sums + [0.0] * 4), np.array(mag + [0.0] * 4)
    with np.errstate(divide="ignore", invalid="ignore"):
        P = (np.arange(1, n + 1, dtype=np.float64) / float(n))[:-1]
        Q = np.asarray(np.cumsum(W.astype(np.longdouble)) / np.longdouble(S), np.float64)[:-1]
        M = 0.5 * (P + Q)
        b = np.diff(x)
        lp, lq, lm = _log2_or_zero(P), _log2_or_zero(Q), _log2_or_zero(M)
        i_p, i_q = math.fsum(b * P), math.fsum(b * Q)
        sums += [math.fsum(b * P * (lp - lm)), math.fsum(b * Q * (lq - lm)), i_p, i_q]
        a_mag = math.fsum(b * (np.abs(P * lp) + np.abs(Q * lq) + (P + Q) * np.abs(lm))) + 2.0 * (i_p + i_q) / LN2
    return np.array(sums), np.array(mag + [a_mag, a_mag, i_p, 2.0 * i_q])


def cjs_sums(values, order, lw, shift=None):
    """(out [K, D, 8], magnitude [K, D, 8]) for values, order [D, N] and lw [K, N]."""
    values, order, lw = np.asarray(values), np.asarray(order), np.atleast_2d(np.asarray(lw, np.float64))
    D, K = values.shape[0], lw.shape[0]
    out, mag = np.zeros((K, D, 8)), np.zeros((K, D, 8))
    for k in range(K):
        for d in range(D):
            out[k, d], mag[k, d] = cjs_row(values[d], order[d], lw[k], 0.0 if shift is None else float(shift[d]))
    return out, mag


def bound(N, magnitude):
    """The header's first-order bound of the float columns: (ceil(N / 256) + 64) 2^-52 times the magnitude."""
    return (math.ceil(N / 256.0) + 64.0) * 2.0 ** -52 * np.asarray(magnitude, np.float64)


def distance(row):
    """The cumulative Jensen-Shannon distance of one [8] row of sums; NaN for a constant element."""
    a_pq, a_qp, i_p, i_q = (float(v) for v in row[4:8])
    pq = max(0.0, a_pq + (i_q - i_p) / (2.0 * LN2))
    qp = max(0.0, a_qp + (i_p - i_q) / (2.0 * LN2))
    if math.isnan(a_pq) or math.isnan(a_qp) or not i_p + i_q > 0:
        return float("nan")
    return math.sqrt((pq + qp) / (i_p + i_q))


def moments(row):
    """(weighted mean of u, weighted sd) of one [8] row."""
    if not row[1] > 0:
        return float("nan"), float("nan")
    m = row[2] / row[1]
    return m, math.sqrt(max(row[3] / row[1] - m * m, 0.0))


def summary(sums):
    """The report from sums [5, D, 8] (prior lower, prior upper, likelihood lower, likelihood upper, unweighted): a dict of
    [D] arrays prior, likelihood, mean_shift_prior, mean_shift_likelihood, sd_ratio_prior, sd_ratio_likelihood, the lists
    conflict and weak_likelihood, and constant, the number of elements without a distance."""
    s = np.asarray(sums, np.float64)
    D = s.shape[1]
    out = {k: np.full(D, np.nan) for k in ("prior", "likelihood", "mean_shift_prior", "mean_shift_likelihood",
                                           "sd_ratio_prior", "sd_ratio_likelihood")}
    scale = 2.0 * math.log2(1.0 + DELTA)
    for d in range(D):
        out["prior"][d] = (distance(s[0, d]) + distance(s[1, d])) / scale
        out["likelihood"][d] = (distance(s[2, d]) + distance(s[3, d])) / scale
        m0, sd0 = moments(s[4, d])
        for name, k in (("prior", 1), ("likelihood", 3)):
            m, sd = moments(s[k, d])
            if sd0 > 0:
                out["mean_shift_" + name][d] = (m - m0) / sd0
                out["sd_ratio_" + name][d] = sd / sd0
    p, l = out["prior"], out["likelihood"]
    out["conflict"] = [d for d in range(D) if p[d] > THRESHOLD and l[d] > THRESHOLD]
    out["weak_likelihood"] = [d for d in range(D) if p[d] > THRESHOLD and not l[d] > THRESHOLD]
    out["constant"] = int(sum(1 for d in range(D) if math.isnan(p[d]) or math.isnan(l[d])))
    return out
