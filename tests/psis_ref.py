"""Float64 definition of the PSIS-LOO / WAIC columns `arp_psis_loo` (csrc/psis.hip) writes, numpy and
scipy.special.logsumexp only, written from the papers: Vehtari, Gelman, Gabry 2017 (PSIS-LOO, WAIC), Vehtari, Simpson,
Gelman, Yao, Gabry 2024 (Pareto smoothing, the tail length, the k-hat threshold), Zhang & Stephens 2009 (the profile
estimate of the generalised Pareto distribution, with the weakly informative prior on k that loo::gpdfit and ArviZ add).

One observation at a time over its R' kept draws (float32 log-likelihoods taken to float64 before anything else):

  columns = {elpd_loo, pareto_k, lppd, p_waic, tail_len, cutoff, gpd_sigma, draws_used}

A row with a non-finite log-likelihood among its kept draws is not fitted: elpd_loo = NaN for a NaN input, -inf otherwise,
pareto_k = +inf, lppd = p_waic = cutoff = gpd_sigma = NaN; tail_len and draws_used are still the row's.  A row without a
kept draw gives NaN, k = +inf and zeros in the two counts."""
import math

import numpy as np
from scipy.special import logsumexp

COLUMNS = ("elpd_loo", "pareto_k", "lppd", "p_waic", "tail_len", "cutoff", "gpd_sigma", "draws_used")
R_MAX = 1 << 24


def tail_len(R):
    """min(floor(R / 5), m), m the smallest integer with m^2 >= 9 R (= ceil(3 sqrt(R)) without a square root)."""
    R = int(R)
    m = math.isqrt(9 * R)
    if m * m < 9 * R:
        m += 1
    return min(R // 5, m)


def gpdfit(x):
    """(k, sigma) of the generalised Pareto distribution fitted to the ascending exceedances x [M] (Zhang & Stephens 2009,
    with the prior of loo::gpdfit: k <- (M k + 5) / (M + 10)).  Degenerate input ends in non-finite values, not an error."""
    x = np.asarray(x, np.float64)
    M = x.size
    m_grid = 30 + int(math.floor(math.sqrt(M)))
    with np.errstate(all="ignore"):
        xq = x[int(math.floor(M / 4.0 + 0.5)) - 1]
        i = np.arange(1, m_grid + 1, dtype=np.float64)
        b = 1.0 / x[M - 1] + (1.0 - np.sqrt(m_grid / (i - 0.5))) / (3.0 * xq)
        k = np.mean(np.log1p(-b[:, None] * x[None, :]), axis=1)
        L = M * (np.log(-b / k) - k - 1.0)
        w = 1.0 / np.sum(np.exp(L[None, :] - L[:, None]), axis=1)
        w = w / np.sum(w)
        bb = np.sum(b * w)
        kk = np.mean(np.log1p(-bb * x))
        sigma = -kk / bb
        kk = (M * kk + 5.0) / (M + 10.0)
    return float(kk), float(sigma)


def psis_row(ll):
    """The eight columns of one observation from its kept draws `ll` (any float array; float64 from here on)."""
    ll = np.asarray(ll, np.float64).reshape(-1)
    R = ll.size
    nan, inf = float("nan"), float("inf")
    if R == 0:
        return np.array([nan, inf, nan, nan, 0.0, nan, nan, 0.0])
    M = tail_len(R)
    if not np.all(np.isfinite(ll)):
        return np.array([nan if np.any(np.isnan(ll)) else -inf, inf, nan, nan, float(M), nan, nan, float(R)])
    lppd = float(logsumexp(ll) - math.log(R))
    p_waic = float(np.var(ll, ddof=1)) if R > 1 else nan
    order = np.argsort(ll, kind="stable")          # ascending ll = descending importance ratio: the tail comes first
    s = ll[order]
    lw = -s - np.max(-s)                           # log ratios shifted by their maximum: lw[0] = 0, descending
    cutoff = float(lw[M])                          # the largest value not in the tail (M <= R / 5 < R)
    k, sigma = inf, nan
    lws = lw.copy()
    if M >= 5:
        x = (np.exp(lw[:M]) - math.exp(cutoff))[::-1]           # ascending exceedances
        k, sigma = gpdfit(x)
        if not (np.isfinite(k) and np.isfinite(sigma)):
            k, sigma = inf, nan
        else:
            p = (np.arange(1, M + 1, dtype=np.float64) - 0.5) / M
            if k == 0.0:
                q = -sigma * np.log1p(-p)
            else:
                q = sigma * np.expm1(-k * np.log1p(-p)) / k
            with np.errstate(all="ignore"):
                sm = np.minimum(np.log(math.exp(cutoff) + q), 0.0)           # j-th smallest tail weight, ascending
            lws[:M] = sm[::-1]
    elpd = float(logsumexp(lws + s) - logsumexp(lws))
    return np.array([elpd, k, lppd, p_waic, float(M), cutoff, sigma, float(R)])


def psis_loo(ll, mask=None):
    """out [N, 8] float64 of ll [N, R] (float32 or float64) with the draws where mask [R] != 0 left out."""
    ll = np.asarray(ll)
    keep = np.ones(ll.shape[1], bool) if mask is None else (np.asarray(mask).reshape(-1) == 0)
    return np.stack([psis_row(row[keep]) for row in ll]) if ll.shape[0] else np.zeros((0, 8))


# ---- the host formulas of the report (diagnostics.loo_summary / loo_compare / pareto_k_threshold) ----
def summary(elpd_loo_i, lppd_i, p_waic_i):
    e, l, p = (np.asarray(v, np.float64) for v in (elpd_loo_i, lppd_i, p_waic_i))
    N = e.size
    w = l - p
    se = lambda v: float(math.sqrt(N * np.var(v, ddof=1))) if N > 1 else float("nan")
    return {"elpd_loo": float(e.sum()), "elpd_loo_se": se(e), "p_loo": float((l - e).sum()),
            "elpd_waic": float(w.sum()), "elpd_waic_se": se(w), "p_waic": float(p.sum())}


def compare(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    N = d.size
    return float(d.sum()), (float(math.sqrt(N * np.var(d, ddof=1))) if N > 1 else float("nan"))


def k_threshold(R):
    return min(1.0 - 1.0 / math.log10(R), 0.7) if R > 1 else float("nan")
