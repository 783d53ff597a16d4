"""float64 numpy restatement of nested R-hat (Margossian, Hoffman, Sountsov, Riou-Durand, Vehtari, Gelman 2024) -- TEST
YARDSTICK: written from the definition, shares no code with autoreparam_amd/diagnostics.py.

C = K M chains of N draws; superchain k owns chains k M ... k M + M - 1.  Per element: m_km, v_km the mean and unbiased
variance of a chain (v = 0 for N = 1), g_k = mean_m m_km, b_k = sum_m (m_km - g_k)^2 / (M - 1), w_k = mean_m v_km,
B = sum_k (g_k - gbar)^2 / (K - 1), W = mean_k (b_k + w_k), nested R-hat = sqrt(1 + B / W).  A superchain counts only if
all its chains have a finite mean and variance; NaN where W = 0 or fewer than two superchains count.
"""
import collections

import numpy as np

Nested = collections.namedtuple("Nested", ["rhat", "excess", "between", "within", "superchains", "left_out"])


def groups(mean, var, M):
    """(ok, g, b, w) [K, ...] of per-chain moments [C, ...]; var None: one draw per chain."""
    m = np.asarray(mean, np.float64)
    v = np.zeros_like(m) if var is None else np.asarray(var, np.float64)
    m, v = m.reshape((-1, M) + m.shape[1:]), v.reshape((-1, M) + v.shape[1:])
    ok = np.isfinite(m).all(axis=1) & np.isfinite(v).all(axis=1)
    with np.errstate(all="ignore"):
        g = m.mean(axis=1)
        return ok, g, ((m - g[:, None]) ** 2).sum(axis=1) / (M - 1), v.mean(axis=1)


def from_moments(mean, var, M):
    ok, g, b, w = groups(mean, var, M)
    k = ok.sum(axis=0).astype(np.float64)
    with np.errstate(all="ignore"):
        gbar = np.where(ok, g, 0.0).sum(axis=0) / k
        B = np.where(k >= 2, np.where(ok, (g - gbar) ** 2, 0.0).sum(axis=0) / (k - 1), np.nan)
        W = np.where(ok, b + w, 0.0).sum(axis=0) / k
        excess = np.where(W > 0, B / W, np.nan)
        return Nested(np.sqrt(1.0 + excess), excess, B, W, k, ok.shape[0] - k)


def chain_moments(trace):
    """(mean, var) [C, ...] of a [S, C, ...] trace; var None for S = 1."""
    x = np.asarray(trace, np.float64)
    with np.errstate(all="ignore"):
        return x.mean(axis=0), (x.var(axis=0, ddof=1) if x.shape[0] > 1 else None)


def nested(trace, M):
    """Nested of a [S, C, ...] trace over all S draws of every chain."""
    return from_moments(*chain_moments(trace), M)


def by_step(trace, M):
    """[S, ...]: nested R-hat of every row alone, one draw per chain."""
    return np.stack([from_moments(row, None, M).rhat for row in np.asarray(trace, np.float64)])


def sums(mean, var, M):
    """[6, ...]: superchains that count, sum g, sum g^2, sum b, sum w over them, superchains left out."""
    ok, g, b, w = groups(mean, var, M)
    z = lambda a: np.where(ok, a, 0.0).sum(axis=0)
    k = ok.sum(axis=0).astype(np.float64)
    return np.stack([k, z(g), z(g * g), z(b), z(w), ok.shape[0] - k])


def step_sums(trace, M):
    """[4, S, ...]: the first four of `sums` for every row alone."""
    return np.stack([sums(row, None, M)[:4] for row in np.asarray(trace, np.float64)], axis=1)
