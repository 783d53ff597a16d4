"""float64 numpy restatement of the potential scale reduction factor (Gelman-Rubin; the split form of BDA3 / Stan /
ArviZ, no rank normalisation) -- TEST YARDSTICK: written from the formulas, shares no code with
autoreparam_amd/diagnostics.py.

With m rows of n draws each:  W = mean over rows of the rows' variances (n - 1 divisor),  B/n = variance over rows of
the rows' means (m - 1 divisor),  var+ = (n-1)/n W + B/n,  rhat = sqrt(var+ / W),  pooled mean = mean of the row means,
pooled sd = sqrt(var+).  Split: every chain gives two rows, its first and its last n = S // 2 draws (an odd run drops
its middle draw).  A row enters only if its variance is finite; W = 0 or fewer than two rows give NaN.
"""
import numpy as np


def parts(trace, split):
    """[S, C, ...] -> the rows as [P, n, C, ...]: P = 2 halves of n = S // 2 draws, or P = 1 and n = S."""
    x = np.asarray(trace, np.float64)
    if not split:
        return x[None]
    h = x.shape[0] // 2
    return np.stack([x[:h], x[x.shape[0] - h:]])


def moments(trace, split):
    """(mean, var) [P, C, ...] of every row, float64; var = NaN for a row of one draw, both NaN for an empty one."""
    p = parts(trace, split)
    n = p.shape[1]
    with np.errstate(all="ignore"):
        mean = p.sum(axis=1) / n if n else np.full(p.shape[:1] + p.shape[2:], np.nan)
        var = ((p - mean[:, None]) ** 2).sum(axis=1) / (n - 1) if n > 1 else np.full_like(mean, np.nan)
    return mean, var


def rhat(trace, split=True):
    """(rhat, pooled mean, pooled sd, constant rows) per element [...], over the chain axis 1 of a [S, C, ...] trace."""
    mean, var = moments(trace, split)
    n = parts(trace, split).shape[1]
    mean, var = mean.reshape((-1,) + mean.shape[2:]), var.reshape((-1,) + var.shape[2:])      # rows: [P C, ...]
    ok = np.isfinite(var)
    m = ok.sum(axis=0).astype(np.float64)
    with np.errstate(all="ignore"):
        w = np.where(ok, var, 0.0).sum(axis=0) / m
        centre = np.where(ok, mean, 0.0).sum(axis=0) / m
        b_n = np.where(m >= 2, (np.where(ok, mean - centre, 0.0) ** 2).sum(axis=0) / (m - 1), np.nan)
        plus = (n - 1.0) / n * w + b_n if n else np.full_like(w, np.nan)
        return np.where(w > 0, np.sqrt(plus / w), np.nan), centre, np.sqrt(plus), (ok & (var == 0)).sum(axis=0)
