"""The float64 definition of the leave-one-out predictive report (csrc/loopred.hip, include/autoreparam.h:
arp_loo_predictive; diagnostics.loo_predictive_summary), numpy / scipy only, nothing fitted to the device:

  * the six per-observation columns {sum W, sum W^2, sum W mu, sum W (mu^2 + var), sum W pit, draws counted} from an
    observation table, centred draws and log weights, over the draws with lw != -inf, W = exp(lw); mu, mu^2 + var and pit
    per (observation, draw) are tests/ppc_ref.py's;
  * the summary formulas, written out here independently of diagnostics.py (Vehtari, Gelman, Gabry 2017 section 2);
  * the Pareto-smoothed log weights of tests/psis_ref.py: psis_row IN DRAW ORDER, as include/autoreparam.h states them
    for arp_psis_weights: the draw at position i < M of the stable ascending-ll order takes the (M - 1 - i)-th smallest
    smoothed tail weight, every other kept draw its raw weight llmin - ll."""
import collections
import math

import numpy as np

import ppc_ref as pp
import psis_ref as pr

NORMAL, BERNOULLI = pp.NORMAL, pp.BERNOULLI
COLUMNS = ("sum_w", "sum_w_sq", "sum_w_mu", "sum_w_second_moment", "sum_w_pit", "draws_counted")
# what `columns` returns: sums [n, 6]; absw [n, 5] = sum W |h| of the five float columns (h = 1, W, mu, m2, pit) and
# terms [n] = the draws counted, for the float64 part of an allowance; r: ppc_ref's Ref of the same (n, r), for the
# float32 part (its eta, s, A, mu, m2, pit, p)
Columns = collections.namedtuple("Columns", ["sums", "absw", "terms", "W", "r"])


def columns(table, x, lw, n0=0, n1=None):
    """The six columns of the observations [n0, n1) from x [R, D] (float32 values) and lw [n1 - n0, R] float64 -> Columns.
    A draw with lw = -inf enters nothing, whatever its state holds; a NaN lw enters and carries through."""
    N = table.idx.shape[0]
    n1 = N if n1 is None else n1
    lw = np.asarray(lw, np.float64)
    r = pp.reference(table, x, n0, n1)
    inside = lw != -np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        W = np.where(inside, np.exp(np.where(inside, lw, 0.0)), 0.0)
        h = (np.ones_like(W), W, r.mu, r.m2, r.pit)
        sums = np.stack([np.where(inside, W * v, 0.0).sum(1) for v in h] + [inside.sum(1).astype(np.float64)], axis=1)
        absw = np.stack([np.where(inside, W * np.abs(v), 0.0).sum(1) for v in h], axis=1)
    return Columns(sums, absw, inside.sum(1).astype(np.float64), W, r)


def summary(sums, y, kind):
    """The report from the [N, 6] columns, as a dict: per observation loo_mean, loo_sd, loo_pit, is_ess; counted / left_out;
    Normal: pit_ks, coverage_90, rmse, r2; Bernoulli: brier, accuracy, balanced_accuracy; both: is_ess_min and its
    observation.  None where the figure is not defined."""
    s = np.asarray(sums, np.float64).reshape(-1, 6)
    y = np.asarray(y, np.float64).reshape(-1)
    N = y.size
    mean, sd, pit, ess = (np.full(N, np.nan) for _ in range(4))
    with np.errstate(all="ignore"):                            # (numpy scalars: IEEE division, 0 / 0 = NaN, no exception)
        for n in range(N):
            s0, s1, s2, s3, s4 = s[n, :5]
            mean[n] = s2 / s0
            v = s3 / s0 - mean[n] * mean[n]
            sd[n] = math.sqrt(v) if v > 0.0 else (0.0 if v <= 0.0 else float("nan"))
            pit[n] = s4 / s0
            ess[n] = s0 * s0 / s1
    ok = [n for n in range(N) if all(math.isfinite(a[n]) for a in (mean, sd, pit, ess))]
    out = {"loo_mean": mean, "loo_sd": sd, "loo_pit": pit, "is_ess": ess, "observations": len(ok), "left_out": N - len(ok)}
    for name in ("pit_ks", "coverage_90", "rmse", "r2", "brier", "accuracy", "balanced_accuracy", "is_ess_min"):
        out[name] = None
    out["is_ess_min_observation"] = -1
    if not ok:
        return out
    at = min(ok, key=lambda n: (ess[n], n))
    out["is_ess_min"], out["is_ess_min_observation"] = float(ess[at]), at
    err2 = [(y[n] - mean[n]) ** 2 for n in ok]
    if kind == NORMAL:
        u = sorted(pit[n] for n in ok)
        m = len(u)
        out["pit_ks"] = max(max((i + 1.0) / m - u[i] for i in range(m)), max(u[i] - float(i) / m for i in range(m)))
        out["coverage_90"] = sum(1 for n in ok if 0.05 <= pit[n] <= 0.95) / float(m)
        out["rmse"] = math.sqrt(math.fsum(err2) / m)
        ybar = math.fsum(y[n] for n in ok) / m
        total = math.fsum((y[n] - ybar) ** 2 for n in ok)
        out["r2"] = 1.0 - math.fsum(err2) / total if m >= 2 and total > 0.0 else None
    else:
        out["brier"] = math.fsum(err2) / len(ok)
        hit = {n: (mean[n] > 0.5) == (y[n] > 0.5) for n in ok}
        out["accuracy"] = sum(hit.values()) / float(len(ok))
        pos, neg = [n for n in ok if y[n] > 0.5], [n for n in ok if not y[n] > 0.5]
        if pos and neg:
            out["balanced_accuracy"] = 0.5 * (sum(hit[n] for n in pos) / float(len(pos)) + sum(hit[n] for n in neg) / float(len(neg)))
    return out


def psis_log_weights_row(ll):
    """lw [R'] float64 of one observation's kept draws `ll`, in draw order: psis_ref.psis_row's `lws`, put back where the
    draws are.  A row with a non-finite ll is NaN throughout; a row that is not fitted keeps its raw weights."""
    ll = np.asarray(ll, np.float64).reshape(-1)
    R = ll.size
    if R == 0:
        return np.zeros(0)
    if not np.all(np.isfinite(ll)):
        return np.full(R, np.nan)
    M = pr.tail_len(R)
    order = np.argsort(ll, kind="stable")                  # ascending ll; ties in ascending draw index
    s = ll[order]
    lws = -s - np.max(-s)                                  # raw: llmin - ll, descending from 0
    cutoff = float(lws[M])
    if M >= 5:
        x = (np.exp(lws[:M]) - math.exp(cutoff))[::-1]
        k, sigma = pr.gpdfit(x)
        if np.isfinite(k) and np.isfinite(sigma):
            p = (np.arange(1, M + 1, dtype=np.float64) - 0.5) / M
            q = -sigma * np.log1p(-p) if k == 0.0 else sigma * np.expm1(-k * np.log1p(-p)) / k
            with np.errstate(all="ignore"):
                sm = np.minimum(np.log(math.exp(cutoff) + q), 0.0)       # ascending: the j-th smallest smoothed tail weight
            lws[:M] = sm[::-1]                                           # position i takes the (M - 1 - i)-th smallest
    out = np.empty(R)
    out[order] = lws
    return out


def psis_log_weights(ll, mask=None):
    """lw [N, R] float64 of ll [N, R]: -inf where mask [R] != 0, psis_log_weights_row over the other draws."""
    ll = np.asarray(ll)
    keep = np.ones(ll.shape[1], bool) if mask is None else (np.asarray(mask).reshape(-1) == 0)
    out = np.full(ll.shape, -np.inf, np.float64)
    for n in range(ll.shape[0]):
        out[n, keep] = psis_log_weights_row(ll[n, keep])
    return out


def loglik(table, x, n0=0, n1=None):
    """ll [n1 - n0, R] in float64 from the table and centred states x [R, D]: the definition arp_pointwise_loglik follows."""
    N = table.idx.shape[0]
    n1 = N if n1 is None else n1
    sub = type(table)(table.kind, table.idx[n0:n1], table.w[n0:n1], table.y[n0:n1], table.scale_idx[n0:n1], table.log_scale[n0:n1])
    eta, s, _ = pp.predictor(sub, np.asarray(x, np.float64))
    y = sub.y.astype(np.float64)[:, None]
    if table.kind == NORMAL:
        return -0.5 * ((y - eta) * np.exp(-s)) ** 2 - s - 0.5 * pp.LOG_2PI
    return y * eta - pp.softplus(eta)
