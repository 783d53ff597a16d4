"""Float64 numpy restatement of moment matching for importance sampling (Paananen, Piironen, Buerkner, Vehtari 2021,
"Implicitly adaptive importance sampling"; loo::loo_moment_match with the maps T1 and T2 and the split of section 4),
written from the paper and the project's issue text, one target at a time.  What it is held against:
diagnostics.moment_match and the two kernels of csrc/mmatch.hip.

The tail fits are tests/psis_ref.py's (through vicheck_ref.weights_row, which puts the smoothed weights back in the draws'
places).  The fit reads the NEGATED log ratio as float32 about its mean over the kept draws -- that is the interface of
arp_psis_weights, so it is part of the definition and restated here.  The affine map is restated in float32, operation
for operation; everything else is float64 (the moment sums in np.longdouble)."""
import collections

import numpy as np

import vicheck_ref as vr

MAX_ITERATIONS = 30
U53 = 2.0 ** -53

Result = collections.namedtuple("Result", ["attempted", "elpd", "pareto_k", "pareto_k_full", "pareto_k_split", "is_ess", "maps",
                                           "scale", "shift", "centre"])


def weighted_moments(x, lw, centre):
    """(out [B, 4 + 2 D], magnitude [B, 4 + 2 D]) float64: the row of arp_weighted_moments per target and, under every sum,
    the sum of its absolute terms (what the header's bound multiplies).  w = exp(lw - lw_max) in float64 -- the subtraction
    is part of the definition -- and the sums in np.longdouble."""
    x = np.asarray(x, np.float32)
    lw = np.asarray(lw, np.float64)
    R, D = x.shape
    e = x.astype(np.longdouble) - np.asarray(centre, np.float32).astype(np.longdouble)[None]
    out, mag = np.zeros((lw.shape[0], 4 + 2 * D)), np.zeros((lw.shape[0], 4 + 2 * D))
    for b, row in enumerate(lw):
        keep = ~np.isneginf(row)
        finite = row[keep & ~np.isnan(row)]
        top = finite.max() if finite.size else -np.inf
        out[b, 0], out[b, 3] = top, keep.sum()
        if not keep.any():
            continue
        with np.errstate(all="ignore"):
            w = np.exp(row[keep] - top).astype(np.longdouble)
        live = np.asarray(w != 0)                          # a weight that underflows enters nothing
        w, ek = w[live], e[keep][live]
        out[b, 1], out[b, 2] = w.sum(), (w * w).sum()
        mag[b, 1], mag[b, 2] = out[b, 1], out[b, 2]
        out[b, 4::2], out[b, 5::2] = (w[:, None] * ek).sum(axis=0), (w[:, None] * ek * ek).sum(axis=0)
        mag[b, 4::2], mag[b, 5::2] = (w[:, None] * np.abs(ek)).sum(axis=0), out[b, 5::2]
    return out, mag


def bound(kept, magnitude):
    """The header's first-order bound of a sum over `kept` draws whose absolute terms add up to `magnitude`."""
    return (kept + 32.0) * 2.0 * U53 * magnitude


def affine_rows(x, m, s, u, parity=-1):
    """out [B, R, D] float32: (x - m[b]) * s[b] + u[b] rounded after every operation, on every row (parity < 0) or on the
    rows with (r & 1) == parity; the others are x's, bit for bit."""
    x = np.asarray(x, np.float32)
    m, s, u = (np.asarray(v, np.float32) for v in (m, s, u))
    R = x.shape[0]
    pick = np.ones(R, bool) if parity < 0 else (np.arange(R) & 1) == parity
    out = np.repeat(x[None], m.shape[0], axis=0)
    with np.errstate(all="ignore"):
        a = (x[None, pick] - m[:, None]).astype(np.float32)
        p = (a * s[:, None]).astype(np.float32)
        out[:, pick] = (p + u[:, None]).astype(np.float32)
    return out


def smooth(rho, keep):
    """(k-hat, lw [R]) of the log ratios rho [R] float64: the fit of the negated ratio in float32 about its kept mean."""
    rho = np.asarray(rho, np.float64)
    with np.errstate(all="ignore"):
        centre = np.where(keep, rho, 0.0).sum() / max(int(keep.sum()), 1)
        ll = (-np.where(keep, rho - centre, 0.0)).astype(np.float32)
    out8, lw, _ = vr.weights_row(ll, (~keep).astype(np.uint8))
    return float(out8[1]), lw


def _moments(x, lw, m0_32):
    out, _ = weighted_moments(x, lw[None], m0_32)
    with np.errstate(all="ignore"):
        mean = out[0, 4::2] / out[0, 1]
        return mean, out[0, 5::2] / out[0, 1] - mean * mean


def log_sum(lw):
    """lw_max + log sum exp(lw - lw_max) over the draws with lw > -inf."""
    lw = lw[~np.isneginf(lw)]
    with np.errstate(all="ignore"):
        return lw.max() + np.log(np.exp(lw - lw.max()).sum()) if lw.size else -np.inf


def match_one(x, keep, L0, logp_fn, loglik, threshold, m0_32, base):
    """One target above the threshold -> (elpd, k, k_f, k_split, ess, maps, S, U); elpd None where no map was accepted."""
    D = x.shape[1]
    m0 = m0_32.astype(np.float64)
    l0 = np.asarray(loglik(x), np.float32)
    out8, lw, _ = vr.weights_row(l0, (~keep).astype(np.uint8))
    k, k_f, S, U, maps = float(out8[1]), 0.0, np.ones(D), m0.copy(), ""
    mean0, var0 = _moments(x, base, m0_32)
    m_of = lambda: np.repeat(m0_32[None], 1, axis=0)
    while (k > threshold or not np.isfinite(k)) and len(maps) < MAX_ITERATIONS:
        mean_w, var_w = _moments(x, lw, m0_32)
        with np.errstate(all="ignore"):
            mu_w, v_w, mu, v = mean_w * S + U, var_w * S * S, mean0 * S + U, var0 * S * S
            f = np.sqrt(v_w / v)
        moved = False
        for S_c, U_c, name in ((S, U + (mu_w - mu), "1"), (S * f, (U - mu) * f + mu_w, "2")):
            rows = affine_rows(x, m_of(), S_c[None], U_c[None])[0]
            with np.errstate(all="ignore"):
                rho_f = np.asarray(logp_fn(rows), np.float64) - L0
                k_c, lw_c = smooth(rho_f - np.asarray(loglik(rows), np.float64), keep)
            if k_c < k:
                k_f = smooth(rho_f, keep)[0]
                S, U, k, lw, maps, moved = S_c, U_c, k_c, lw_c, maps + name, True
                break
        if not moved:
            break
    if not maps:
        return None, k, k_f, np.nan, np.nan, maps, S, U
    A = affine_rows(x, m_of(), S[None], U[None], 0)[0]
    B = affine_rows(x, U[None], (1.0 / S)[None], m_of(), 1)[0]
    with np.errstate(all="ignore"):
        LA, lA, LB = (np.asarray(v, np.float64) for v in (logp_fn(A), loglik(A), logp_fn(B)))
        rho = -lA + LA - np.logaddexp(LA, LB - np.log(S).sum())
        k_s, lw_s = smooth(rho, keep)
        lA = np.where(keep, lA, 0.0)
        elpd = log_sum(lw_s + lA) - log_sum(lw_s)
        w = np.exp(lw_s[keep] - lw_s[keep].max())
        ess = w.sum() ** 2 / (w * w).sum()
    return float(elpd), k, k_f, k_s, float(ess), maps, S, U


def moment_match(x, left, logp_fn, loglik_fn, targets, plain_k, plain_elpd, threshold):
    """diagnostics.moment_match's arguments with numpy closures -> Result; a target at or below the threshold is not touched
    and keeps its plain figures."""
    x = np.asarray(x, np.float32)
    R, D = x.shape
    plain_k, plain_elpd = np.asarray(plain_k, np.float64), np.asarray(plain_elpd, np.float64)
    T = len(targets)
    L0 = np.asarray(logp_fn(x), np.float64)
    keep = ~(np.asarray(left).reshape(-1) != 0) & np.isfinite(L0)
    base = np.where(keep, 0.0, -np.inf)
    zeros, _ = weighted_moments(x, base[None], np.zeros(D, np.float32))
    m0_32 = (zeros[0, 4::2] / zeros[0, 1]).astype(np.float32)
    res = Result(~(plain_k <= threshold), plain_elpd.copy(), plain_k.copy(), np.full(T, np.nan), np.full(T, np.nan),
                 np.full(T, np.nan), [""] * T, np.full((T, D), np.nan), np.full((T, D), np.nan), m0_32.astype(np.float64))
    for t in np.flatnonzero(res.attempted):
        elpd, k, k_f, k_s, ess, maps, S, U = match_one(x, keep, L0, logp_fn, lambda rows: loglik_fn(targets[t], rows), threshold,
                                                       m0_32, base)
        if elpd is not None:
            res.elpd[t] = elpd
        res.pareto_k[t], res.pareto_k_full[t], res.pareto_k_split[t], res.is_ess[t], res.maps[t] = k, k_f, k_s, ess, maps
        res.scale[t], res.shift[t] = S, U - res.centre
    return res
