"""Float64 restatement of arp_site_prior_draws, written from the contract in include/autoreparam.h -- NOT from
csrc/prior_draw.hip, which is under test against this file.  Philox4x32-10 in numpy integers; the words -> u', a exactly as
float32 forms them (they are inputs: both are exact in float64); everything after that in float64.

`philox(c0, c1, c2, c3, k0, k1)` -> four uint64 arrays holding the 32-bit words
`draw(table, n, seed, offset, parents=None)` -> Draws(x [n, D], undrawn [n], terms): the table's columns as given (the
    float32-rounded host copies of an uploaded table), draws offset ... offset + n - 1.  With `parents` (the device's own
    float32 output [n, D]) every x_d is computed from THOSE parents -- teacher forcing, so that float32 error does not
    compound down the hierarchy; without, from the reference's own earlier elements.  terms: what the bounds are made of.
`bound(table, d)`     -> [n, D], the header's first-order bound of x per form
`undecided(table, d)` -> [n, D] bool: log-Gamma elements one of whose attempts, up to the accepting one, has |m| <= E_m
`tainted(table, marks)` -> [n, D] bool: the marked elements and everything that descends from them in the same draw"""
import collections

import numpy as np

NORMAL, NORMAL_SOFTPLUS, LOG_GAMMA = 0, 1, 2
U32 = 2.0 ** -24
ATTEMPTS = 32
MASK = np.uint64(0xFFFFFFFF)

Draws = collections.namedtuple("Draws", ["x", "undrawn", "terms"])


def philox(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3 = (np.asarray(v, np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + np.uint64(0x9E3779B9)) & MASK
        k1 = (k1 + np.uint64(0xBB67AE85)) & MASK
    return c0, c1, c2, c3


def open_uniform(w):
    """u' = fma((float)w, 2^-32, 2^-33) as float32 forms it, in float64: the conversion rounds to nearest even, the
    multiply-add is exact in float64 (34 bits at most) and rounds once to float32."""
    f = np.asarray(w, np.uint64).astype(np.float32).astype(np.float64)
    return (f * 2.0 ** -32 + 2.0 ** -33).astype(np.float32).astype(np.float64)


def cos_revolutions(frac):
    """cos(2 pi frac) for frac in [0, 1) with the relative accuracy of float64 EVERYWHERE: frac = q / 4 + r, q the nearest
    quarter and |r| <= 1 / 8 (exact: frac is a multiple of 2^-23), so that cos is +-cos(2 pi r) or -+sin(2 pi r) and the
    zeros at a quarter and three quarters of a revolution are exact zeros, as cospi's are -- cos(pi / 2) in float64 is
    6e-17, which against an exact 0 is an error of 100 % of the value."""
    q = np.rint(4.0 * frac)
    r = 2.0 * np.pi * (frac - q / 4.0)
    k = q.astype(np.int64) % 4
    return np.where(k == 0, np.cos(r), np.where(k == 1, -np.sin(r), np.where(k == 2, -np.cos(r), np.sin(r))))


def standard_normal(w0, w1):
    """z = sqrt(-2 log u') cospi(2 a), a = 1 + (w1 mod 2^23) 2^-23: cos over the fraction of a revolution, which is exact"""
    frac = (np.asarray(w1, np.uint64) & np.uint64(0x7FFFFF)).astype(np.float64) * 2.0 ** -23
    return np.sqrt(-2.0 * np.log(open_uniform(w0))) * cos_revolutions(frac)


def _softplus(s):
    return np.maximum(s, 0.0) + np.log1p(np.exp(-np.abs(s)))


def _chain(src, idx, w, c, d):
    """(c + sum_t w[d][t] src[idx[d][t]], |c| + sum_t |w src|) over the elements before d; one not drawn yet reads as 0"""
    value = np.full(src.shape[0], float(c))
    size = np.abs(value)
    D = src.shape[1]
    for t in range(idx.shape[1]):
        i = min(max(int(idx[d, t]), 0), D - 1)
        term = float(w[d, t]) * (src[:, i] if i < d else np.zeros(src.shape[0]))
        value = value + term
        size = size + np.abs(term)
    return value, size


def draw(table, n, seed, offset, parents=None):
    form = np.asarray(table.form).reshape(-1)
    D = form.size
    loc_idx, scale_idx = np.asarray(table.loc_idx, np.int64), np.asarray(table.scale_idx, np.int64)
    loc_w, scale_w = np.asarray(table.loc_w, np.float64), np.asarray(table.scale_w, np.float64)
    loc0, ls0 = np.asarray(table.loc0, np.float64).reshape(-1), np.asarray(table.log_scale0, np.float64).reshape(-1)
    g = np.arange(int(n), dtype=np.uint64) + np.uint64(int(offset))
    g_lo, g_hi = g & MASK, g >> np.uint64(32)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    x = np.zeros((int(n), D))
    src = x if parents is None else np.asarray(parents, np.float64)
    names = ("z", "loc", "s", "A_loc", "A_s", "sigma", "t", "log_u", "log_ub", "min_slack")
    T = {name: np.full((int(n), D), np.nan) for name in names}
    undrawn = np.zeros(int(n), bool)
    with np.errstate(all="ignore"):
        for d in range(D):
            s, a_s = _chain(src, scale_idx, scale_w, ls0[d], d)
            T["s"][:, d], T["A_s"][:, d] = s, a_s
            f = int(form[d])
            if f == LOG_GAMMA:
                k = loc0[d]
                if not (np.isfinite(k) and k > 0):
                    x[:, d] = np.nan
                    continue
                boost = k < 1
                a = k + 1 if boost else k
                dd = a - 1.0 / 3.0
                c = 1.0 / np.sqrt(9.0 * dd)
                todo = np.ones(int(n), bool)
                value = np.full(int(n), np.nan)
                slack = np.full(int(n), np.inf)          # min over the attempts so far of |m| - E_m
                for j in range(ATTEMPTS):
                    at = np.flatnonzero(todo)
                    if not at.size:
                        break
                    w0, w1, w2, w3 = philox(d, g_lo[at], g_hi[at], 1 + j, k0, k1)
                    z = standard_normal(w0, w1)
                    t = 1.0 + c * z
                    log_u = np.log(open_uniform(w2))
                    lt = np.log(t)
                    t3 = t ** 3
                    sum2 = 0.5 * z * z + dd - dd * t3
                    rhs = sum2 + 3.0 * dd * lt
                    m = rhs - log_u
                    big_t = 29.0 * np.abs(t - 1.0) / t + 1.0
                    e_m = U32 * (19.0 * z * z + 6.0 * dd + 8.0 * dd * t3 + 39.0 * dd * np.abs(lt) + np.abs(sum2) + np.abs(rhs)
                                 + 1.0 + 6.0 * np.abs(log_u) + 3.0 * dd * np.abs(1.0 - t3) * big_t)
                    positive = t > 0
                    slack[at] = np.minimum(slack[at], np.where(positive, np.abs(m) - e_m, np.inf))
                    ok = positive & (log_u < rhs)
                    log_ub = np.log(open_uniform(w3))
                    b = log_ub / k if boost else np.zeros(at.size)
                    hit = at[ok]
                    value[hit] = (np.log(dd) + 3.0 * lt[ok] + b[ok]) - s[hit]
                    T["z"][hit, d], T["t"][hit, d], T["log_u"][hit, d], T["log_ub"][hit, d] = z[ok], t[ok], log_u[ok], log_ub[ok]
                    todo[hit] = False
                undrawn |= todo
                T["min_slack"][:, d] = slack
                x[:, d] = value
            else:
                w0, w1, _, _ = philox(d, g_lo, g_hi, 0, k0, k1)
                z = standard_normal(w0, w1)
                loc, a_loc = _chain(src, loc_idx, loc_w, loc0[d], d)
                sigma = _softplus(s) if f == NORMAL_SOFTPLUS else np.exp(s)
                x[:, d] = loc + sigma * z
                T["z"][:, d], T["loc"][:, d], T["A_loc"][:, d], T["sigma"][:, d] = z, loc, a_loc, sigma
    return Draws(x, undrawn, T)


def bound(table, d):
    """include/autoreparam.h: arp_site_prior_draws, the three forms' bounds of x, in float64"""
    form = np.asarray(table.form).reshape(-1)[None, :]
    k = np.asarray(table.loc0, np.float64).reshape(-1)[None, :]
    T, x = d.terms, np.abs(d.x)
    with np.errstate(all="ignore"):
        z = np.abs(T["z"])
        b0 = 3.0 * T["A_loc"] + T["sigma"] * z * (25.0 + 3.0 * T["A_s"]) + x
        b1 = 3.0 * T["A_loc"] + z * (3.0 * T["A_s"] + 6.0 + 20.0 * T["sigma"]) + x
        boost = k < 1
        dd = np.where(boost, k + 1.0, k) - 1.0 / 3.0
        t = T["t"]
        lt = np.log(t)
        big_t = 29.0 * np.abs(t - 1.0) / t + 1.0
        L = np.log(dd) + 3.0 * lt
        B = np.where(boost, T["log_ub"] / k, 0.0)
        b2 = (5.0 + 6.0 * np.abs(np.log(dd)) + 3.0 * big_t + 21.0 * np.abs(lt) + np.abs(L)
              + np.where(boost, (1.0 + 7.0 * np.abs(T["log_ub"])) / k, 0.0) + np.abs(L + B) + 3.0 * T["A_s"] + x)
    return U32 * np.where(form == LOG_GAMMA, b2, np.where(form == NORMAL_SOFTPLUS, b1, b0))


def undecided(table, d):
    form = np.asarray(table.form).reshape(-1)[None, :]
    with np.errstate(invalid="ignore"):
        return (form == LOG_GAMMA) & (d.terms["min_slack"] <= 0.0)


def tainted(table, marks):
    """`marks` [n, D] and every element a term of non-zero weight ties to a marked or tainted one, in ancestral order"""
    out = np.array(marks, bool)
    D = out.shape[1]
    form = np.asarray(table.form).reshape(-1)
    columns = ((np.asarray(table.loc_idx), np.asarray(table.loc_w)), (np.asarray(table.scale_idx), np.asarray(table.scale_w)))
    for d in range(D):
        for idx, w in columns[1:] if form[d] == LOG_GAMMA else columns:      # (the log-Gamma form does not read its loc terms)
            for t in range(idx.shape[1]):
                i = int(idx[d, t])
                if w[d, t] != 0 and 0 <= i < d:
                    out[:, d] |= out[:, i]
    return out
