"""Float64 reference of the group log-likelihood (csrc/logo.hip), independent of the kernel's formula.

For the float32 inputs the kernel reads -- the rows x [R, D], an observation table (kind, idx, w, y, scale_idx,
log_scale), group_of [N], slope [N], elem [G] and a site table -- and every (group g, draw r):

  lc[g, r]  the sum over the group's observations of loglik_ref.loglik_from (the CONDITIONAL form);
  lm[g, r]  scipy.stats.multivariate_normal.logpdf of the group's y with mean c + a loc and covariance
            diag(exp(2 s_n)) + exp(2 sj) a a^T, where a = slope, c = eta - a t0 is the linear predictor without the
            group's element t0 = x[r, elem[g]], and (loc, sj) are the element's site chains at the row: y = c + a t + e with
            t ~ N(loc, exp(sj)) is jointly Normal, no integral is evaluated (the MARGINAL form; Normal data only).

`closed_form` restates the kernel's expression in float64 (the self-check of the reference against it: tests/test_logo_host.py);
`bound` is the first-order bound of the kernel's header, per (g, r), from float64 quantities."""
import collections

import numpy as np

import loglik_ref as lr

U = 2.0 ** -24
Quantities = collections.namedtuple("Quantities", ["eta", "s", "A", "ll", "z", "b", "loc", "sj", "A_loc", "A_s", "t0"])


def _f64(a):
    return np.asarray(a, np.float64)


def quantities(table, site, x, slope, elem):
    """eta, s, A, ll, z, b [N, R] and loc, sj, A_loc, A_s, t0 [G, R] in float64 (z and b are 0 for Bernoulli data; the site
    columns None without a site table)."""
    x = _f64(x)
    idx, w = np.asarray(table.idx, np.int64), _f64(table.w)
    terms = w[:, :, None] * x.T[idx]                                           # [N, T, R]
    eta, A = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    si = np.asarray(table.scale_idx, np.int64).reshape(-1)
    s = _f64(table.log_scale).reshape(-1)[:, None] + np.where((si >= 0)[:, None], x.T[np.maximum(si, 0)], 0.0)
    y = _f64(table.y).reshape(-1)
    ll = lr.loglik_from(int(table.kind), eta, s, y[:, None])
    normal = int(table.kind) == lr.NORMAL
    z = (y[:, None] - eta) * np.exp(-s) if normal else np.zeros_like(eta)
    b = _f64(slope).reshape(-1)[:, None] * np.exp(-s) if normal else np.zeros_like(eta)
    loc = sj = A_loc = A_s = t0 = None
    if site is not None:
        elem = np.asarray(elem, np.int64).reshape(-1)
        chain = lambda c0, ix, wt: (_f64(c0)[elem][:, None] + (_f64(wt)[elem][:, :, None] * x.T[np.asarray(ix, np.int64)[elem]]).sum(axis=1),
                                    np.abs(_f64(c0)[elem])[:, None] + np.abs(_f64(wt)[elem][:, :, None] * x.T[np.asarray(ix, np.int64)[elem]]).sum(axis=1))
        (loc, A_loc), (sj, A_s) = chain(site.loc0, site.loc_idx, site.loc_w), chain(site.log_scale0, site.scale_idx, site.scale_w)
        t0 = x.T[elem]
    return Quantities(eta, s, A, ll, z, b, loc, sj, A_loc, A_s, t0)


def members_of(group_of, g):
    return np.flatnonzero(np.asarray(group_of).reshape(-1) == g)


def conditional(q, group_of, G):
    """lc [G, R]: the float64 sum of the pointwise log-likelihoods of every group; 0 for an empty one."""
    return np.stack([q.ll[members_of(group_of, g)].sum(axis=0) for g in range(G)])


def marginal(table, q, group_of, G, slope):
    """lm [G, R] by multivariate_normal.logpdf; 0 for an empty group."""
    from scipy.stats import multivariate_normal
    y, a_all = _f64(table.y).reshape(-1), _f64(slope).reshape(-1)
    R = q.eta.shape[1]
    out = np.zeros((G, R))
    for g in range(G):
        mem = members_of(group_of, g)
        if not mem.size:
            continue
        a = a_all[mem]
        for r in range(R):
            mean = q.eta[mem, r] - a * q.t0[g, r] + a * q.loc[g, r]
            cov = np.diag(np.exp(2.0 * q.s[mem, r])) + np.exp(2.0 * q.sj[g, r]) * np.outer(a, a)
            out[g, r] = multivariate_normal.logpdf(y[mem], mean=mean, cov=cov, allow_singular=False)
    return out


def _sums(q, group_of, G):
    S_ll, S_bz, S_bb = (np.stack([v[members_of(group_of, g)].sum(axis=0) for g in range(G)]) for v in (q.ll, q.b * q.z, q.b * q.b))
    tau = np.exp(-2.0 * q.sj)
    m = q.t0 - q.loc
    return S_ll, S_bz, S_bb, tau, m, S_bb + tau, S_bz - m * tau


def closed_form(q, group_of, G):
    """The kernel's expression, restated in float64: S_ll - 0.5 (m^2 tau - q^2 / P) - 0.5 log1p(S_bb / tau); 0 for an empty group."""
    S_ll, S_bz, S_bb, tau, m, P, qq = _sums(q, group_of, G)
    lm = S_ll - 0.5 * (m * m * tau - qq * qq / P) - 0.5 * np.log1p(S_bb / tau)
    empty = np.array([members_of(group_of, g).size == 0 for g in range(G)])
    lm[empty] = 0.0
    return lm


def bound(table, q, group_of, G, lm):
    """[G, R]: the header's first-order bound of |lm_dev - lm|,
    E_ll + |q / P| E_bz + 0.5 (q^2 / P^2 + 1 / P) E_bb + 3 u A_loc tau |c| + 3 u A_s (S_bb / P + c^2 tau) + u |lm|."""
    T = np.asarray(table.idx).shape[1]
    ems, az, asb = np.exp(-q.s), np.abs(q.z), np.abs(q.s)
    e_ll = U * (T * q.A * ems * az + q.z ** 2 * (5.0 + asb) + 3.0 * asb + np.abs(q.ll))
    e_bz = U * (T * q.A * ems * np.abs(q.b) + np.abs(q.b * q.z) * (8.0 + 2.0 * asb))
    e_bb = U * q.b ** 2 * (7.0 + 2.0 * asb)
    E_ll, E_bz, E_bb = (np.stack([v[members_of(group_of, g)].sum(axis=0) for g in range(G)]) for v in (e_ll, e_bz, e_bb))
    S_ll, S_bz, S_bb, tau, m, P, qq = _sums(q, group_of, G)
    c = (m * S_bb + S_bz) / P
    return (E_ll + np.abs(qq / P) * E_bz + 0.5 * (qq * qq / (P * P) + 1.0 / P) * E_bb + 3.0 * U * q.A_loc * tau * np.abs(c)
            + 3.0 * U * q.A_s * (S_bb / P + c * c * tau) + U * np.abs(lm))
