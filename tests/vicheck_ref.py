"""The float64 definition of the variational-fit check (csrc/vicheck.hip, csrc/psis.hip: arp_vi_draws, arp_psis_weights,
arp_vi_fold; diagnostics.vi_check): the draws from ppc_ref's Philox restatement with the sine branch added, the smoothed
log weights of psis_ref's row scattered back through the stable order, the fold in np.longdouble, and the whole pipeline
on any log joint handed in as a function."""
import collections
import math

import numpy as np

import ppc_ref
import psis_ref

LOG_2PI = math.log(2.0 * math.pi)
Draws = collections.namedtuple("Draws", ["z", "z32", "x32", "logq"])
Pipeline = collections.namedtuple("Pipeline", ["draws", "logp", "grad", "e", "e0", "ll", "mask", "out8", "lw", "elem", "tot"])


def normals(D, g, seed):
    """z [len(g), D] float64: for global draw numbers g and element d = 4 e + i, ONE philox4x32_10(counter (e, lo32 g, hi32 g,
    0), key (lo32 seed, hi32 seed)); words (0, 1) give rho cos(2 pi a), rho sin(2 pi a), words (2, 3) the next pair."""
    g = np.asarray(g, np.uint64).reshape(-1, 1)
    E = (D + 3) // 4
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = ppc_ref.philox4x32_10((np.arange(E, dtype=np.uint64)[None, :], g & ppc_ref.M32, g >> np.uint64(32), 0),
                              (seed & 0xFFFFFFFF, seed >> 32))
    z = np.empty((g.shape[0], 4 * E))
    for p in range(2):
        up, a = ppc_ref.normal_inputs(w[2 * p], w[2 * p + 1])
        rho = np.sqrt(-2.0 * np.log(up))
        z[:, 2 * p::4] = rho * np.cos(2.0 * np.pi * (a - 1.0))
        z[:, 2 * p + 1::4] = rho * np.sin(2.0 * np.pi * (a - 1.0))
    return z[:, :D]


def logq_of(z32, scale):
    """log q of rows of float32 normals z32 under scales `scale` (float32 values), float64."""
    z = np.asarray(z32, np.float64)
    s = np.asarray(scale, np.float32).astype(np.float64)
    return -np.sum(0.5 * z * z + np.log(s)[None, :], axis=1) - 0.5 * z.shape[1] * LOG_2PI


def logq_terms(z32, scale):
    """sum of the absolute values of logq's terms, per row (what its error bound scales with)."""
    z = np.asarray(z32, np.float64)
    s = np.asarray(scale, np.float32).astype(np.float64)
    return np.sum(0.5 * z * z + np.abs(np.log(s))[None, :], axis=1) + 0.5 * z.shape[1] * LOG_2PI


def draws(loc, scale, n, seed, offset=0):
    """-> Draws: z float64 (the definition), z32 its float32 rounding, x32 = float32(scale z32 + loc), logq of z32."""
    loc, scale = np.asarray(loc, np.float32), np.asarray(scale, np.float32)
    z = normals(loc.size, np.uint64(offset) + np.arange(n, dtype=np.uint64), seed)
    z32 = z.astype(np.float32)
    x32 = (scale.astype(np.float64)[None, :] * z32.astype(np.float64) + loc.astype(np.float64)[None, :]).astype(np.float32)
    return Draws(z, z32, x32, logq_of(z32, scale))


def weights_row(ll, mask=None):
    """(out8, lw [R], tail) of one row of float32 ll: psis_ref.psis_row's columns over the kept draws, the smoothed log
    weight of every draw in its own place (-inf: masked; NaN: a kept draw of a row with a non-finite kept ll) and the
    indices of the draws whose weight the fit replaced (empty for a row that is not fitted)."""
    ll = np.asarray(ll).reshape(-1)
    R = ll.size
    keep = np.ones(R, bool) if mask is None else (np.asarray(mask).reshape(-1) == 0)
    k = ll[keep].astype(np.float64)
    out8 = psis_ref.psis_row(k)
    lw = np.full(R, -np.inf)
    none = np.zeros(0, np.int64)
    if k.size == 0:
        return out8, lw, none
    if not np.all(np.isfinite(k)):
        lw[keep] = np.nan
        return out8, lw, none
    order = np.argsort(k, kind="stable")
    s = k[order]
    raw = -s - np.max(-s)
    lws = raw.copy()
    M = psis_ref.tail_len(k.size)
    fitted = False
    if M >= 5:
        cutoff = float(raw[M])
        kk, sigma = psis_ref.gpdfit((np.exp(raw[:M]) - math.exp(cutoff))[::-1])
        if np.isfinite(kk) and np.isfinite(sigma):
            fitted = True
            p = (np.arange(1, M + 1, dtype=np.float64) - 0.5) / M
            q = -sigma * np.log1p(-p) if kk == 0.0 else sigma * np.expm1(-kk * np.log1p(-p)) / kk
            with np.errstate(all="ignore"):
                lws[:M] = np.minimum(np.log(math.exp(cutoff) + q), 0.0)[::-1]
    back = np.empty(k.size)
    back[order] = lws
    lw[keep] = back
    return out8, lw, (np.flatnonzero(keep)[order[:M]] if fitted else none)


def fold(z, grad, e, ll, lw, scale, e0):
    """(elem [D, 9], tot [5], elem_abs [D, 9], tot_abs [5]) in np.longdouble over the draws with lw > -inf; the _abs arrays
    hold the sums of the absolute values of the terms."""
    L = np.longdouble
    lw = np.asarray(lw, np.float64)
    kept = lw > -np.inf
    z, g, c = (np.asarray(v, np.float32)[kept].astype(L) for v in (z, grad, e))
    sc, c0 = np.asarray(scale, np.float32).astype(L), np.asarray(e0, np.float32).astype(L)
    w = np.exp(lw[kept].astype(L))[:, None]
    l = np.asarray(ll, np.float32)[kept].astype(L)
    u = sc[None, :] * g
    c = c - c0[None, :]
    terms = [u, u * u, u * z, (u * z) ** 2, (u + z) ** 2, w * z, w * z * z, w * c, w * c * c]
    D = sc.size
    elem = np.stack([t.sum(axis=0) if t.size else np.zeros(D, L) for t in terms], axis=1)
    elem_abs = np.stack([np.abs(t).sum(axis=0) if t.size else np.zeros(D, L) for t in terms], axis=1)
    tot = np.array([L(kept.sum()), w.sum(), (w * w).sum(), l.sum(), l.min() if l.size else L(np.inf)], L)
    tot_abs = np.array([L(kept.sum()), w.sum(), (w * w).sum(), np.abs(l).sum(), L(0)], L)
    return elem, tot, elem_abs, tot_abs


def pipeline_from(z32, logq, logp, grad, e, e0, scale):
    """Steps 2 to 5 of diagnostics.vi_check on given arrays -> Pipeline (draws = None): ll = float32(logq - float64(logp)),
    the mask, the weights of the one row, the fold."""
    grad32, e32, e032 = (np.asarray(v).astype(np.float32) for v in (grad, e, e0))
    ll = (np.asarray(logq, np.float64) - np.asarray(logp).astype(np.float64)).astype(np.float32)
    bad = ~(np.isfinite(np.asarray(logp, np.float64)) & np.isfinite(grad32).all(axis=1) & np.isfinite(e32).all(axis=1))
    out8, lw, _ = weights_row(ll, bad.astype(np.uint8))
    elem, tot, _, _ = fold(z32, grad32, e32, ll, lw, scale, e032)
    return Pipeline(None, logp, grad32, e32, e032, ll, bad, out8, lw, elem.astype(np.float64), tot.astype(np.float64))


def pipeline(logp_grad, to_centered, loc, scale, n, seed):
    """diagnostics.vi_check restated -> Pipeline.  logp_grad(x32) -> (logp [n], grad [n, D]) and to_centered(x32) -> [n, D]
    are the density's, of any float type."""
    d = draws(loc, scale, n, seed)
    logp, grad = logp_grad(d.x32)
    e0 = to_centered(np.asarray(loc, np.float32).reshape(1, -1))[0]
    return pipeline_from(d.z32, d.logq, logp, grad, to_centered(d.x32), e0, scale)._replace(draws=d)


# ---- the known answer: radon MN, whose posterior is exactly normal ----
R, SEED = 65536, 2018


class Case(object):
    """radon MN under one parameterisation: the exact normal posterior from the float64 oracle (P and the mean as
    tests/test_gpu_hmc.py: test_radon_posterior_means_config2 takes them), the KL-optimal q, and the reference pipeline on it."""

    def __init__(self, oracle_lib, kind):
        import helpers
        self.sp = sp = helpers.spec("radon_MN")
        self.orc = orc = oracle_lib.OracleModel(sp)
        self.a, self.b = a, b = helpers.params(sp, kind)
        D = sp.D
        _, g0 = orc.logp_grad(np.zeros((1, D)), a, b)
        _, gI = orc.logp_grad(np.eye(D), a, b)
        self.P = P = -(gI - g0)
        self.mean = np.linalg.solve(P, g0[0])
        self.sd = np.sqrt(np.diag(np.linalg.inv(P)))
        self.loc = self.mean.astype(np.float32)
        self.scale = (1.0 / np.sqrt(np.diag(P))).astype(np.float32)
        self.const = float(orc.logp_const(b))
        self.logp_mean = float(orc.logp_grad(self.mean[None], a, b)[0][0])

    def run(self, loc=None):
        loc = self.loc if loc is None else loc
        p = pipeline(lambda x: self.orc.logp_grad(x, self.a, self.b), lambda x: self.orc.transform(x, self.a, self.b),
                        loc, self.scale, R, SEED)
        from autoreparam_amd import diagnostics
        return p, diagnostics.vi_check_summary(p.elem, p.tot, p.out8, loc, self.scale, p.e0, self.const)


def check_known_answer(c, s, say=print):
    """The statistical bounds of the known answer on a ViCheckSummary `s` of case `c` at loc = mean (CP)."""
    D = c.sp.D
    P, sq = c.P, c.scale.astype(np.float64)
    assert s.draws == R
    say("k-hat %.4f (threshold %.4f)" % (s.pareto_k, s.pareto_k_threshold))
    assert s.pareto_k < 0.7
    _, logdet = np.linalg.slogdet(P)
    evidence = c.logp_mean + 0.5 * D * math.log(2.0 * math.pi) - 0.5 * logdet + c.const
    say("log evidence %.4f against %.4f, se %.4g" % (s.log_evidence, evidence, s.log_evidence_se))
    assert abs(s.log_evidence - evidence) <= 5.0 * s.log_evidence_se
    A = P * np.outer(sq, sq)                                          # P Sigma_q up to similarity
    kl = 0.5 * (np.trace(A) - D - np.linalg.slogdet(A)[1])
    say("KL %.4f against %.4f, se %.4g" % (s.kl_estimate, kl, s.kl_estimate_se))
    assert abs(s.kl_estimate - kl) <= 5.0 * s.kl_estimate_se
    t_loc, t_scale = np.abs(s.elbo_grad_loc / s.elbo_grad_loc_se), np.abs(s.elbo_grad_scale / s.elbo_grad_scale_se)
    say("largest |gradient| / se: loc %.2f, scale %.2f" % (t_loc.max(), t_scale.max()))
    assert t_loc.max() <= 6.0 and t_scale.max() <= 6.0
    off = A - np.diag(np.diag(A))
    gap = np.sqrt((off * off).sum(axis=1))
    say("score gap: largest relative deviation %.4f" % np.abs(s.score_gap / gap - 1.0).max())
    assert np.abs(s.score_gap / gap - 1.0).max() <= 0.05
    say("corrected sd: largest relative deviation %.4f (q's own: %.4f)" % (np.abs(s.sd_ratio * sq / c.sd - 1.0).max(),
                                                                          np.abs(sq / c.sd - 1.0).max()))
    assert np.abs(s.sd_ratio * sq / c.sd - 1.0).max() <= 0.05
