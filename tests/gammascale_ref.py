"""float64 restatement of german_credit_gammascale (reference models.py:926-964) for the tests: log density and
gradient under the VIP parameterisation, the state converters, the VI parameter gradients (dparam) and plain
fixed-step HMC drawing its momenta and Metropolis uniforms from the oracle's exported random streams
(oracle.c: orc_stream; the layout of oracle_impl.h: draw_momentum for German credit, one top-level scalar and two
sliced parts, consecutive elements per slot).  Written from the model's formulas, not from the kernels:

  ols ~ N(0, 10)                   top level: ot ~ N(0, 10^b0), ols = 10^(1-b0) ot
  bls_d = log g_d, g_d ~ Gamma(1/2, 1/2)   never reparameterised (a, b of bls are ignored)
  beta_d ~ N(0, exp(ols + bls_d))  bt_d ~ N(0, exp(b_d s_d)), beta_d = exp((1-b_d) s_d) bt_d, s_d = ols + bls_d
  y_n ~ Bernoulli(logits = X beta)

`prior="lognormal"` switches in german_credit_lognormalcentered (bls_d ~ N(ols, 1) under its own a, b), the model the
oracle covers: the tests pin this module's HMC and RNG layout against the oracle with it.  Arrays are [C, D].
"""
import ctypes as C

import numpy as np

HALF_LOG_2PI = 0.9189385332046727


class GermanRef(object):
    def __init__(self, X, y, prior="gamma"):
        assert prior in ("gamma", "lognormal")
        self.X = np.asarray(X, np.float32).astype(np.float64)
        self.y = np.asarray(y, np.float32).astype(np.float64)
        self.N, self.F = self.X.shape
        self.D = 1 + 2 * self.F
        self.prior = prior

    # ---- coordinates ----
    def _split(self, q, a, b):
        F = self.F
        q = np.asarray(q, np.float64)
        a = np.asarray(a, np.float32).astype(np.float64); b = np.asarray(b, np.float32).astype(np.float64)
        c0 = 10.0 ** (1.0 - b[0])
        ols = c0 * q[:, 0]
        bl = q[:, 1:1 + F]
        bt = q[:, 1 + F:]
        ab, bb = a[1:1 + F], b[1 + F:]
        if self.prior == "gamma":
            bls = bl
            s = ols[:, None] + bls           # log scale of beta
        else:
            bls = bl + (1.0 - ab) * ols[:, None]
            s = bls
        return c0, ols, bl, bls, bt, ab, bb, s

    def logp_const(self, b):
        """constant the engine drops (arp_model_logp_const): the same for both priors"""
        return -(1.0 + 2.0 * self.F) * HALF_LOG_2PI - float(np.float32(b[0])) * np.log(10.0)

    def logp_grad(self, q, a, b):
        """(log density without logp_const, gradient) in the coordinates (a, b) define"""
        F = self.F
        c0, ols, bl, bls, bt, ab, bb, s = self._split(q, a, b)
        q = np.asarray(q, np.float64)
        s0i = 10.0 ** (-np.float64(np.float32(b[0])))
        eb = np.exp((1.0 - bb) * s)
        beta = eb * bt
        eta = beta @ self.X.T                                     # [C, N]
        lik = (self.y * eta - (np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta))))).sum(axis=1)
        v = (self.y - (0.5 + 0.5 * np.tanh(0.5 * eta))) @ self.X   # [C, F]: y - sigmoid(eta)
        e = np.exp(-bb * s)
        zb = bt * e
        h = bb * (zb * zb - 1.0) + v * (1.0 - bb) * beta           # d/ds of the beta terms and the likelihood
        u0 = q[:, 0] * s0i
        g = np.zeros_like(q)
        g[:, 1 + F:] = v * eb - zb * e
        lp = lik - 0.5 * u0 * u0 + (-0.5 * zb * zb - bb * s).sum(axis=1)
        if self.prior == "gamma":
            g[:, 1:1 + F] = h + 0.5 - 0.5 * np.exp(bls)
            g[:, 0] = c0 * h.sum(axis=1) - u0 * s0i
            lp += (0.5 * bls - 0.5 * np.exp(bls)).sum(axis=1)
        else:
            r = bl - ab * ols[:, None]
            g[:, 1:1 + F] = h - r
            g[:, 0] = c0 * (ab * r + (1.0 - ab) * h).sum(axis=1) - u0 * s0i
            lp += (-0.5 * r * r).sum(axis=1)
        return lp, g

    def to_centered(self, q, a, b):
        F = self.F
        c0, ols, bl, bls, bt, ab, bb, s = self._split(q, a, b)
        x = np.empty((np.shape(q)[0], self.D))
        x[:, 0] = ols
        x[:, 1:1 + F] = bls
        x[:, 1 + F:] = np.exp((1.0 - bb) * s) * bt
        return x

    def from_centered(self, x, a, b):
        F = self.F
        x = np.asarray(x, np.float64)
        a = np.asarray(a, np.float32).astype(np.float64); b = np.asarray(b, np.float32).astype(np.float64)
        c0 = 10.0 ** (1.0 - b[0])
        ols = x[:, 0]
        bls = x[:, 1:1 + F]
        s = ols[:, None] + bls if self.prior == "gamma" else bls
        q = np.empty_like(x)
        q[:, 0] = ols / c0
        q[:, 1:1 + F] = bls if self.prior == "gamma" else bls - (1.0 - a[1:1 + F]) * ols[:, None]
        q[:, 1 + F:] = x[:, 1 + F:] * np.exp(-(1.0 - b[1 + F:]) * s)
        return q

    def dparam(self, q, g, a, b, w=1.0):
        """(da, db): derivatives of the log density w.r.t. a and b at fixed sampler coordinates q (gradient g there),
        the VI kernel's `dparam`; `w` is the weight of the constant 1 of the affine forms (the row-part prior weight)."""
        assert self.prior == "gamma"
        F = self.F
        c0, ols, bl, bls, bt, ab, bb, s = self._split(q, a, b)
        q = np.asarray(q, np.float64); g = np.asarray(g, np.float64)
        da = np.zeros_like(q); db = np.zeros_like(q)
        db[:, 0] = -np.log(10.0) * (q[:, 0] * g[:, 0] + w)
        db[:, 1 + F:] = -s * (bt * g[:, 1 + F:] + w)
        return da, db

    # ---- HMC on the oracle's streams ----
    def hmc(self, oracle_lib, q0, a, b, eps, L, n, seed, chain_offset=0, lanes=4):
        """n plain HMC transitions (unit mass, fixed element-wise step `eps`, L leapfrog steps) per chain, as
        oracle_impl.h: hmc_transition.  Returns dict(x [n, C, D] states after each step, acc [n, C], margin [n, C] =
        log u - log alpha, escale [n, C] = largest energy term compared, q, logp)."""
        q = np.array(q0, np.float64)
        Cn, D = q.shape
        eps = np.asarray(eps, np.float32).astype(np.float64)
        mom, logu = self.draws(oracle_lib, Cn, n, seed, chain_offset, lanes)
        lp, g = self.logp_grad(q, a, b)
        xs = np.zeros((n, Cn, D)); acc = np.zeros((n, Cn), np.uint8)
        mg = np.zeros((n, Cn)); es = np.zeros((n, Cn))
        for t in range(n):
            p = mom[t].copy()
            ke0 = 0.5 * (p * p).sum(axis=1)
            q1 = q.copy()
            p = p + 0.5 * eps * g
            for l in range(L):
                q1 = q1 + eps * p
                lp1, g1 = self.logp_grad(q1, a, b)
                p = p + (1.0 if l + 1 < L else 0.5) * eps * g1
            ke1 = 0.5 * (p * p).sum(axis=1)
            la = (lp1 - lp) + (ke0 - ke1)
            la = np.where(np.isfinite(la), la, -np.inf)
            ok = logu[t] < la
            mg[t] = logu[t] - la
            es[t] = np.maximum.reduce([np.abs(lp), np.abs(lp1), ke0, ke1])
            q = np.where(ok[:, None], q1, q); g = np.where(ok[:, None], g1, g); lp = np.where(ok, lp1, lp)
            xs[t] = q; acc[t] = ok
        return dict(x=xs, acc=acc, margin=mg, escale=es, q=q, logp=lp)

    def draws(self, oracle_lib, Cn, n, seed, chain_offset, lanes):
        """momenta [n, C, D] and log u [n, C] of n transitions, from the per-slot word streams"""
        F, D = self.F, self.D
        per_lane = (F + lanes - 1) // lanes
        nd = 1 + 2 * per_lane                 # normals every slot draws: the scalar, then each part's slice
        npair = (nd + 1) // 2
        W = 2 * npair + 1                     # words of one transition: the pairs, then the Metropolis uniform
        L_ = oracle_lib.lib()
        mom = np.zeros((n, Cn, D)); logu = np.zeros((n, Cn))
        buf = np.empty(n * W, np.uint32)
        for c in range(Cn):
            for s in range(lanes):
                L_.orc_stream(C.c_uint64(seed), C.c_uint64(chain_offset + c), C.c_uint32(s), C.c_uint32(lanes),
                              C.c_int(n * W), buf.ctypes.data_as(C.c_void_p))
                w = buf.reshape(n, W)
                z = _box_muller(w[:, 0:2 * npair:2], w[:, 1:2 * npair:2])        # [n, npair, 2]
                z = z.reshape(n, 2 * npair)[:, :nd]
                if s == 0:
                    mom[:, c, 0] = z[:, 0]
                    logu[:, c] = np.log(((w[:, W - 1] >> 8) + 1).astype(np.float64) * 2.0 ** -24)
                for ii in range(1, nd):
                    part, k = divmod(ii - 1, per_lane)
                    j = s * per_lane + k
                    if j < F:
                        mom[:, c, 1 + part * F + j] = z[:, ii]
        return mom, logu


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _box_muller(w0, w1):
    """oracle.c: orc_normal_pair, every float32 operation rounded as float32 (the functions of the C library are
    taken as correctly rounded)"""
    u = _f32(w0.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33)
    rev = (w1 & 0x007fffff).astype(np.float64) * 2.0 ** -23
    r = _f32(np.sqrt(_f32(_f32(-1.3862943611198906) * _f32(np.log2(u)))))
    ang = _f32(_f32(6.283185307179586) * rev)
    return np.stack([_f32(r * _f32(np.cos(ang))), _f32(r * _f32(np.sin(ang)))], axis=-1)
