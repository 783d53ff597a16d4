"""float64 yardstick of the single-chain ESS (arp_ess / arp_ess_ws) that also says WHERE each series' sum is cut.

The statistic is oracle/ess_ref.py: ess_direct -- tfp.mcmc.effective_sample_size with its defaults, from the definition
of the lag sums -- computed in float64 on the float32 trace the kernel sees, lag by lag and only as far as the first
negative one, so it costs O(S cut) and serves series of any length.  tests/test_ess_routes_host.py holds it to
ess_ref.ess_fft on the AR(1) traces of the older tests.

    rho_k = c_k / c_0,   c_k = sum_{t < S-k} (x_t - m)(x_{t+k} - m) / (S - k)
    cut   = the first k with rho_k < 0 (S if there is none)
    tau   = -1 + 2 sum_{k < cut} (S - k)/S rho_k,     ESS = S / tau
    sens  = min(2 (S - cut + 1)/S rho_{cut-1},  2 (S - cut)/S |rho_cut|) / tau
            the relative change of the ESS if the cut moved one lag either way (the first term alone where cut = S)
"""
import collections

import numpy as np

# ess, tau, sens: [n] float64 (nan for a constant series and for S = 1); cut: [n] int64 (0 where ess is nan);
# rho: [max cut + 1, n] float64, rho[k, i] for k <= cut[i] (k < S), nan past that
Ess = collections.namedtuple("Ess", "ess tau cut rho sens")


def ess(x):
    """x [S, n] (the float32 trace) -> Ess."""
    x = np.asarray(x)
    assert x.ndim == 2
    S, n = x.shape
    y = x.astype(np.float64)
    y = y - y.mean(axis=0, keepdims=True)
    c0 = (y * y).sum(axis=0) / S
    varies = x.max(axis=0) > x.min(axis=0)        # (a constant series: 0 / 0, whatever the mean's rounding leaves of it)
    live = np.flatnonzero(varies)
    cut = np.zeros(n, np.int64)
    total = np.full(n, np.nan)
    total[live] = 1.0
    rows = [np.where(varies, 1.0, np.nan)]
    k = 1
    while live.size:
        if k == S:
            cut[live] = S
            break
        row = np.full(n, np.nan)
        r = (y[:S - k, live] * y[k:, live]).sum(axis=0) / (S - k) / c0[live]
        row[live] = r
        rows.append(row)
        neg = r < 0.0
        cut[live[neg]] = k
        live = live[~neg]
        total[live] += (S - k) / S * r[~neg]
        k += 1
    rho = np.stack(rows)
    tau = -1.0 + 2.0 * total
    sens = np.full(n, np.nan)
    for i in np.flatnonzero(~np.isnan(tau)):
        c = cut[i]
        s = 2.0 * (S - c + 1) / S * rho[c - 1, i]
        if c < S:
            s = min(s, 2.0 * (S - c) / S * abs(rho[c, i]))
        sens[i] = s / tau[i]
    with np.errstate(divide="ignore", invalid="ignore"):
        return Ess(S / tau, tau, cut, rho, sens)
