"""float64 numpy / scipy restatement of the rank-normalised, folded split R-hat (Vehtari, Gelman, Simpson, Carpenter,
Buerkner 2021) and of the pooled order statistics -- TEST YARDSTICK: written from the formulas, shares no code with
autoreparam_amd/diagnostics.py or csrc/rank.hip.

Pool of element d: its N = S C values.  rank2 = #{v' < v} + #{v' <= v} = 2 (average 1-based rank) - 1 (two searchsorted
calls on the sorted pool).  p = (4 rank2 + 1) / (8 N + 2) = (r - 3/8) / (N + 1/4), z = Phi^-1(p) (scipy.special.ndtri in
float64; the upper half as -Phi^-1(1 - p) with 1 - p = (8 N + 1 - 4 rank2) / (8 N + 2) from the integers).  Folded:
v = |x - median| in float32, median = 0.5f (x_(floor((N+1)/2)) + x_(ceil((N+1)/2))) in float32.  Quantile: x_(k),
k = clamp(ceil(p N), 1, N) in float64.  The statistic: rhat_ref.rhat on the z trace, split, all S rows ranked.
"""
import numpy as np
from scipy.special import ndtri

import rhat_ref


def pools(x):
    """[S, C, D] float32 -> [D, N] float32, every element's pooled draws in (s, c) order."""
    x = np.asarray(x, np.float32)
    return np.ascontiguousarray(x.reshape(-1, x.shape[-1]).T)


def median(x):
    """[D] float32."""
    p = np.sort(pools(x), axis=1)
    N = p.shape[1]
    return np.float32(0.5) * (p[:, (N + 1) // 2 - 1] + p[:, (N + 2) // 2 - 1])


def quantiles(x, probs):
    """[len(probs), D] float32: order statistics, no interpolation."""
    p = np.sort(pools(x), axis=1)
    N = p.shape[1]
    ks = [int(min(max(np.ceil(np.float64(q) * np.float64(N)), 1), N)) for q in probs]
    return np.stack([p[:, k - 1] for k in ks])


def folded(x):
    """|x - median| in float32, [S, C, D]."""
    x = np.asarray(x, np.float32)
    return np.abs(x - median(x)[None, None, :]).astype(np.float32)


def rank2(v):
    """[S, C, D] uint32 of the values v [S, C, D] float32 (already folded, if folding is wanted)."""
    v = np.asarray(v, np.float32) + np.float32(0.0)                       # (-0 + 0 = +0: the zeros tie either way)
    out = np.empty(v.shape, np.uint32)
    for d in range(v.shape[-1]):
        col = v[..., d].reshape(-1)
        order = np.argsort(col, kind="stable")                            # (the needles in order: a pool of 2^21 draws
        srt = col[order]                                                  # is searched in a fraction of the time)
        r = np.empty(col.size, np.int64)
        r[order] = np.searchsorted(srt, srt, side="left") + np.searchsorted(srt, srt, side="right")
        out[..., d] = r.reshape(v.shape[:-1])
    return out


def z_scores(r2, N):
    """float64 normal scores of rank2 among N."""
    a = 4 * r2.astype(np.int64) + 1
    den = 8 * int(N) + 2
    b = den - a
    lower = a <= b
    with np.errstate(all="ignore"):
        z = np.where(lower, ndtri(np.minimum(a, b) / np.float64(den)), -ndtri(np.minimum(a, b) / np.float64(den)))
    return np.where(a == b, 0.0, z)


def rank_rhat(x):
    """dict of [D] float64: bulk, tail, rhat = fmax, median, q05, q95 -- and the two float64 z traces [S, C, D] with the
    rank2 [S, C, D] uint32 they come from."""
    x = np.asarray(x, np.float32)
    N = x.shape[0] * x.shape[1]
    rb, rt = rank2(x), rank2(folded(x))
    zb, zt = z_scores(rb, N), z_scores(rt, N)
    bulk, tail = rhat_ref.rhat(zb, True)[0], rhat_ref.rhat(zt, True)[0]
    q = quantiles(x, (0.05, 0.95)).astype(np.float64)
    return dict(bulk=bulk, tail=tail, rhat=np.fmax(bulk, tail), median=median(x).astype(np.float64), q05=q[0], q95=q[1],
                z_bulk=zb, z_tail=zt, rank2_bulk=rb, rank2_tail=rt)


def table_input(seed, S=400, Cn=64):
    """The three elements of the issue's table: N(0,1); N(0,1) with chains :16 at 3 x the scale; standard Cauchy with
    chains :16 shifted by +2."""
    rs = np.random.RandomState(seed)
    x = rs.randn(S, Cn, 3)
    x[:, :16, 1] *= 3.0
    x[:, :, 2] = rs.standard_cauchy((S, Cn))
    x[:, :16, 2] += 2.0
    return x.astype(np.float32)
