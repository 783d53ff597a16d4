"""NumPy restatement of the in-kernel streaming statistics (arp_hmc_io.stats, the six [6][C][D] planes) -- TEST
YARDSTICK: written from the formulas, shares no code with autoreparam_amd/engine.py, inference.StreamingStats or the
kernels.

float64 part (`summary`): per (chain, element) of a [S, C, D] trace the mean, the unbiased variance and the batch-means
ESS = n var / (batch var(batch means)) over the COMPLETE batches only, capped at n.

float32 part: the two recurrences the kernels run, restated sample by sample in float32 (vectorised over [C, D] only),
each returning the six planes {ref, s1, s2, cur, sb1, sb2} of include/autoreparam.h:

  ref    a level near the samples.  The first recorded sample (or the mean of the first stretch folded) until the first
         batch ends; at the batch ends that complete 1, 2, 4, 8, ... batches it MOVES to the mean of the samples so far
         and every sum moves with it -- the squared offset cancels a few times per run instead of once per sample
  s1     sum of (x - ref)
  s2     sum of (x - ref)^2
  cur    s1 as it was when the current batch began
  sb1    sum of the batch means (of x - ref)
  sb2    sum of their squares

  mean = ref + s1 / n,  var = (s2 - s1^2 / n) / (n - 1),  var(batch means) = (sb2 - sb1^2 / nb) / (nb - 1).

`per_sample_planes` is kernels.h: stats_update_staged (three planes touched per sample), `welford_fold_planes` is
pk_chain.h: pk_stats_accumulate / pk_stats_fold with kernels.h: stats_fold_staged (Welford within a batch in LDS, the planes
touched when a batch or a launch ends); both call `_reref` (kernels.h: stats_reref_staged) after every batch end, which acts at
those batch counts.  Fused multiply-adds are restated as the float32 rounding of the float64 result (the product of two float32
is exact in float64), so on the same samples the per-sample restatement follows the device operation by operation.
`reref=False` gives the recurrences without that step, as they were: what the step is worth on a given trace.
"""
import numpy as np

f32 = np.float32


def summary(trace, batch):
    """(mean, var, ess) float64 [C, D] of a [S, C, D] trace."""
    x = np.asarray(trace, np.float64)
    n = x.shape[0]
    nb = n // batch
    if nb < 2:
        raise ValueError("batch-means ESS needs at least two complete batches")
    mean = x.mean(axis=0)
    var = x.var(axis=0, ddof=1)
    bm = x[:nb * batch].reshape((nb, batch) + x.shape[1:]).mean(axis=1)
    vb = bm.var(axis=0, ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = np.minimum(n * var / (batch * vb), float(n))
    return mean, var, ess


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _batch_end(P, batch):
    """sb1 += bm, sb2 += bm^2, cur = s1 with bm = (s1 - cur) / batch: both routes, every batch end"""
    ref, s1, s2, cur, sb1, sb2 = P
    bm = (s1 - cur) * (f32(1) / f32(batch))
    sb1 += bm
    sb2[...] = _fma(bm, bm, sb2)
    cur[...] = s1


def _reref(P, n, k):
    """After the batch end that completes k = 1, 2, 4, 8, ... batches (n samples): ref moves to the mean so far.  With h the
    shift ref actually takes (rounding included): s1 - n h, s2 + h (n h - 2 s1), cur = s1, sb1 - k h, sb2 + h (k h - 2 sb1)."""
    if k & (k - 1):
        return
    ref, s1, s2, cur, sb1, sb2 = P
    fn, fk = f32(n), f32(k)
    nref = _fma(s1, f32(1) / fn, ref)
    h = nref - ref
    s2[...] = _fma(h, _fma(fn, h, f32(-2) * s1), s2)
    sb2[...] = _fma(h, _fma(fk, h, f32(-2) * sb1), sb2)
    sb1[...] = _fma(-fk, h, sb1)
    s1[...] = _fma(-fn, h, s1)
    cur[...] = s1
    ref[...] = nref


def per_sample_planes(trace, batch, reref=True):
    """The plane-per-sample route in float32: [6, C, D]."""
    x = np.asarray(trace, f32)
    S = x.shape[0]
    P = np.zeros((6,) + x.shape[1:], f32)
    ref, s1, s2, cur, sb1, sb2 = P
    for r in range(S):
        if r == 0:
            ref[...] = x[0]
        dx = x[r] - ref
        s1 += dx
        s2[...] = _fma(dx, dx, s2)
        if (r + 1) % batch == 0:
            _batch_end(P, batch)
            if reref:
                _reref(P, r + 1, (r + 1) // batch)
    return P


def welford_fold_planes(trace, batch, launch_ends=(), reref=True):
    """The LDS route in float32: Welford updates of (m, M2) since the last fold, folded into the planes when a batch ends
    and after each recorded-sample count in `launch_ends` (where a launch ends): [6, C, D]."""
    x = np.asarray(trace, f32)
    S = x.shape[0]
    P = np.zeros((6,) + x.shape[1:], f32)
    ref, s1, s2, cur, sb1, sb2 = P
    ends = set(int(e) for e in launch_ends) | {S}
    m = np.zeros(x.shape[1:], f32); M2 = np.zeros(x.shape[1:], f32)
    n_acc, folded = 0, False
    for r in range(S):
        n_acc += 1
        if n_acc == 1:
            m[...] = x[r]; M2[...] = 0
        else:
            rn = f32(1) / f32(n_acc)
            d = x[r] - m
            m[...] = _fma(d, rn, m)
            M2[...] = _fma(d, x[r] - m, M2)
        bend = (r + 1) % batch == 0
        if bend or (r + 1) in ends:
            if not folded:
                ref[...] = m
                folded = True
            d = m - ref
            nd = f32(n_acc) * d
            s1 += nd
            s2 += _fma(nd, d, M2)
            if bend:
                _batch_end(P, batch)
                if reref:
                    _reref(P, r + 1, (r + 1) // batch)
            n_acc = 0
    return P


def ar1(S, C, D, rho, off, seed, mean=0.0, sd=1.0):
    """[S, C, D] float32 AR(1) series of unit-free correlation rho whose FIRST sample sits `off` standard deviations from
    the mean (where a post-burn-in draw lands routinely among many chains x elements)."""
    rs = np.random.RandomState(seed)
    z = np.zeros((S, C, D))
    z[0] = rs.randn(C, D)
    e = rs.randn(S, C, D) * np.sqrt(1 - rho * rho)
    for t in range(1, S):
        z[t] = rho * z[t - 1] + e[t]
    z[0] = off
    return (mean + sd * z).astype(f32)
