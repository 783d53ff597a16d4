"""A numpy float64 restatement of arp_sbc_fold (include/autoreparam.h), for the tests: counts by comparison, sums by
math.fsum (correctly rounded sums of the float64 terms the kernel adds), and the left-out rule.  Nothing here is shared
with the kernel or with diagnostics.sbc_summary."""
import math

import numpy as np


def fold(draws, truth):
    """draws [N, L, Q], truth [N, Q] (anything numpy reads; the values are taken as float32) -> dict of
    counts [N, Q, 2] int64 = (#{x < t}, #{x == t}); sums [N, Q, 2] float64 = (fsum (x - t), fsum (x - t)^2), every term
    rounded to float64 once as the kernel rounds it; abs_terms [N, Q, 2] = (fsum |x - t|, fsum (x - t)^2), what the bound of
    recursive summation is a multiple of; left_out [N] uint8 (a non-finite truth or draw: counts and sums 0);
    n_left_out int."""
    x = np.asarray(draws, np.float32).astype(np.float64)
    t = np.asarray(truth, np.float32).astype(np.float64)
    N, L, Q = x.shape
    assert t.shape == (N, Q)
    counts = np.zeros((N, Q, 2), np.int64)
    sums, abs_terms = np.zeros((N, Q, 2)), np.zeros((N, Q, 2))
    left_out = np.zeros(N, np.uint8)
    for r in range(N):
        if not (np.isfinite(x[r]).all() and np.isfinite(t[r]).all()):
            left_out[r] = 1
            continue
        d = x[r] - t[r][None, :]                                 # one float64 subtraction per term
        sq = d * d                                               # one float64 product per term
        counts[r, :, 0] = np.sum(d < 0, axis=0)
        counts[r, :, 1] = np.sum(d == 0, axis=0)
        for q in range(Q):
            sums[r, q, 0] = math.fsum(d[:, q])
            sums[r, q, 1] = math.fsum(sq[:, q])
            abs_terms[r, q, 0] = math.fsum(np.abs(d[:, q]))
            abs_terms[r, q, 1] = sums[r, q, 1]
    return {"counts": counts, "sums": sums, "abs_terms": abs_terms, "left_out": left_out, "n_left_out": int(left_out.sum())}


def sum_bound(n_draws, abs_terms):
    """n 2^-53 sum |term|: the bound of recursive summation of n terms in any order against their exact sum (Higham,
    Accuracy and Stability of Numerical Algorithms, 4.2: (n - 1) u to first order, u = 2^-53), with fsum's own half ulp of
    the result inside the spare term.  Not a measured tolerance."""
    return float(n_draws) * 2.0 ** -53 * np.asarray(abs_terms, np.float64)
