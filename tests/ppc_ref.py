"""The float64 definition of the posterior predictive check (csrc/ppc.hip, include/autoreparam.h: arp_predictive_check),
from an observation table and centred draws: Philox4x32-10 restated on Python / numpy integers (held to the Random123
known answers tests/test_rng.py quotes), the uniform and the Box-Muller normal derived in float64 from the SAME float32 u
and angle the kernel forms, y_rep, the eight per-draw columns and the four per-observation columns."""
import collections
import math

import numpy as np

NORMAL, BERNOULLI = 0, 1
LOG_2PI = math.log(2.0 * math.pi)
M32 = np.uint64(0xFFFFFFFF)
# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, output)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))

Ref = collections.namedtuple("Ref", ["eta", "s", "A", "mu", "var", "m2", "p", "u", "z", "y_rep", "pit", "dev_rep", "dev_obs",
                                     "used", "draw_stats", "obs_sums"])


def philox4x32_10(counter, key):
    """Four uint64 arrays (values < 2^32) of one shape from counter words (c0, c1, c2, c3) and key words (k0, k1), each an
    integer or an integer array: ten rounds, multipliers 0xD2511F53 / 0xCD9E8D57, key bumps 0x9E3779B9 / 0xBB67AE85."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) & M32 for c in counter])
    k0, k1 = (np.asarray(k, np.uint64) & M32 for k in key)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0                      # < 2^64: exact in uint64
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def words(n, g, seed):
    """(w0, w1) of observation(s) n and global draw number(s) g under `seed`: counter (n, lo32 g, hi32 g, 0), key
    (lo32 seed, hi32 seed)."""
    g = np.asarray(g, np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = philox4x32_10((n, g & M32, g >> np.uint64(32), 0), (seed & 0xFFFFFFFF, seed >> 32))
    return out[0], out[1]


def uniform(w0):
    """u = (w0 >> 8) 2^-24 in [0, 1): exact in float32, returned as float64."""
    return (np.asarray(w0, np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def normal_inputs(w0, w1):
    """The float32 u' in (0, 1] and angle a in [1, 2) revolutions the kernel forms, as float64: u' = fma((float)w0, 2^-32,
    2^-33) -- the conversion rounds to nearest even, the fma rounds once -- and a's mantissa is the low 23 bits of w1."""
    a0 = np.asarray(w0, np.uint64).astype(np.uint32).astype(np.float32).astype(np.float64)
    up = (a0 * 2.0 ** -32 + 2.0 ** -33).astype(np.float32).astype(np.float64)        # (the float64 sum is exact)
    a = 1.0 + (np.asarray(w1, np.uint64) & np.uint64(0x7FFFFF)).astype(np.float64) * 2.0 ** -23
    return up, a


def normal(w0, w1):
    """z = sqrt(-2 log u') cos(2 pi a) in float64."""
    up, a = normal_inputs(w0, w1)
    return np.sqrt(-2.0 * np.log(up)) * np.cos(2.0 * np.pi * (a - 1.0))


def predictor(table, x):
    """(eta, s, A) [N, R] in float64 from a table and centred states x [R, D] (float32 values): A = sum_t |w_t x_t|."""
    x = np.asarray(x, np.float64)
    w = table.w.astype(np.float64)
    xs = x[:, table.idx]                                                              # [R, N, T]
    eta = np.einsum("nt,rnt->nr", w, xs)
    A = np.einsum("nt,rnt->nr", np.abs(w), np.abs(xs))
    s = np.repeat(table.log_scale.astype(np.float64)[:, None], x.shape[0], axis=1)
    on = table.scale_idx >= 0
    s[on] += x[:, table.scale_idx[on]].T
    return eta, s, A


def softplus(e):
    return np.maximum(e, 0.0) + np.log1p(np.exp(-np.abs(e)))


def deviance(kind, v, eta, s):
    """-2 log-likelihood of the value(s) v."""
    if kind == NORMAL:
        return ((v - eta) * np.exp(-s)) ** 2 + 2.0 * s + LOG_2PI
    return -2.0 * (v * eta - softplus(eta))


def fold(kind, y, y_rep, mu, m2, pit, dev_rep, dev_obs, used):
    """(draw_stats [R, 8], obs_sums [N, 4]) in float64 from [N, R] per-(n, r) values and used [R] (False: the draw is left
    out -- a zero row, no part in obs_sums)."""
    N, R = y_rep.shape
    ds = np.stack([y_rep.sum(0), (y_rep * y_rep).sum(0), y_rep.min(0), y_rep.max(0), dev_rep.sum(0), dev_obs.sum(0), mu.sum(0),
                   np.full(R, float(N))], axis=1)
    ds[~used] = 0.0
    le = (y_rep <= np.asarray(y, np.float64)[:, None]).astype(np.float64)
    obs = np.stack([a[:, used].sum(1) for a in (mu, m2, pit, le)], axis=1)
    return ds, obs


def reference(table, x, n0=0, n1=None, seed=0, draw_offset=0):
    """Every output of arp_predictive_check for the observations [n0, n1) in float64 -> Ref ([n1 - n0, R] arrays).  A draw
    with a non-finite element is left out (its per-(n, r) values are computed from a zeroed state and never counted)."""
    x = np.asarray(x, np.float64)
    R = x.shape[0]
    N = table.idx.shape[0]
    n1 = N if n1 is None else n1
    used = np.isfinite(x).all(axis=1)
    x = np.where(used[:, None], x, 0.0)
    sub = type(table)(table.kind, table.idx[n0:n1], table.w[n0:n1], table.y[n0:n1], table.scale_idx[n0:n1], table.log_scale[n0:n1])
    eta, s, A = predictor(sub, x)
    y = sub.y.astype(np.float64)[:, None]
    w0, w1 = words(np.arange(n0, n1, dtype=np.uint64)[:, None], np.uint64(draw_offset) + np.arange(R, dtype=np.uint64)[None, :], seed)
    u, z, p = uniform(w0), None, None
    if table.kind == NORMAL:
        z = normal(w0, w1)
        mu, var = eta, np.exp(2.0 * s)
        y_rep = eta + np.exp(s) * z
        zo = (y - eta) * np.exp(-s)
        pit = 0.5 * np.vectorize(math.erfc)(-zo / math.sqrt(2.0))
    else:
        p = 1.0 / (1.0 + np.exp(-eta))
        mu, var = p, p * (1.0 - p)
        y_rep = (u < p).astype(np.float64)
        pit = np.where(y > 0.5, 1.0 - 0.5 * p, 0.5 * (1.0 - p))
    m2 = mu * mu + var
    dev_rep, dev_obs = deviance(table.kind, y_rep, eta, s), deviance(table.kind, y, eta, s)
    ds, obs = fold(table.kind, sub.y, y_rep, mu, m2, pit, dev_rep, dev_obs, used)
    return Ref(eta, s, A, mu, var, m2, p, u, z, y_rep, pit, dev_rep, dev_obs, used, ds, obs)
