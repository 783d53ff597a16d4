"""Inputs for the single-chain ESS kernels (csrc/ess.hip, csrc/ess_tail.h) that put every series' cut -- the first lag with
a negative auto-correlation -- at a CHOSEN lag K, so that a test can say which stage of the kernel took which lag and a
lag dropped or counted twice at a hand-over between stages cannot pass.

Families (offset 100, amplitude 3; float32):
    comb(S, K, seed)   cos(2 pi (t + phi) / 8K) + sqrt(0.6) (e_t - e_{t-K}), e white: the slow cosine keeps every lag below K
                       clearly positive, the comb term drives lag K clearly negative (rho[K-1] ~ +0.2, rho[K] ~ -0.15)
    wave(S, K, seed)   cos(2 pi (t + phi) / (4K - 2)) + 0.05 e_t: for short S, where the comb's noise decides the cut
    noise(S, K, seed)  white: the few samples of S <= 3

Seeds are chosen on the CPU: series number `slot` of a case takes the first seed of its own pool of 64 (64 slot .. 64 slot
+ 63) for which the float64 yardstick (tests/ess_direct_ref.py) cuts at exactly K with

    sens >= 4 x allowance,    allowance = (2 cut + 3) 3e-5 / tau   (relative, on the ESS)

i.e. moving the cut by one lag either way moves the ESS by at least four times what a test allows: no series is excused.
`pick` raises where a pool has no such seed; tests/test_ess_routes_host.py asserts both conditions again on the finished
traces.  Pairs (S, K) no pool of 64 reached and that are therefore absent:
    S = 33, K = 17 (cooperative tail, no dense pass possible) -- neither wave nor comb cuts past lag 16 at S = 33;
    S = 16, 17, 18 with K >= 8 -- the short cases cut at lags 1 .. 5.

Every case states its ROUTE as predicates of the yardstick (`expect`, checked against `plan`, which restates the
kernel's decisions from the yardstick's cuts); the kernel is not instrumented.

Hand-overs covered (last lag of one stage / first of the next): 16/17 (sweep 1), 48/49 (dense), 80/81 and 112/113
(cooperative rounds of 64 from 16 and 48), 32/33, 64/65 and 80/81 (far passes of 16), and for the matrix-core tail both
the lags where the host's chunks of 256 would end (272/273 from 16, 304/305 from 48) and where its rounds DO end: a
round started at lag0 completes lags lag0 - 15 .. lag0 + 240, so the first round ends at 256/257 (from 16) and 288/289
(from 48).
"""
import collections
import functools

import numpy as np

import ess_direct_ref

RHO_TOL = 3e-5          # the project's float32 element tolerance
POOL = 64
OFFSET, AMP = 100.0, 3.0

# the kernel's constants (csrc/ess.hip, csrc/ess_tail.h)
W, DENSE_LAGS, DENSE_ABOVE, LDS_FLOATS = 16, 32, 3, 36 * 64


def comb(S, K, seed):
    rs = np.random.RandomState(seed)
    phi = rs.uniform(0, 8 * K)
    e = rs.randn(S + K)
    t = np.arange(S)
    return (OFFSET + AMP * (np.cos(2 * np.pi * (t + phi) / (8 * K)) + np.sqrt(0.6) * (e[K:] - e[:S]))).astype(np.float32)


def wave(S, K, seed):
    rs = np.random.RandomState(seed)
    phi = rs.uniform(0, 4 * K - 2)
    e = rs.randn(S)
    t = np.arange(S)
    return (OFFSET + AMP * (np.cos(2 * np.pi * (t + phi) / (4 * K - 2)) + 0.05 * e)).astype(np.float32)


def noise(S, K, seed):
    return (OFFSET + AMP * np.random.RandomState(seed).randn(S)).astype(np.float32)


def lifted(S, K, seed):
    """comb with its first 16 samples lifted by 30 standard deviations: the reference level of the kernel's first sweep
    (the mean of the first 16 samples) sits ~ 30 sd from the mean and the sweep is retaken."""
    x = comb(S, K, seed)
    x[:16] += np.float32(30.0 * x.astype(np.float64).std())
    return x


def allowance_rel(ref):
    """|ESS - ESS64| / ESS64 allowed, per series."""
    return (2 * ref.cut + 3) * RHO_TOL / ref.tau


def qualifies(ref, K):
    return (ref.cut == K) & (ref.sens >= 4.0 * allowance_rel(ref))


@functools.lru_cache(maxsize=None)
def pick(family, S, K, slot):
    """The series of `slot`: the first seed of its pool that cuts at K with the margin."""
    step = 8 if S <= 20000 else 2        # (seeds tried together: a long series costs O(S K) each)
    for s0 in range(0, POOL, step):
        seeds = [POOL * slot + s0 + j for j in range(step)]
        X = np.stack([family(S, K, s) for s in seeds], axis=1)
        ok = np.flatnonzero(qualifies(ess_direct_ref.ess(X), K))
        if ok.size:
            return X[:, ok[0]]
    raise AssertionError("%s(S=%d, K=%d): no seed of pool %d qualifies" % (family.__name__, S, K, slot))


# name: trace x [S, n] float32 (read-only); K [n] intended cut (0: a series whose ESS is nan);
# modes: how the test calls the kernel -- "plain" arp_ess, "ws" arp_ess_ws with arp_ess_workspace_bytes, "rows64"
# arp_ess_ws with a row area of exactly 64 rows; expect: route predicates (see `plan`)
Case = collections.namedtuple("Case", "name x K modes expect")
Plan = collections.namedtuple("Plan", "unfinished dense route listed")


def plan(S, n, cut, mode):
    """The kernel's decisions restated from the yardstick's cuts: per wave the number of series unfinished at lag 16 and
    whether it takes the dense pass; per series the stage that takes its LAST lag ("sweep1", "dense", "coop16", "coop48",
    "far16", "far48", "mfma16", "mfma48": the tail and the lag it starts from); the number of series listed for the
    matrix-core tail."""
    waves = (n + 63) // 64
    go = (cut > W) & (S > W)
    unfinished = [int(go[64 * w:64 * w + 64].sum()) for w in range(waves)]          # (shadow lanes are not series)
    dense = [u > DENSE_ABOVE and S > W + DENSE_LAGS for u in unfinished]
    tail = "coop" if S + 72 <= LDS_FLOATS else ("far" if mode == "plain" else "mfma")
    route = []
    for i in range(n):
        d = dense[i // 64]
        if not go[i]:
            route.append("sweep1")
        elif d and cut[i] <= W + DENSE_LAGS:
            route.append("dense")
        else:
            route.append("%s%d" % (tail, W + DENSE_LAGS if d else W))
    listed = sum(r.startswith("mfma") for r in route)
    return Plan(unfinished, dense, route, listed)


FILL = (3, 15, 16)      # cuts of the series that finish in the first sweep


def _build(family, S, Ks, slot0=0):
    cols = [np.full(S, OFFSET, np.float32) if K == 0 else pick(family, S, K, slot0 + i) for i, K in enumerate(Ks)]
    x = np.stack(cols, axis=1)
    x.setflags(write=False)
    return x, np.asarray(Ks, np.int64)


def _filled(n, special):
    """n cuts: FILL in turn, `special` {index: K} on top."""
    Ks = [FILL[i % 3] for i in range(n)]
    for i, K in special.items():
        Ks[i] = K
    return Ks


def _case(name, family, S, Ks, modes, expect, slot0=0):
    x, K = _build(family, S, Ks, slot0)
    return Case(name, x, K, modes, expect)


def _short(S):
    if S == 1:      # one sample: 0 / 0 on both sides
        x = (OFFSET + AMP * np.random.RandomState(1).randn(1, 5)).astype(np.float32)
        x.setflags(write=False)
        return Case("short_S1", x, np.zeros(5, np.int64), ("plain",), dict(unfinished=[0], dense=[False]))
    if S <= 3:
        x, K = _build(noise, S, [1] * 5)
    else:
        cols = [pick(noise, S, 1, 0)] + [pick(wave, S, k, k) for k in (2, 3, 4, 5)]
        x = np.stack(cols, axis=1)
        x.setflags(write=False)
        K = np.array([1, 2, 3, 4, 5], np.int64)
    return Case("short_S%d" % S, x, K, ("plain",), dict(unfinished=[0], dense=[False]))


def _retake():
    Ks = [(3, 16, 17, 49)[i % 4] for i in range(64)]
    x, K = _build(comb, 600, Ks)
    x = x.copy()
    x[:, 21] = pick(lifted, 600, RETAKE_K, 21)
    x.setflags(write=False)
    K[21] = RETAKE_K
    u = int((K > 16).sum())
    return Case("retake", x, K, ("plain",), dict(unfinished=[u], dense=[True], retakes=[21]))


RETAKE_K = 17           # where the lifted series cuts: unfinished at lag 16, its last lag is the dense pass's first

# matrix-core tail: cuts about where the host's chunks of 256 lags would end and about where its rounds do end
MFMA_K = (271, 272, 273, 303, 304, 305)
ROUND_K = (256, 257, 288, 289)
LIMIT_K = (16, 17, 48, 49, 80, 81, 112, 113, 272, 273, 304, 305)


def _limit(S, arrangement):
    long_modes = ("plain", "ws", "rows64") if S + 72 > LDS_FLOATS else ("plain",)
    if arrangement == "dense":
        # wave 0: every cut of the list and the rounds' own ends (15 unfinished: dense, tails from 48); wave 1 (6 series):
        # 3 unfinished (tails from 16) -- both `from` values in one launch
        sp = {4 * i + 1: K for i, K in enumerate(LIMIT_K + ROUND_K)}
        sp.update({64: 80, 66: 272, 69: 305})
        return _case("limit_S%d_dense" % S, comb, S, _filled(70, sp), long_modes,
                     dict(unfinished=[15, 3], dense=[True, False]))
    three = {"a": ((17, 81, 273), (49, 113, 305)), "b": ((48, 112, 304), (80, 272, 17)),
             "c": ((256, 257, 288), (289, 257, 256))}[arrangement]
    sp = {5: three[0][0], 30: three[0][1], 63: three[0][2], 64: three[1][0], 66: three[1][1], 69: three[1][2]}
    return _case("limit_S%d_sparse_%s" % (S, arrangement), comb, S, _filled(70, sp), long_modes,
                 dict(unfinished=[3, 3], dense=[False, False]), slot0=100)


def _far():
    sp = {2: 32, 33: 33, 60: 64, 64: 65, 100: 33, 127: 64, 128: 80, 129: 81, 131: 49, 133: 48}
    return _case("far_S2233", comb, 2233, _filled(134, sp), ("plain",),
                 dict(unfinished=[3, 3, 4], dense=[False, False, True]), slot0=200)


def _mfma(S):
    sp = {7 * i + 3: K for i, K in enumerate(MFMA_K)}                         # wave 0: dense, from 48
    sp.update({64: 271, 90: 272, 127: 273, 128: 303, 130: 304, 133: 305})       # waves 1, 2: from 16
    return _case("mfma_S%d" % S, comb, S, _filled(134, sp), ("ws",),
                 dict(unfinished=[6, 3, 3], dense=[True, False, False], listed=12), slot0=300)


def _chunks(listed):
    # wave 0: all 64 series past the dense pass (listed from 48); wave 1: one more from 16, or none
    Ks = [(49, 80, 81, 112, 113) [i % 5] if i % 8 else (MFMA_K + ROUND_K)[(i // 8) % 10] for i in range(64)]
    Ks += _filled(64, {40: 273} if listed == 65 else {})
    return _case("chunks_%d" % listed, comb, 2233, Ks, ("ws", "rows64"),
                 dict(unfinished=[64, listed - 64], dense=[True, False], listed=listed), slot0=500)


def _inner():
    # the 64 series of chains 3 .. 10 of a [S, 16, 8] trace (tests take the block in place)
    sp = {8 * i + 2: K for i, K in enumerate((17, 49, 81, 113, 257, 273, 289, 305))}
    return _case("inner_S2233", comb, 2233, _filled(64, sp), ("ws",),
                 dict(unfinished=[8], dense=[True], listed=7), slot0=700)


def _shadow(n):
    waves = (n + 63) // 64
    return _case("shadow_n%d" % n, comb, 600, _filled(n, {n - 1: 81}), ("plain",),
                 dict(unfinished=[0] * (waves - 1) + [1], dense=[False] * waves))


BUILDERS = {
    **{"short_S%d" % S: functools.partial(_short, S) for S in (1, 2, 3, 16, 17, 18)},
    # cooperative tail where no dense pass is possible: all 64 series of the wave unfinished at lag 16
    "coop_nodense_S48": lambda: _case("coop_nodense_S48", wave, 48, [17] * 64, ("plain",),
                                      dict(unfinished=[64], dense=[False])),
    # the dense guard S > 48: four unfinished series, cut at 17
    **{"dense_guard_S%d" % S: functools.partial(
        lambda S: _case("dense_guard_S%d" % S, wave, S, _filled(64, {0: 17, 21: 17, 42: 17, 63: 17}), ("plain",),
                        dict(unfinished=[4], dense=[S > 48])), S) for S in (48, 49)},
    # the 3 / 4 vote: wave 0 has exactly 3 unfinished series (cooperative tail from 16, across its first round's end at
    # 80), wave 1 exactly 4 (dense, then the cooperative tail from 48 across its round end at 112)
    "dense_vote": lambda: _case("dense_vote", comb, 600,
                                _filled(128, {9: 17, 31: 80, 63: 81, 64: 17, 77: 48, 100: 49, 127: 113}), ("plain",),
                                dict(unfinished=[3, 4], dense=[False, True])),
    # shadow lanes: the last series is the only unfinished one of its wave
    **{"shadow_n%d" % n: functools.partial(_shadow, n) for n in (1, 63, 65, 257)},
    "retake": _retake,
    # cuts at the ends of 16-lag rounds (the one-pass tile kernel's hand-overs 16/17, 32/33, 48/49), an odd series count
    "rounds16": lambda: _case("rounds16", comb, 600, _filled(67, {5: 17, 9: 32, 20: 33, 33: 48, 40: 49, 63: 33, 64: 32,
                                                                  66: 33}), ("plain",),
                              dict(unfinished=[6, 2], dense=[True, False]), slot0=900),
    **{"limit_S%d_%s" % (S, a if a == "dense" else "sparse_" + a): functools.partial(_limit, S, a)
       for S in (2232, 2233) for a in ("dense", "a", "b", "c")},
    "far_S2233": _far,
    **{"mfma_S%d" % S: functools.partial(_mfma, S) for S in (2233, 2240, 2304, 2305)},
    "chunks_64": functools.partial(_chunks, 64),
    "chunks_65": functools.partial(_chunks, 65),
    "inner_S2233": _inner,
    # past a fold of the matrix-core tail's float accumulators (every 65 536 samples)
    "fold_S65600": lambda: _case("fold_S65600", comb, 65600, [305] * 4, ("ws",),
                                 dict(unfinished=[4], dense=[True], listed=4), slot0=800),
}
NAMES = tuple(BUILDERS)
# the short cases the one-pass tile kernel serves as well (32 <= S <= 1 024, at least two series)
TILE_NAMES = ("coop_nodense_S48", "dense_guard_S48", "dense_guard_S49", "dense_vote", "shadow_n63", "shadow_n65",
              "shadow_n257", "retake", "rounds16")


@functools.lru_cache(maxsize=None)
def case(name):
    """(Case, yardstick) -- computed once, shared, never modified."""
    c = BUILDERS[name]()
    assert c.name == name and c.x.dtype == np.float32 and not c.x.flags.writeable
    return c, ess_direct_ref.ess(c.x)


def retake_predicate(x):
    """m^2 > 16 of the kernel's first attempt, per series, with its formula for the reference level r (float32: the first
    sample plus the mean difference of the first 16 samples to it)."""
    S = x.shape[0]
    nh = min(S, W)
    d = np.zeros(x.shape[1], np.float32)
    for j in range(1, nh):
        d = d + (x[j] - x[0])
    r = x[0] + d / np.float32(nh)
    y = x.astype(np.float64) - r.astype(np.float64)
    mp = y.mean(axis=0)
    c0 = (y * y).mean(axis=0) - mp * mp
    return mp * mp > 16.0 * c0, r
