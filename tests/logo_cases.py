"""The synthetic cases of the group log-likelihood (csrc/logo.hip), shared by tests/test_logo_host.py (the self-check of the
reference) and tests/test_gpu_logo.py: test_gpu_ppc's make_table and test_gpu_ppc_groups's make_groups, with a synthetic
site table.  The grouped part -- G elements, one per group -- sits behind two parent elements: element 0 and 1 are the
parents its loc and its log-scale read (both terms of either chain are in use), the part is [2, 2 + G); with D = 1 the part is
element 0, G = 1, and loc0 and log_scale0 are constants.  The table is make_table's with the FIRST term of every grouped
observation pointed at its group's element (weight: the slope) and every other index, the scale's included, moved off the
part -- the leaf rule of diagnostics.marginal_selection.

far: every group's element is recorded FIVE prior standard deviations above its loc, t0 = loc + 5 exp(sj), at every draw,
and the data lie where such a state predicts them (y = the draws' median eta + N(0, 1.5^2)): the point of the centred form.
Computed once and shared, never written to."""
import collections
import functools

import numpy as np

import ppc_ref as pp
from test_gpu_ppc import make_table
from test_gpu_ppc_groups import make_groups

# (kind, D, T, N, S, C, G, layout, bad draws, random slopes, log of the part's prior scale, far)
CASES = ((pp.NORMAL, 1, 1, 7, 1, 1, 1, "all", False, False, 0.0, False),
         (pp.NORMAL, 88, 3, 64, 1, 64, 9, "holes", False, True, 0.0, False),
         (pp.NORMAL, 255, 3, 33, 5, 13, 5, "full", True, True, 6.0, True),
         (pp.NORMAL, 88, 1, 64, 26, 5, 4, "full", True, False, -6.0, False),
         (pp.NORMAL, 88, 3, 40, 1, 65, 5, "full", False, True, 0.0, True),
         (pp.NORMAL, 255, 1, 9, 1, 64, 1, "all", False, True, 6.0, False),
         (pp.BERNOULLI, 1, 1, 5, 1, 64, 1, "all", False, False, 0.0, False),
         (pp.BERNOULLI, 88, 3, 64, 26, 5, 9, "holes", True, True, 0.0, False),
         (pp.BERNOULLI, 255, 1, 40, 5, 13, 5, "full", False, False, 0.0, False))
IDS = ["%s-D%d-T%d-N%d-R%dx%d-G%d-%s%s%s-sj%g%s" % ((("normal", "bernoulli")[c[0]],) + c[1:8] + (
    "-bad" if c[8] else "", "-slopes" if c[9] else "", c[10], "-far" if c[11] else "")) for c in CASES]
NORMAL_CASES = [i for i, c in enumerate(CASES) if c[0] == pp.NORMAL]
SiteTable = collections.namedtuple("SiteTable", ("form", "loc_idx", "loc_w", "loc0", "scale_idx", "scale_w", "log_scale0", "norm",
                                                 "part"))          # models.SiteTable's fields
Case = collections.namedtuple("Case", ["table", "x3", "group_of", "slope", "elem", "site", "G"])


def part_of(D, G):
    """(lo, hi) of the grouped part in a state of D elements."""
    if D == 1:
        assert G == 1
        return 0, 1
    assert D >= 2 * G + 2
    return 2, 2 + G


def make_site(D, G, log_sj, seed):
    """The site table, float columns as float32: the part's rows read the parents 0 and 1; every other row is a constant."""
    rs = np.random.RandomState(seed)
    lo, hi = part_of(D, G)
    form, part = np.zeros(D, np.int32), np.zeros(D, np.int32)
    loc_idx, scale_idx = np.zeros((D, 2), np.int32), np.zeros((D, 2), np.int32)
    loc_w, scale_w = np.zeros((D, 2), np.float32), np.zeros((D, 2), np.float32)
    loc0, log_scale0 = (0.3 * rs.randn(D)).astype(np.float32), (0.1 * rs.randn(D)).astype(np.float32)
    log_scale0[lo:hi] += np.float32(log_sj)
    part[lo:hi] = 1
    if D > 1:
        loc_idx[lo:hi], scale_idx[lo:hi] = (0, 1), (1, 0)
        loc_w[lo:hi] = np.stack([1.0 + 0.2 * rs.randn(G), 0.25 * rs.randn(G)], axis=1)
        # (a wide prior: its log-scale barely moves with the parents, or exp(sj) -- and t0 of a `far` case -- would jump by tens)
        scale_w[lo:hi] = np.stack([0.02 * rs.randn(G), 0.01 * rs.randn(G)], axis=1) * np.exp(-max(log_sj, 0.0))
    return SiteTable(form, loc_idx, loc_w, loc0, scale_idx, scale_w, log_scale0, np.zeros(D, np.float32), part)


def ground(table, group_of, D, G, random_slopes, seed):
    """(table, slope [N] float32): make_table's table with the grouped part as its leaf."""
    rs = np.random.RandomState(seed)
    lo, hi = part_of(D, G)
    idx, w, si = table.idx.copy(), table.w.copy(), table.scale_idx.copy()
    N = idx.shape[0]
    slope = np.zeros(N, np.float32)
    if D == 1:
        si[:] = -1
    else:
        inside = (idx >= lo) & (idx < hi)
        idx[inside] += G                                           # (D >= 2 G + 2: still inside the state, outside the part)
        si[(si >= lo) & (si < hi)] += G
    grouped = group_of >= 0
    slope[grouped] = (2.0 * rs.rand(int(grouped.sum())) + 0.01).astype(np.float32) if random_slopes else 1.0
    idx[grouped, 0] = lo + group_of[grouped]
    w[grouped, 0] = slope[grouped]
    if D == 1:
        assert grouped.all() and idx.shape[1] == 1
    return table._replace(idx=idx, w=w, scale_idx=si), slope


@functools.lru_cache(maxsize=None)
def case(i):
    kind, D, T, N, S, Cn, G, layout, bad, random_slopes, log_sj, far = CASES[i]
    seed = 9000 + 17 * i
    group_of = make_groups(N, G, layout, seed + 2)
    table, slope = ground(make_table(N, T, D, kind, seed), group_of, D, G, random_slopes, seed + 3)
    site = make_site(D, G, log_sj, seed + 4)
    lo, hi = part_of(D, G)
    rs = np.random.RandomState(seed + 1)
    x3 = (0.5 * rs.randn(S, Cn, D)).astype(np.float32)
    if far:
        x = x3.reshape(-1, D).astype(np.float64)
        chain = lambda c0, ix, wt: c0[lo:hi].astype(np.float64)[None, :] + (wt[lo:hi].astype(np.float64)[None] * x[:, ix[lo:hi]]).sum(axis=2)
        loc, sj = chain(site.loc0, site.loc_idx, site.loc_w), chain(site.log_scale0, site.scale_idx, site.scale_w)
        x3.reshape(-1, D)[:, lo:hi] = (loc + 5.0 * np.exp(sj)).astype(np.float32)
        x = x3.reshape(-1, D).astype(np.float64)
        eta = (table.w.astype(np.float64)[:, :, None] * x.T[table.idx]).sum(axis=1)
        table = table._replace(y=(np.median(eta, axis=1) + 1.5 * rs.randn(N)).astype(np.float32))
    if bad:
        x3[0, 3, D // 2] = np.nan
        x3[S - 1, Cn - 1, 0] = np.inf
    for a in (x3, group_of, slope):
        a.setflags(write=False)
    return Case(table, x3, group_of, slope, np.arange(lo, hi, dtype=np.int32), site, G)
