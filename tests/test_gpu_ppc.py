"""GPU: arp_predictive_check (csrc/ppc.hip) through diagnostics.predictive_check against the float64 definition of
tests/ppc_ref.py: y_rep, the PIT and every column per element within twice the first-order bounds of the ppc.hip header
(evaluated per element here, as tests/test_gpu_loglik.py evaluates loglik's; nothing is fitted to the device's output),
the Bernoulli draws wherever u is outside the bound around p, the fold recomputed from the device's own y_rep, the
structural properties (two calls, split observation ranges, draw_offset, seed, y_rep = NULL), masked draws, one
statistical tie between the random and the analytic path, refusals, and the report through the CLI.

Share of Bernoulli (n, r) inside the margin |u - p| <= 2 bp over the cases below, counted from the reference alone on the
CPU when the test was written: 0 of 108 237 (by the margin's width, about 2 10^-5 of them were to be expected)."""
import collections
import ctypes as C
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

import ppc_ref as pp

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FACTOR = 2.0                 # second-order terms: twice the header's first-order figures, as for loglik.hip
F64 = 2.0 ** -52
Table = collections.namedtuple("Table", ("kind", "idx", "w", "y", "scale_idx", "log_scale"))
# (T, N, S, C): every T in {1, 3, 5, 25} (the loop is unrolled by 4), N in {1, 3, 5, 130} (fewer observations than waves, a
# ragged last round, many blockIdx.y groups at small R), R = S C in {1, 63, 64, 65, 200}
SHAPES = ((1, 1, 1, 1), (3, 3, 1, 63), (5, 5, 2, 32), (25, 130, 5, 13), (1, 130, 5, 40), (25, 1, 1, 64), (3, 130, 1, 1),
          (5, 3, 4, 50), (25, 5, 1, 65))
DIMS = (1, 9, 255)


def make_table(N, T, D, kind, seed):
    """idx hits 0 and D - 1; weights of size 3 / sqrt(T), so that eta ~ N(0, 1.5^2) at states N(0, 0.5^2); the scale latent
    set on every other observation and unset on the rest, in one table."""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, D, size=(N, T)).astype(np.int32)
    idx[0, 0], idx[-1, -1] = 0, D - 1
    w = (3.0 / math.sqrt(T) * rs.randn(N, T)).astype(np.float32)
    y = (1.5 * rs.randn(N)).astype(np.float32) if kind == pp.NORMAL else (rs.rand(N) < 0.5).astype(np.float32)
    si = np.full(N, -1, np.int32)
    si[::2] = rs.randint(0, D, size=si[::2].shape)
    return Table(kind, idx, w, y, si, (0.3 * rs.randn(N)).astype(np.float32))


def make_case(kind, D, shape):
    T, N, S, Cn = shape
    seed = 1000 * D + 37 * T + 11 * N + S * Cn + kind
    rs = np.random.RandomState(seed)
    return make_table(N, T, D, kind, seed), (0.5 * rs.randn(S, Cn, D)).astype(np.float32), seed


def run(gpu, x3, table, n0=0, n1=None, seed=0, draw_offset=0, want_y_rep=True):
    """(draw_stats [R, 8], obs_sums [n, 4], y_rep [n, R] or None, mask [R], count) on the host."""
    from autoreparam_amd import diagnostics
    xd = x3 if torch.is_tensor(x3) else torch.as_tensor(np.ascontiguousarray(x3, np.float32), device=gpu)
    dt = diagnostics.upload_table(table, int(xd.shape[2]), gpu)
    ds, obs, yr, mask, count = diagnostics.predictive_check(xd, dt, n0, n1, seed=seed, draw_offset=draw_offset, want_y_rep=want_y_rep)
    return ds.cpu().numpy(), obs.cpu().numpy(), None if yr is None else yr.cpu().numpy(), mask.cpu().numpy(), int(count.item())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}.get(a.dtype, a.dtype))


# ---- the header's bounds, per element, from float64 quantities ----
def normal_bounds(T, r, y):
    """Allowances [N, R] of y_rep, pit, dev(y_rep) (the device's y_rep within its own allowance), dev(y), mu, m2."""
    A, s, eta = r.A, r.s, r.eta
    es, ems = np.exp(s), np.exp(-s)
    b_y = U * (T * A + es * np.abs(r.z) * (26.0 + np.abs(s)) + np.abs(r.y_rep))
    zo = (y[:, None] - eta) * ems
    phi = np.exp(-0.5 * zo * zo) / math.sqrt(2.0 * math.pi)
    b_pit = U * (phi * (T * A * ems + np.abs(zo) * (10.0 + np.abs(s))) + 32.0 * r.pit) + 2.0 ** -126

    def b_dev(v, dev, dv):
        zv = (v - eta) * ems
        return U * (2.0 * T * A * ems * np.abs(zv) + zv * zv * (18.0 + 2.0 * np.abs(s)) + 4.0 * np.abs(s) + np.abs(dev) + 2.0) \
            + 2.0 * ems * np.abs(zv) * dv
    b_m2 = U * (2.0 * np.abs(eta) * T * A + eta * eta + np.exp(2.0 * s) * (14.0 + 2.0 * np.abs(s)) + r.m2)
    return b_y, b_pit, b_dev(r.y_rep, r.dev_rep, FACTOR * b_y), b_dev(y[:, None], r.dev_obs, 0.0), T * U * A, b_m2, b_dev


def bernoulli_bounds(T, r, y):
    """Allowances [N, R] of p, pit, m2 and a function for dev(v)."""
    A, eta, p = r.A, r.eta, r.p
    bp = U * (p * (1.0 - p) * (T * A + 6.0) + 2.0 * p)
    sp = pp.softplus(eta)

    def b_dev(v):
        return 2.0 * U * (T * A * (np.abs(v) + 1.0) + np.abs(v * eta) + 8.0 + sp + np.abs(v * eta - sp))
    return bp, 0.5 * bp + U, 3.0 * bp + 4.0 * U, b_dev


def sums_close(got, ref, allow, terms, what):
    """A float64 sum of float32 values against the reference's: the values' own allowances added up, plus the float64
    association of `terms` [n] values of the given magnitude."""
    slack = FACTOR * allow + 4.0 * F64 * terms
    assert np.all(np.abs(got - ref) <= slack), (what, float(np.max(np.abs(got - ref) / np.maximum(slack, 1e-300))))


def check_normal(gpu, table, x3, seed, n0=0, n1=None, draw_offset=0, what=""):
    S, Cn, D = x3.shape
    N, T = table.idx.shape
    n1 = N if n1 is None else n1
    x = np.asarray(x3, np.float32).reshape(S * Cn, D)
    r = pp.reference(table, x, n0, n1, seed, draw_offset)
    y = table.y[n0:n1].astype(np.float64)
    ds, obs, yr, mask, count = run(gpu, x3, table, n0, n1, seed, draw_offset)
    assert count == 0 and not mask.any() and np.isfinite(ds).all() and np.isfinite(obs).all() and np.isfinite(yr).all(), what
    b_y, b_pit, b_dr, b_do, b_mu, b_m2, _ = normal_bounds(T, r, y)
    n = n1 - n0
    # per element: y_rep
    dev = np.abs(yr.astype(np.float64) - r.y_rep)
    assert np.all(dev <= FACTOR * b_y), (what, "y_rep", float((dev / b_y).max()))
    # the draw columns (sums over the observations)
    sums_close(ds[:, 0], r.draw_stats[:, 0], b_y.sum(0), n * np.abs(r.y_rep).sum(0), (what, "sum y_rep"))
    sums_close(ds[:, 1], r.draw_stats[:, 1], (2.0 * np.abs(r.y_rep) * b_y).sum(0) * 1.01, n * (r.y_rep ** 2).sum(0), (what, "sum y_rep^2"))
    assert np.all(np.abs(ds[:, 2] - r.draw_stats[:, 2]) <= FACTOR * b_y.max(0)) and np.all(np.abs(ds[:, 3] - r.draw_stats[:, 3]) <= FACTOR * b_y.max(0)), what
    assert np.array_equal(ds[:, 2], yr.min(0).astype(np.float64)) and np.array_equal(ds[:, 3], yr.max(0).astype(np.float64)), what
    sums_close(ds[:, 4], r.draw_stats[:, 4], b_dr.sum(0), n * np.abs(r.dev_rep).sum(0), (what, "deviance rep"))
    sums_close(ds[:, 5], r.draw_stats[:, 5], b_do.sum(0), n * np.abs(r.dev_obs).sum(0), (what, "deviance obs"))
    sums_close(ds[:, 6], r.draw_stats[:, 6], b_mu.sum(0), n * np.abs(r.mu).sum(0), (what, "sum mu"))
    assert np.array_equal(ds[:, 7], np.full(S * Cn, float(n))), what
    # the observation columns (sums over the draws; R = 1: per element)
    R = S * Cn
    sums_close(obs[:, 0], r.obs_sums[:, 0], b_mu.sum(1), R * np.abs(r.mu).sum(1), (what, "obs mu"))
    sums_close(obs[:, 1], r.obs_sums[:, 1], b_m2.sum(1), R * r.m2.sum(1), (what, "obs m2"))
    sums_close(obs[:, 2], r.obs_sums[:, 2], b_pit.sum(1), R * r.pit.sum(1), (what, "obs pit"))
    near = (np.abs(r.y_rep - y[:, None]) <= FACTOR * b_y).sum(1)          # an indicator may only differ at a near tie
    assert np.all(np.abs(obs[:, 3] - r.obs_sums[:, 3]) <= near), what
    assert np.array_equal(obs[:, 3], (yr <= table.y[n0:n1, None]).sum(1).astype(np.float64)), what
    return r, ds, obs, yr


def margin(T, r):
    """(inside [N, R], bp): where |u - p| is within the allowance around p -- from the reference alone."""
    bp = bernoulli_bounds(T, r, None)[0]
    return np.abs(r.u - r.p) <= FACTOR * bp, bp


def check_bernoulli(gpu, table, x3, seed, what=""):
    S, Cn, D = x3.shape
    N, T = table.idx.shape
    x = np.asarray(x3, np.float32).reshape(S * Cn, D)
    r = pp.reference(table, x, 0, N, seed, 0)
    y = table.y.astype(np.float64)
    assert r.A.max() <= 30.0, what
    inside, bp = margin(T, r)                                            # before the device is consulted
    assert inside.sum() <= 0.01 * inside.size, (what, int(inside.sum()), inside.size)
    ds, obs, yr, mask, count = run(gpu, x3, table, 0, N, seed, 0)
    assert count == 0 and not mask.any() and np.isfinite(ds).all() and np.isfinite(obs).all(), what
    assert set(np.unique(yr)) <= {0.0, 1.0}, what
    wrong = (yr.astype(np.float64) != r.y_rep) & ~inside
    assert not wrong.any(), (what, int(wrong.sum()))
    _, b_pit, b_m2, b_dev = bernoulli_bounds(T, r, y)
    R = S * Cn
    sums_close(ds[:, 5], r.draw_stats[:, 5], b_dev(y[:, None]).sum(0), N * np.abs(r.dev_obs).sum(0), (what, "deviance obs"))
    sums_close(ds[:, 6], r.draw_stats[:, 6], bp.sum(0), N * r.mu.sum(0), (what, "sum mu"))
    assert np.array_equal(ds[:, 7], np.full(R, float(N))), what
    sums_close(obs[:, 0], r.obs_sums[:, 0], bp.sum(1), R * r.mu.sum(1), (what, "obs mu"))
    sums_close(obs[:, 1], r.obs_sums[:, 1], b_m2.sum(1), R * r.m2.sum(1), (what, "obs m2"))
    sums_close(obs[:, 2], r.obs_sums[:, 2], b_pit.sum(1), R * r.pit.sum(1), (what, "obs pit"))
    return r, ds, obs, yr


def check_fold(table, r, ds, obs, yr, T, what=""):
    """Teacher-forced: the columns recomputed in float64 from the device's OWN y_rep and the reference's mu, m2, pit and
    deviances -- exact inputs, so no random flip and no y_rep rounding can hide a fold error.  All observations."""
    n = yr.shape[0]
    assert n == table.y.size
    y = table.y.astype(np.float64)
    v = yr.astype(np.float64)
    dev_rep = pp.deviance(table.kind, v, r.eta, r.s)
    fds, fobs = pp.fold(table.kind, y, v, r.mu, r.m2, r.pit, dev_rep, r.dev_obs, r.used)
    if table.kind == pp.NORMAL:
        _, b_pit, _, b_do, b_mu, b_m2, b_dev = normal_bounds(T, r, y)
        b_dr = b_dev(v, dev_rep, 0.0)
    else:
        b_mu, b_pit, b_m2, bd = bernoulli_bounds(T, r, y)
        b_dr, b_do = bd(v), bd(y[:, None])
    R = v.shape[1]
    zero = np.zeros(R)
    sums_close(ds[:, 0], fds[:, 0], zero, n * np.abs(v).sum(0), (what, "fold sum"))
    sums_close(ds[:, 1], fds[:, 1], zero, n * (v * v).sum(0), (what, "fold sum of squares"))
    assert np.array_equal(ds[:, 2], fds[:, 2]) and np.array_equal(ds[:, 3], fds[:, 3]), what
    sums_close(ds[:, 4], fds[:, 4], b_dr.sum(0), n * np.abs(dev_rep).sum(0), (what, "fold deviance rep"))
    sums_close(ds[:, 5], fds[:, 5], b_do.sum(0), n * np.abs(r.dev_obs).sum(0), (what, "fold deviance obs"))
    sums_close(ds[:, 6], fds[:, 6], b_mu.sum(0), n * np.abs(r.mu).sum(0), (what, "fold mu"))
    assert np.array_equal(ds[:, 7], fds[:, 7]) and np.array_equal(obs[:, 3], fobs[:, 3]), what
    sums_close(obs[:, 0], fobs[:, 0], b_mu.sum(1), R * np.abs(r.mu).sum(1), (what, "fold obs mu"))
    sums_close(obs[:, 1], fobs[:, 1], b_m2.sum(1), R * r.m2.sum(1), (what, "fold obs m2"))
    sums_close(obs[:, 2], fobs[:, 2], b_pit.sum(1), R * r.pit.sum(1), (what, "fold obs pit"))


@pytest.mark.parametrize("D", DIMS)
def test_normal_parity_and_fold_at_the_shape_edges(gpu, D):
    for shape in SHAPES:
        table, x3, seed = make_case(pp.NORMAL, D, shape)
        r, ds, obs, yr = check_normal(gpu, table, x3, seed, what=(D, shape))
        check_fold(table, r, ds, obs, yr, shape[0], what=(D, shape))
    # a ragged observation range and a draw offset past 2^32
    table, x3, seed = make_case(pp.NORMAL, D, SHAPES[3])
    check_normal(gpu, table, x3, seed, 3, 127, draw_offset=(1 << 33) + 5, what=(D, "ragged"))
    check_normal(gpu, table, x3, seed, 129, 130, what=(D, "last"))


@pytest.mark.parametrize("D", DIMS)
def test_bernoulli_draws_outside_the_margin_and_fold(gpu, D):
    for shape in SHAPES:
        table, x3, seed = make_case(pp.BERNOULLI, D, shape)
        r, ds, obs, yr = check_bernoulli(gpu, table, x3, seed, what=(D, shape))
        check_fold(table, r, ds, obs, yr, shape[0], what=(D, shape))


def test_bernoulli_at_large_logits(gpu):
    """eta = +-80: p is 1 or exp(-80) without an overflow, y_rep follows, the deviance is finite."""
    table = Table(pp.BERNOULLI, np.zeros((4, 1), np.int32), np.array([[1.0], [1.0], [-1.0], [-1.0]], np.float32),
                  np.array([1.0, 0.0, 1.0, 0.0], np.float32), np.full(4, -1, np.int32), np.zeros(4, np.float32))
    ds, obs, yr, mask, count = run(gpu, np.full((1, 70, 1), 80.0, np.float32), table, seed=3)
    assert np.isfinite(ds).all() and np.isfinite(obs).all() and count == 0
    assert np.all(yr[:2] == 1.0) and np.all(yr[2:] == 0.0)
    assert np.allclose(obs[:, 0], [70.0, 70.0, 0.0, 0.0], atol=1e-4) and np.allclose(obs[:, 2], [35.0, 0.0, 70.0, 35.0], atol=1e-4)
    assert np.allclose(ds[:, 5], 2.0 * 160.0, rtol=1e-6) and np.allclose(ds[:, 4], 0.0, atol=1e-6)


@pytest.mark.parametrize("lo, hi", [(0, 37), (7, 44)])
def test_block_of_chains_read_in_place_is_bitwise_its_copy(gpu, lo, hi):
    """row_stride > n_chains * D: a leading and an inner block of chains of a wider trace."""
    from autoreparam_amd import _lib
    table = make_table(17, 5, 33, pp.NORMAL, 9)
    wide = torch.as_tensor((0.5 * np.random.RandomState(11).randn(4, 50, 33)).astype(np.float32), device=gpu)
    block = wide[:, lo:hi]
    x, S, Cn, D, stride = _lib.trace_view(block, "test")
    assert x.data_ptr() == block.data_ptr() and stride == 50 * 33 and stride > Cn * D
    a = run(gpu, block, table, seed=5)
    b = run(gpu, block.contiguous(), table, seed=5)
    for u, v in zip(a[:4], b[:4]):
        assert np.array_equal(bits(u), bits(v))
    check_normal(gpu, table, block.contiguous().cpu().numpy(), 5, what="block")


@pytest.mark.parametrize("kind", (pp.NORMAL, pp.BERNOULLI))
def test_structure(gpu, kind):
    """Two calls; a split observation range; a sub-block of draws under its draw_offset; another seed; y_rep = NULL."""
    from autoreparam_amd import diagnostics
    N, T, D, S, Cn = 130, 5, 9, 5, 13
    table = make_table(N, T, D, kind, 21 + kind)
    x3 = (0.5 * np.random.RandomState(22).randn(S, Cn, D)).astype(np.float32)
    whole = run(gpu, x3, table, seed=77)
    again = run(gpu, x3, table, seed=77)
    r = pp.reference(table, x3.reshape(-1, D), 0, N, 77, 0)
    # sum_n |term| of the five summed columns, from the reference (1 % over: the device's terms are its own)
    size = {0: np.abs(r.y_rep).sum(0), 1: (r.y_rep ** 2).sum(0), 4: np.abs(r.dev_rep).sum(0) + 2.0 * N, 5: np.abs(r.dev_obs).sum(0),
            6: np.abs(r.mu).sum(0)}
    for u, v in zip(whole[:4], again[:4]):
        assert np.array_equal(bits(u), bits(v))
    # [0, N) = [0, a) + [a, N)
    for a in (1, 67, 129):
        lo, hi = run(gpu, x3, table, 0, a, seed=77), run(gpu, x3, table, a, N, seed=77)
        assert np.array_equal(bits(np.concatenate([lo[2], hi[2]])), bits(whole[2]))
        assert np.array_equal(bits(np.concatenate([lo[1], hi[1]])), bits(whole[1]))     # obs_sums: per observation, no split
        both = diagnostics.combine_draw_stats(lo[0], hi[0])
        assert np.array_equal(bits(both[:, (2, 3, 7)]), bits(whole[0][:, (2, 3, 7)]))
        for c in (0, 1, 4, 5, 6):                                        # two orders of one float64 sum of N terms
            assert np.all(np.abs(both[:, c] - whole[0][:, c]) <= F64 * N * 1.01 * size[c]), (a, c)
    # a sub-block of draws: steps 2 ... 4 are draws 26 ... 64 of the whole
    sub = run(gpu, x3[2:], table, seed=77, draw_offset=2 * Cn)
    assert np.array_equal(bits(sub[2]), bits(np.ascontiguousarray(whole[2][:, 2 * Cn:])))
    shifted = run(gpu, x3[2:], table, seed=77, draw_offset=0)
    assert not np.array_equal(shifted[2], sub[2])
    other = run(gpu, x3, table, seed=78)
    assert not np.array_equal(other[2], whole[2]) and np.array_equal(bits(other[0][:, 5:]), bits(whole[0][:, 5:]))
    bare = run(gpu, x3, table, seed=77, want_y_rep=False)
    assert bare[2] is None
    for i in (0, 1, 3):
        assert np.array_equal(bits(bare[i]), bits(whole[i]))


@pytest.mark.parametrize("kind", (pp.NORMAL, pp.BERNOULLI))
def test_masked_draws(gpu, kind):
    """A NaN and an inf element in two draws, one of them in the last ragged tile: mask, count, zero rows, zero y_rep and
    obs_sums over the remaining draws."""
    N, T, D, S, Cn = 9, 3, 12, 3, 70
    table = make_table(N, T, D, kind, 4 + kind)
    x3 = (0.5 * np.random.RandomState(2).randn(S, Cn, D)).astype(np.float32)
    x3[0, 5, 11] = np.nan            # draw 5
    x3[2, 69, 3] = -np.inf           # draw 209, the last: tile 3 holds 18 draws
    bad = np.array([5, 209])
    ds, obs, yr, mask, count = run(gpu, x3, table, seed=9)
    assert count == 2 and np.array_equal(np.flatnonzero(mask), bad) and set(np.unique(mask)) == {0, 1}
    assert np.all(ds[bad] == 0.0) and np.all(yr[:, bad] == 0.0) and np.isfinite(ds).all() and np.isfinite(obs).all() and np.isfinite(yr).all()
    r = pp.reference(table, x3.reshape(-1, D), 0, N, 9, 0)
    assert np.array_equal(np.flatnonzero(~r.used), bad)
    keep = np.flatnonzero(r.used)
    # the other draws are what they are without the two: bitwise a clean run's
    clean = x3.copy().reshape(-1, D)
    clean[bad] = 0.0
    ds_c, obs_c, yr_c, _, _ = run(gpu, clean.reshape(S, Cn, D), table, seed=9)
    assert np.array_equal(bits(ds[keep]), bits(ds_c[keep])) and np.array_equal(bits(yr[:, keep]), bits(yr_c[:, keep]))
    # obs_sums against the reference over the remaining draws, teacher-forced on the device's y_rep
    check_fold(table, r, ds, obs, yr, T, what="masked")
    assert np.array_equal(obs[:, 3], (yr[:, keep] <= table.y[:, None]).sum(1).astype(np.float64))
    if kind == pp.BERNOULLI:                                             # (a zeroed state has p = 1 / 2: the clean run counts it)
        assert np.all(obs_c[:, 0] - obs[:, 0] > 0.9)


def test_empirical_share_agrees_with_the_analytic_pit(gpu):
    """Normal table, R = 4 096, N = 64: #{y_rep <= y} / R is a mean of R indicators whose expectations average to the mean
    PIT, each of variance at most 1 / 4 -- five standard deviations; the seed is fixed, so the test is deterministic."""
    N, T, D, S, Cn = 64, 3, 9, 64, 64
    table = make_table(N, T, D, pp.NORMAL, 31)
    x3 = (0.5 * np.random.RandomState(32).randn(S, Cn, D)).astype(np.float32)
    ds, obs, _, _, count = run(gpu, x3, table, seed=2024, want_y_rep=False)
    R = S * Cn
    assert count == 0
    gap = np.abs(obs[:, 3] / R - obs[:, 2] / R)
    print("largest |empirical - pit| %.4f of %.4f allowed" % (gap.max(), 5.0 * math.sqrt(0.25 / R)))
    assert np.all(gap <= 5.0 * math.sqrt(0.25 / R)), float(gap.max())
    # and the replicated moments are the predictive ones
    assert abs(ds[:, 0].sum() - obs[:, 0].sum()) <= 5.0 * math.sqrt(obs[:, 1].sum())


def test_refusals(gpu):
    from autoreparam_amd import _lib, diagnostics
    L = _lib.lib()
    table = make_table(5, 2, 8, pp.NORMAL, 1)
    dt = diagnostics.upload_table(table, 8, gpu)
    x = torch.zeros(2, 3, 8, device=gpu)
    ds = torch.full((6, 8), -7.0, dtype=torch.float64, device=gpu)
    obs = torch.full((5, 4), -7.0, dtype=torch.float64, device=gpu)
    yr = torch.full((5, 6), -7.0, device=gpu)
    mask = torch.zeros(6, dtype=torch.uint8, device=gpu)
    cnt = torch.zeros((), dtype=torch.int64, device=gpu)
    need = diagnostics.predictive_workspace_bytes(5, 6)
    assert need > 0 and need % 256 == 0
    assert L.arp_predictive_workspace_bytes(0, 6) <= 0 and L.arp_predictive_workspace_bytes(5, 0) <= 0
    assert L.arp_predictive_workspace_bytes(1 << 31, 6) <= 0 and L.arp_predictive_workspace_bytes(5, 1 << 31) <= 0
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=gpu)
    p = _lib.ptr

    def call(x_=x, S=2, Cn=3, D=8, stride=24, kind=0, T=2, n0=0, n1=5, ds_=ds, obs_=obs, yr_=yr, yr_stride=6, idx=dt.idx,
             mask_=mask, ws_=ws, ws_bytes=need, offset=0):
        return L.arp_predictive_check(p(x_), S, Cn, D, stride, kind, p(idx), p(dt.w), T, p(dt.y), p(dt.scale_idx),
                                      p(dt.log_scale), n0, n1, 11, offset, p(ds_), p(obs_), p(yr_), yr_stride, p(mask_), p(cnt),
                                      C.c_void_p(ws_.data_ptr() if ws_ is not None else 0), ws_bytes, C.c_void_p(0))
    refused = ((dict(x_=None), b"required"), (dict(ds_=None), b"required"), (dict(obs_=None), b"required"),
               (dict(idx=None), b"required"), (dict(mask_=None), b"required"), (dict(D=0), b"D"), (dict(D=256), b"D"),
               (dict(stride=23), b"row_stride"), (dict(kind=2), b"kind"), (dict(T=0), b"T"), (dict(T=4097), b"T"),
               (dict(n0=5, n1=5), b"n0"), (dict(n0=3, n1=2), b"n0"), (dict(n0=-1), b"n0"), (dict(yr_stride=5), b"y_rep_stride"),
               (dict(S=0), b"n_samples"), (dict(offset=-1), b"draw_offset"), (dict(ws_bytes=need - 1), b"workspace too small"),
               (dict(ws_=None), b"workspace too small"), (dict(ws_=ws[8:]), b"256-byte aligned"))
    for kwargs, word in refused:
        assert call(**kwargs) == 1, kwargs
        msg = L.arp_last_error()
        assert word in msg and b"arp_predictive_check" in msg, (kwargs, msg)
    torch.cuda.synchronize()
    # no launch was made for a refused call: the outputs still hold what they held
    assert bool((ds == -7.0).all()) and bool((obs == -7.0).all()) and bool((yr == -7.0).all())
    assert call() == 0 and call(yr_=None, yr_stride=0) == 0
    torch.cuda.synchronize()
    assert bool((ds != -7.0).all()) and bool((obs != -7.0).all()) and bool((yr != -7.0).all())
    with pytest.raises(ValueError, match="observations is required"):
        diagnostics.predictive_check(x, dt, 0, 6)
    with pytest.raises(ValueError, match="draw_offset"):
        diagnostics.predictive_check(x, dt, draw_offset=-1)


# ---- through the CLI ----
HM = ["--num_samples=200", "--num_burnin_steps=200", "--num_adaptation_steps=150"]


def _cli(args, out=None):
    from autoreparam_amd import flags as flags_mod
    from autoreparam_amd import main as cli
    return cli.main(args, flags=flags_mod.FlagValues(), out=out)


def pipeline(root, plain, model, extra):
    """VI, one tuning run and the sampling run of `model` (CP, 256 chains) under `root` with --predictive_checks, and under
    `plain`, copied before the sampling run, without it."""
    common = ["--model=" + model, "--num_chains=256", "--seed=3", "--num_optimization_steps=400", "--method=CP"] + extra
    _cli(common + ["--results_dir=" + root, "--inference=VI"])
    _cli(common + ["--results_dir=" + root, "--inference=HMCtuning", "--num_leapfrog_steps=4"] + HM)
    shutil.copytree(root, plain)
    _cli(common + ["--results_dir=" + plain, "--inference=HMC"] + HM)
    _cli(common + ["--results_dir=" + root, "--inference=HMC", "--predictive_checks", "--loo_draws=8192"] + HM)


def check_cli(tmp_path, capsys, model, extra, kind, N, nulls):
    from autoreparam_amd import analyze, diagnostics, main as cli
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    pipeline(on, off, model, extra)
    text = capsys.readouterr().out
    assert text.count("posterior predictive checks over %d observations" % N) == 1
    path = lambda root, suffix: os.path.join(root, "CP_tied" + suffix)
    r, plain = json.load(open(path(on, ".json"))), json.load(open(path(off, ".json")))
    assert set(r) - set(plain) == set(cli.PPC_KEYS) and set(plain) <= set(r)
    assert not os.path.exists(path(off, "_ppc.npz")) and not any(k.startswith("ppc_") for k in plain)
    for key in plain:
        if "time" not in key:
            assert plain[key] == r[key], key                              # without the flag nothing changes
    for key in cli.PPC_KEYS:
        assert len(r[key]) == 1, key
        if key in nulls:
            assert r[key][0] is None, key
        else:
            assert r[key][0] is not None and math.isfinite(r[key][0]), key
    assert r["ppc_observations"] == [N] and r["ppc_chains"] == [256] and r["ppc_steps"] == [32] and r["ppc_draws"] == [8192]
    assert r["ppc_draws_left_out"] == [0] and 0 < r["ppc_time_sec"][0] <= r["diagnostics_time_sec"][0]
    z = np.load(path(on, "_ppc.npz"))
    assert sorted(z.files) == ["draw_stats", "model", "pit", "predictive_mean", "predictive_sd", "y"] and str(z["model"]) == model
    assert z["draw_stats"].shape == (8192, 8) and all(z[k].shape == (N,) for k in ("pit", "predictive_mean", "predictive_sd", "y"))
    assert np.isfinite(z["draw_stats"]).all() and np.all((z["pit"] > 0) & (z["pit"] < 1)) and np.all(z["predictive_sd"] > 0)
    # the JSON p-values are the npz columns through the one definition
    s = diagnostics.ppc_from_counts(diagnostics.ppc_counts(z["draw_stats"], z["y"]), np.zeros((N, 4)), z["y"], kind)
    for name in diagnostics.PPC_STATISTICS:
        assert r["ppc_p_" + name][0] == s.p[name], name
        assert s.p[name] is None or 0.0 <= s.p[name] <= 1.0
    assert r["ppc_obs_mean"][0] == pytest.approx(float(np.mean(z["y"].astype(np.float64))), rel=1e-12)
    # the warning line names exactly the statistics with an extreme p-value
    extreme = [name for name in diagnostics.PPC_STATISTICS if s.p[name] is not None and not 0.01 <= s.p[name] <= 0.99]
    warned = [l for l in text.splitlines() if "WARNING: posterior predictive p-value outside" in l]
    assert len(warned) == (1 if extreme else 0) and all("for: " + ", ".join(extreme) + " --" in l for l in warned)
    analyze.main(["--results_dir", os.path.dirname(on), "--model", os.path.basename(on), "--ppc"])
    assert "CP_tied: predictive p-values mean" in capsys.readouterr().out
    return r, z


def test_radon_through_the_cli(gpu, tmp_path, capsys):
    r, z = check_cli(tmp_path, capsys, "radon", ["--dataset=MN"], pp.NORMAL, 919, ())
    # a regression with an intercept reproduces the mean of its data; its likelihood has the scale fixed at 1, so nothing
    # is claimed about the spread (the deviance p-value is where that shows)
    assert 0.001 < r["ppc_p_mean"][0] < 0.999 and abs(np.mean(z["predictive_mean"]) - np.mean(z["y"])) < 0.1
    assert 0.0 < r["ppc_pit_ks"][0] < 1.0 and 0.0 <= r["ppc_coverage_90"][0] <= 1.0
    assert np.all(np.abs(z["predictive_sd"] - 1.0) < 0.5)                 # sqrt(1 + posterior variance of eta)


def test_german_credit_through_the_cli(gpu, tmp_path, capsys):
    check_cli(tmp_path, capsys, "german_credit_lognormalcentered", [], pp.BERNOULLI, 1000,
              ("ppc_p_sd", "ppc_p_min", "ppc_p_max", "ppc_rep_sd", "ppc_obs_sd", "ppc_pit_ks", "ppc_coverage_90"))
