"""GPU: arp_group_predictive_check (csrc/ppc_group.hip) through diagnostics.group_predictive_check, on the synthetic
tables of tests/test_gpu_ppc.py and the float64 definition of tests/ppc_ref.py.

1. Against arp_predictive_check under the same seed and draw offset: columns 0 - 3 and 7 of every group are, bit for bit,
   the sequential float64 fold (np.add.accumulate, ascending n) of the rows of ITS y_rep matrix that belong to the group --
   which holds the replicated values, the Philox counter and the order of the sums at once; mask and n_masked are equal;
   a masked draw's rows are zero in every group; an empty group is (0, 0, +inf, -inf, 0, 0, 0, 0).
2. Against the float64 reference: columns 4 - 6 within twice the per-(n, r) bounds of the ppc.hip header (test_gpu_ppc's
   normal_bounds / bernoulli_bounds) summed over the group; nothing is added to that.  Bernoulli deviances of the
   replicated value are taken at the reference's y_rep, which the device's must equal outside the margin around p; an
   (n, r) inside the margin (none is expected at these sizes: the margin is 1e-5 wide) is taken at the device's.
3. Composition: a group range is the slice of the full call, two halves of the draws with draw_offset are the whole, two
   calls agree -- all bit for bit; with every observation in a group, the groups summed are draw_stats to float64
   rounding and exactly in min, max and count.
4. Refusals through the C ABI, each with its message and before any launch, and the uploader's and the wrapper's.

Shapes: R in {1, 64, 65, 130 = 26 steps of 5 chains}, D in {1, 88, 255}, T in {1, 3}, both kinds, G in {1, 4, 5, 9}, N <= 64 in
a scrambled order (group members interleaved), empty groups first, in the middle and last, a group of one, a group of
everything, observations in no group, a NaN and an inf draw, and a block of chains of a wider trace (row_stride > C D)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ppc_ref as pp
from test_gpu_ppc import F64, FACTOR, bernoulli_bounds, bits, make_table, margin, normal_bounds, run

pytestmark = pytest.mark.gpu

SEED, OFFSET = 4242, (1 << 33) + 7
# (kind, D, T, N, S, C, G, layout, bad draws)
CASES = ((pp.NORMAL, 1, 1, 7, 1, 1, 1, "all", False),
         (pp.NORMAL, 88, 3, 64, 1, 64, 9, "holes", False),
         (pp.NORMAL, 255, 3, 33, 5, 13, 5, "full", True),
         (pp.NORMAL, 88, 1, 64, 26, 5, 4, "full", True),
         (pp.BERNOULLI, 1, 1, 5, 1, 64, 4, "full", False),
         (pp.BERNOULLI, 88, 3, 64, 26, 5, 9, "holes", True),
         (pp.BERNOULLI, 255, 1, 40, 5, 13, 5, "full", False),
         (pp.BERNOULLI, 9, 3, 64, 1, 1, 1, "all", False))
IDS = ["%s-D%d-T%d-N%d-R%dx%d-G%d-%s%s" % ((("normal", "bernoulli")[c[0]],) + c[1:8] + ("-bad" if c[8] else "",)) for c in CASES]


def make_groups(N, G, layout, seed):
    """group_of [N] int32.  all: one group of everything.  full: every group filled, nobody left out.  holes (G = 9):
    groups 0, 4 and 8 empty, group 1 of one, an eighth of the observations in no group.  Members are interleaved."""
    rs = np.random.RandomState(seed)
    if layout == "all":
        return np.zeros(N, np.int32)
    if layout == "full":
        g = rs.randint(0, G, size=N)
        g[:G] = np.arange(G)
    else:
        assert G == 9
        filled = np.array([2, 3, 5, 6, 7])
        g = filled[rs.randint(0, filled.size, size=N)]
        g[:filled.size] = filled
        g[filled.size] = 1
        g[filled.size + 1:filled.size + 1 + N // 8] = -1
    return g[rs.permutation(N)].astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(i):
    """(table, x3, group_of, reference) of case i; computed once and shared, never written to."""
    kind, D, T, N, S, Cn, G, layout, bad = CASES[i]
    seed = 7000 + 13 * i
    table = make_table(N, T, D, kind, seed)
    x3 = (0.5 * np.random.RandomState(seed + 1).randn(S, Cn, D)).astype(np.float32)
    if bad:
        x3[0, 3, D // 2] = np.nan
        x3[S - 1, Cn - 1, 0] = np.inf
    r = pp.reference(table, x3.reshape(-1, D), 0, N, SEED, OFFSET)
    return table, x3, make_groups(N, G, layout, seed + 2), r


def run_groups(gpu, x3, table, group_of, G, g0=0, g1=None, seed=SEED, draw_offset=OFFSET):
    """(group_stats [g1 - g0, R, 8], mask [R], count) on the host."""
    from autoreparam_amd import diagnostics
    xd = x3 if torch.is_tensor(x3) else torch.as_tensor(np.ascontiguousarray(x3, np.float32), device=gpu)
    dt = diagnostics.upload_table(table, int(xd.shape[2]), gpu)
    groups = diagnostics.upload_groups(*diagnostics.group_order(group_of, G), table.y.size, gpu)
    stats, mask, count = diagnostics.group_predictive_check(xd, dt, groups, g0, g1, seed=seed, draw_offset=draw_offset)
    return stats.cpu().numpy(), mask.cpu().numpy(), int(count.item())


def sequential_fold(yr, members):
    """Columns 0 - 3 and 7 [R, 5] of one group from the y_rep matrix: float64 sums in ascending n, one addition at a time."""
    R = yr.shape[1]
    if not members.size:
        return np.stack([np.zeros(R), np.zeros(R), np.full(R, np.inf), np.full(R, -np.inf), np.zeros(R)], axis=1)
    v = yr[members].astype(np.float64)
    return np.stack([np.add.accumulate(v, axis=0)[-1], np.add.accumulate(v * v, axis=0)[-1], v.min(axis=0), v.max(axis=0),
                     np.full(R, float(members.size))], axis=1)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_predictive_check_and_the_float64_reference(gpu, i):
    kind, D, T, N, S, Cn, G, layout, bad = CASES[i]
    table, x3, group_of, r = case(i)
    R = S * Cn
    _, _, yr, mask_p, count_p = run(gpu, x3, table, 0, N, SEED, OFFSET)
    stats, mask, count = run_groups(gpu, x3, table, group_of, G)
    assert stats.shape == (G, R, 8)
    # 1. the mask, the masked rows, and the fold of arp_predictive_check's own y_rep
    assert np.array_equal(mask, mask_p) and count == count_p == int(mask.sum()) == (2 if bad else 0)
    assert np.array_equal(mask != 0, ~r.used)
    used = mask == 0
    assert np.all(stats[:, ~used] == 0.0)
    sizes = np.bincount(group_of[group_of >= 0], minlength=G)
    if layout == "holes":
        assert np.array_equal(np.flatnonzero(sizes == 0), [0, 4, 8]) and sizes[1] == 1 and np.sum(group_of < 0) == N // 8
    for g in range(G):
        members = np.flatnonzero(group_of == g)
        want = sequential_fold(yr, members)
        assert np.array_equal(bits(stats[g][used][:, (0, 1, 2, 3, 7)]), bits(want[used])), (g, members.size)
        if not members.size:
            assert np.all(stats[g][used][:, 4:7] == 0.0)
    # 2. columns 4 - 6 against the float64 reference, within twice the header's bounds summed over the group
    y = table.y.astype(np.float64)
    if kind == pp.NORMAL:
        _, _, b_dr, b_do, b_mu, _, _ = normal_bounds(T, r, y)
        dev_rep = r.dev_rep
    else:
        inside, b_mu = margin(T, r)
        assert not ((yr.astype(np.float64) != r.y_rep) & ~inside)[:, used].any()
        print("(n, r) inside the margin around p: %d of %d" % (int(inside[:, used].sum()), inside[:, used].size))
        b_dev = bernoulli_bounds(T, r, y)[3]
        v = np.where(inside, yr.astype(np.float64), r.y_rep)
        dev_rep = pp.deviance(kind, v, r.eta, r.s)
        b_dr, b_do = b_dev(v), b_dev(y[:, None])
    worst = 0.0
    for g in range(G):
        members = np.flatnonzero(group_of == g)
        for c, ref, allow in ((4, dev_rep, b_dr), (5, r.dev_obs, b_do), (6, r.mu, b_mu)):
            gap = np.abs(stats[g][used, c] - ref[members][:, used].sum(axis=0))
            slack = FACTOR * allow[members][:, used].sum(axis=0)
            assert np.all(gap <= slack), (g, c, float(np.max(gap / np.maximum(slack, 1e-300))))
            if members.size:
                worst = max(worst, float(np.max(gap / slack)))
    print("largest share of the allowance used by columns 4 - 6: %.3f" % worst)


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c[6] >= 4], ids=[IDS[i] for i, c in enumerate(CASES) if c[6] >= 4])
def test_composition(gpu, i):
    kind, D, T, N, S, Cn, G, layout, bad = CASES[i]
    table, x3, group_of, r = case(i)
    whole, mask, count = run_groups(gpu, x3, table, group_of, G)
    again = run_groups(gpu, x3, table, group_of, G)
    assert np.array_equal(bits(whole), bits(again[0])) and np.array_equal(mask, again[1]) and count == again[2]
    for g0, g1 in ((0, 1), (1, 3), (G - 1, G), (2, G)):
        part, part_mask, part_count = run_groups(gpu, x3, table, group_of, G, g0, g1)
        assert np.array_equal(bits(part), bits(whole[g0:g1])), (g0, g1)
        assert np.array_equal(part_mask, mask) and part_count == count
    if S > 1:                                                            # two halves of the draws, the second under its offset
        s = S // 2
        lo = run_groups(gpu, x3[:s], table, group_of, G)
        hi = run_groups(gpu, x3[s:], table, group_of, G, draw_offset=OFFSET + s * Cn)
        assert np.array_equal(bits(np.concatenate([lo[0], hi[0]], axis=1)), bits(whole))
        assert np.array_equal(np.concatenate([lo[1], hi[1]]), mask) and lo[2] + hi[2] == count
        shifted = run_groups(gpu, x3[s:], table, group_of, G)            # (without the offset: other random numbers)
        assert not np.array_equal(shifted[0][:, :, 0], hi[0][:, :, 0])
    if layout == "full":                                                 # nobody left out: the groups add up to draw_stats
        ds = run(gpu, x3, table, 0, N, SEED, OFFSET, want_y_rep=False)[0]
        assert np.array_equal(whole[:, :, 7].sum(axis=0), ds[:, 7])
        assert np.array_equal(whole[:, :, 2].min(axis=0), ds[:, 2]) and np.array_equal(whole[:, :, 3].max(axis=0), ds[:, 3])
        size = {0: np.abs(r.y_rep).sum(0), 1: (r.y_rep ** 2).sum(0), 4: np.abs(r.dev_rep).sum(0) + 2.0 * N, 5: np.abs(r.dev_obs).sum(0),
                6: np.abs(r.mu).sum(0)}
        used = mask == 0
        for c in (0, 1, 4, 5, 6):                                        # two orders of one float64 sum of N terms
            gap = np.abs(whole[:, :, c].sum(axis=0) - ds[:, c])[used]
            assert np.all(gap <= F64 * N * 1.01 * size[c][used]), c


def test_the_walk_over_ranges_of_groups_gives_the_counts_of_one_call(gpu, monkeypatch):
    """report_common.replicate_groups: a budget of two groups' statistics per call (five calls for nine groups) against one
    call -- a group's row does not depend on its range, so the counts are equal bit for bit; a further mask is or-ed in."""
    from autoreparam_amd import diagnostics, report_common
    kind, D, T, N, S, Cn, G, layout, bad = CASES[5]
    table, x3, group_of, _ = case(5)
    xd = torch.as_tensor(x3, device=gpu)
    dt = diagnostics.upload_table(table, D, gpu)
    groups = diagnostics.upload_groups(*diagnostics.group_order(group_of, G), N, gpu)
    calls = []
    real = diagnostics.group_predictive_check

    def counted(*a, **k):
        calls.append((a[3], a[4]))
        return real(*a, **k)
    stats, mask, _ = real(xd, dt, groups, seed=SEED, draw_offset=OFFSET)
    want = diagnostics.ppc_group_counts(stats, table.y, group_of, mask)
    monkeypatch.setattr(diagnostics, "group_predictive_check", counted)
    one, left = report_common.replicate_groups(xd, dt, groups, table.y, group_of, SEED, OFFSET)
    assert calls == [(0, 9)]
    del calls[:]
    tiled, _ = report_common.replicate_groups(xd, dt, groups, table.y, group_of, SEED, OFFSET, budget=2 * 64 * S * Cn)
    assert calls == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 9)]
    extra = torch.zeros(S * Cn, dtype=torch.bool, device=gpu)
    extra[7] = True
    fewer, left_more = report_common.replicate_groups(xd, dt, groups, table.y, group_of, SEED, OFFSET, left_out=extra)
    assert np.array_equal(one, want, equal_nan=True) and np.array_equal(tiled, want, equal_nan=True)
    assert np.array_equal(left.cpu().numpy(), mask.cpu().numpy() != 0) and int(left_more.sum()) == int(left.sum()) + 1
    filled = np.bincount(group_of[group_of >= 0], minlength=G) > 0
    assert np.all(one[filled, 0] == S * Cn - 2) and np.all(fewer[filled, 0] == S * Cn - 3) and np.all(one[~filled] == 0.0)


@pytest.mark.parametrize("lo, hi", [(0, 37), (7, 44)])
def test_block_of_chains_read_in_place_is_bitwise_its_copy(gpu, lo, hi):
    """row_stride > n_chains * D: a leading and an inner block of chains of a wider trace."""
    from autoreparam_amd import _lib
    table = make_table(17, 3, 33, pp.NORMAL, 9)
    group_of = make_groups(17, 5, "full", 10)
    wide = torch.as_tensor((0.5 * np.random.RandomState(11).randn(4, 50, 33)).astype(np.float32), device=gpu)
    block = wide[:, lo:hi]
    x, S, Cn, D, stride = _lib.trace_view(block, "test")
    assert x.data_ptr() == block.data_ptr() and stride == 50 * 33 and stride > Cn * D
    a = run_groups(gpu, block, table, group_of, 5)
    b = run_groups(gpu, block.contiguous(), table, group_of, 5)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 0
    assert np.isfinite(a[0]).all() and np.array_equal(a[0][:, :, 7].sum(axis=0), np.full(4 * (hi - lo), 17.0))


def test_refusals(gpu):
    from autoreparam_amd import _lib, diagnostics
    L = _lib.lib()
    table = make_table(5, 2, 8, pp.NORMAL, 1)
    dt = diagnostics.upload_table(table, 8, gpu)
    group_of = np.array([1, 0, -1, 1, 2], np.int32)
    groups = diagnostics.upload_groups(*diagnostics.group_order(group_of, 3), 5, gpu)
    assert groups.G == 3 and groups.n_grouped == 4 and list(groups.sizes) == [1, 2, 1]
    assert groups.order.cpu().tolist() == [1, 0, 3, 4] and groups.group_start.cpu().tolist() == [0, 1, 3, 4]
    x = torch.zeros(2, 3, 8, device=gpu)
    gs = torch.full((3, 6, 8), -7.0, dtype=torch.float64, device=gpu)
    mask = torch.full((6,), 9, dtype=torch.uint8, device=gpu)
    cnt = torch.zeros((), dtype=torch.int64, device=gpu)
    p = _lib.ptr

    def call(x_=x, S=2, Cn=3, D=8, stride=24, kind=0, T=2, idx=dt.idx, n_obs=5, order=groups.order, n_grouped=4,
             start=groups.group_start, G=3, g0=0, g1=3, offset=0, gs_=gs, mask_=mask, cnt_=cnt):
        return L.arp_group_predictive_check(p(x_), S, Cn, D, stride, kind, p(idx), p(dt.w), T, p(dt.y), p(dt.scale_idx),
                                            p(dt.log_scale), n_obs, p(order), n_grouped, p(start), G, g0, g1, 11, offset, p(gs_),
                                            p(mask_), p(cnt_), C.c_void_p(0))
    refused = ((dict(x_=None), b"required"), (dict(idx=None), b"required"), (dict(start=None), b"required"),
               (dict(gs_=None), b"required"), (dict(mask_=None), b"required"), (dict(cnt_=None), b"required"),
               (dict(order=None), b"order"), (dict(D=0), b"D"), (dict(D=256), b"D"), (dict(stride=23), b"row_stride"),
               (dict(kind=2), b"kind"), (dict(T=0), b"T"), (dict(T=4097), b"T"), (dict(S=0), b"n_samples"),
               (dict(n_obs=0), b"n_obs"), (dict(n_obs=1 << 31), b"n_obs"), (dict(n_grouped=-1), b"n_grouped"),
               (dict(G=0, g1=0), b"n_groups"), (dict(g0=-1), b"g0"), (dict(g0=2, g1=2), b"g0"), (dict(g0=2, g1=1), b"g0"),
               (dict(g1=4), b"g0"), (dict(offset=-1), b"draw_offset"))
    for kwargs, word in refused:
        assert call(**kwargs) == 1, kwargs
        msg = L.arp_last_error()
        assert word in msg and b"arp_group_predictive_check" in msg, (kwargs, msg)
    torch.cuda.synchronize()
    # no launch was made for a refused call: the outputs still hold what they held
    assert bool((gs == -7.0).all()) and bool((mask == 9).all())
    assert call() == 0 and call(order=None, n_grouped=0, start=torch.zeros(4, dtype=torch.int32, device=gpu)) == 0
    torch.cuda.synchronize()
    assert bool((gs != -7.0).all()) and bool((mask == 0).all())
    # the uploader and the wrapper
    for order, start, word in (([1, 0, 5], [0, 1, 3], "outside the table"), ([1, -1], [0, 2], "outside the table"),
                               ([1, 0, 3], [0, 2, 1, 3], "ascend"), ([1, 0, 3], [1, 3], "ascend"), ([1, 0, 3], [0, 2], "ascend"),
                               ([1, 0], [0], "at least one group")):
        with pytest.raises(ValueError, match=word):
            diagnostics.upload_groups(order, start, 5, gpu)
    with pytest.raises(ValueError, match="group_of entries"):
        diagnostics.group_order([0, 3], 3)
    with pytest.raises(ValueError, match="groups is required"):
        diagnostics.group_predictive_check(x, dt, groups, 1, 1)
    with pytest.raises(ValueError, match="groups is required"):
        diagnostics.group_predictive_check(x, dt, groups, 0, 4)
    with pytest.raises(ValueError, match="draw_offset"):
        diagnostics.group_predictive_check(x, dt, groups, draw_offset=-1)
    with pytest.raises(ValueError, match="a table of 4 observations"):
        diagnostics.group_predictive_check(x, dt, diagnostics.upload_groups([0], [0, 1], 4, gpu))
