"""GPU: arp_group_loglik (csrc/logo.hip) through diagnostics.group_loglik, on the synthetic cases of tests/logo_cases.py
(test_gpu_ppc's make_table, test_gpu_ppc_groups's make_groups, a synthetic site table) and the float64 reference of
tests/logo_ref.py.

1. lc against arp_pointwise_loglik: lc equals, bit for bit (uint32 views), float32 of the float64 ascending sum
   (np.add.accumulate, one addition at a time) of arp_pointwise_loglik's OWN output rows of the group; mask and n_masked
   are equal; masked draws are 0; empty groups are 0 -- in lc and in lm.
2. lm against logo_ref.marginal (scipy's multivariate_normal, no integral, not the kernel's formula): within FACTOR = 2 of
   the bound in the header of csrc/logo.hip (logo_ref.bound), nothing added; and the bound itself stays below
   2^-8 max(1, |lm|) on every case, so that a vacuous bound cannot pass.
3. Composition, all bitwise: a group range is the slice of the full call, two halves of the draws are the whole, two calls
   agree, lm = NULL leaves lc unchanged, and the report's walk over group ranges (main.logo_columns with a small budget)
   gives the columns of one range.
4. Refusals through the C ABI, each with its message and before any launch; the uploader's and the wrapper's.

Shapes: logo_cases.CASES -- R in {1, 64, 65, 130 = 26 x 5}, D in {1, 88, 255}, T in {1, 3}, both kinds, G in {1, 4, 5, 9} with
holes (empty groups first, in the middle and last, a group of one, ungrouped observations, more waves than groups), N <= 64
interleaved, slopes 1 and random in (0, 2), exp(sj) in {e^-6, 1, e^6}, t0 five prior sds from loc, a NaN and an inf draw; and
a block of chains of a wider trace."""
import ctypes as C

import numpy as np
import pytest
import torch

import logo_cases as cases
import logo_ref as lg
import ppc_ref as pp
from test_gpu_ppc import FACTOR, bits

pytestmark = pytest.mark.gpu

CAP = 2.0 ** -8


def upload(gpu, c, x3=None):
    from autoreparam_amd import diagnostics
    x3 = c.x3 if x3 is None else x3
    xd = x3 if torch.is_tensor(x3) else torch.as_tensor(np.array(x3, np.float32), device=gpu)
    D = int(xd.shape[2])
    dt = diagnostics.upload_table(c.table, D, gpu)
    groups = diagnostics.upload_logo_groups(*diagnostics.group_order(c.group_of, c.G), c.slope, c.elem, c.table.y.size, D, gpu)
    site = diagnostics.upload_site_table(c.site, D, gpu) if c.table.kind == pp.NORMAL else None
    return xd, dt, groups, site


def run_logo(gpu, c, x3=None, g0=0, g1=None, marginal=True):
    """(lc [g1 - g0, R], lm or None, mask [R], count) on the host."""
    from autoreparam_amd import diagnostics
    xd, dt, groups, site = upload(gpu, c, x3)
    lc, lm, mask, count = diagnostics.group_loglik(xd, dt, groups, site if marginal else None, g0, g1)
    return lc.cpu().numpy(), None if lm is None else lm.cpu().numpy(), mask.cpu().numpy(), int(count.item())


@pytest.mark.parametrize("i", range(len(cases.CASES)), ids=cases.IDS)
def test_against_pointwise_loglik_and_the_float64_reference(gpu, i):
    from autoreparam_amd import diagnostics
    kind, D, T, N, S, Cn, G, layout, bad = cases.CASES[i][:9]
    c = cases.case(i)
    R = S * Cn
    xd, dt, _, _ = upload(gpu, c)
    ll, mask_p, count_p = diagnostics.pointwise_loglik(xd, dt)
    ll, mask_p, count_p = ll.cpu().numpy(), mask_p.cpu().numpy(), int(count_p.item())
    lc, lm, mask, count = run_logo(gpu, c)
    assert lc.shape == (G, R) and lc.dtype == np.float32 and (lm is None) == (kind != pp.NORMAL)
    # 1. the mask, the masked draws, the empty groups, and the fold of arp_pointwise_loglik's own rows
    x = c.x3.reshape(-1, D)
    ok = np.isfinite(x).all(axis=1)
    assert np.array_equal(mask, mask_p) and count == count_p == int(mask.sum()) == (2 if bad else 0)
    assert np.array_equal(mask == 0, ok)
    sizes = np.bincount(c.group_of[c.group_of >= 0], minlength=G)
    if layout == "holes":
        assert np.array_equal(np.flatnonzero(sizes == 0), [0, 4, 8]) and sizes[1] == 1 and np.sum(c.group_of < 0) == N // 8
    for out in (lc, lm):
        if out is not None:
            assert np.all(out[:, ~ok] == 0.0) and np.all(out[sizes == 0] == 0.0)
    for g in range(G):
        members = lg.members_of(c.group_of, g)
        want = np.add.accumulate(ll[members].astype(np.float64), axis=0)[-1].astype(np.float32) if members.size else np.zeros(R, np.float32)
        assert np.array_equal(bits(lc[g][ok]), bits(want[ok])), (g, members.size)
    if lm is None:
        return
    # 2. lm against the reference, within twice the header's bound; the bound itself is not vacuous
    q = lg.quantities(c.table, c.site, x[ok], c.slope, c.elem)
    ref = lg.marginal(c.table, q, c.group_of, G, c.slope)
    allow = lg.bound(c.table, q, c.group_of, G, ref)
    filled = sizes > 0
    gap = np.abs(lm[:, ok].astype(np.float64) - ref)
    print("largest share of the bound used by lm: %.3f; largest bound / (2^-8 max(1, |lm|)): %.3g; |lm| up to %.3g" % (
        float(np.max(gap[filled] / allow[filled])), float(np.max((allow / (CAP * np.maximum(1.0, np.abs(ref))))[filled])),
        float(np.abs(ref).max())))
    assert np.all(np.isfinite(lm))
    assert np.all(gap[filled] <= FACTOR * allow[filled]), float(np.max(gap[filled] / allow[filled]))
    assert np.all(allow[filled] < CAP * np.maximum(1.0, np.abs(ref[filled])))


@pytest.mark.parametrize("i", [i for i, c in enumerate(cases.CASES) if c[6] >= 4],
                         ids=[cases.IDS[i] for i, c in enumerate(cases.CASES) if c[6] >= 4])
def test_composition(gpu, i):
    kind, D, T, N, S, Cn, G = cases.CASES[i][:7]
    c = cases.case(i)
    eq = lambda a, b: (a is None and b is None) or np.array_equal(bits(a), bits(b))
    whole = run_logo(gpu, c)
    again = run_logo(gpu, c)
    assert eq(whole[0], again[0]) and eq(whole[1], again[1]) and np.array_equal(whole[2], again[2]) and whole[3] == again[3]
    alone = run_logo(gpu, c, marginal=False)                                # lm = NULL: lc is unchanged
    assert alone[1] is None and eq(alone[0], whole[0]) and np.array_equal(alone[2], whole[2]) and alone[3] == whole[3]
    for g0, g1 in ((0, 1), (1, 3), (G - 1, G), (2, G)):
        part = run_logo(gpu, c, g0=g0, g1=g1)
        assert eq(part[0], whole[0][g0:g1]) and eq(part[1], None if whole[1] is None else whole[1][g0:g1]), (g0, g1)
        assert np.array_equal(part[2], whole[2]) and part[3] == whole[3]
    if S > 1:                                                                # two halves of the draws are the whole
        s = S // 2
        lo, hi = run_logo(gpu, c, c.x3[:s]), run_logo(gpu, c, c.x3[s:])
        for k in (0, 1):
            assert eq(None if lo[k] is None else np.concatenate([lo[k], hi[k]], axis=1), whole[k]), k
        assert np.array_equal(np.concatenate([lo[2], hi[2]]), whole[2]) and lo[3] + hi[3] == whole[3]


@pytest.mark.parametrize("i", [1, 7], ids=["normal", "bernoulli"])
def test_the_walk_over_ranges_of_groups_gives_the_columns_of_one_range(gpu, i, monkeypatch):
    """main.logo_columns: a budget of two groups per call (five calls for nine groups) against one call -- a group's row does
    not depend on its range, so the PSIS columns are equal bit for bit; the rows of empty groups are NaN."""
    from autoreparam_amd import diagnostics, main as cli, report_common
    kind, D, T, N, S, Cn, G = cases.CASES[i][:7]
    c = cases.case(i)
    xd, dt, groups, site = upload(gpu, c)
    R, forms = S * Cn, 2 if site is not None else 1
    calls = []
    real = diagnostics.group_loglik

    def counted(*a, **k):
        calls.append((a[4], a[5]))
        return real(*a, **k)
    monkeypatch.setattr(diagnostics, "group_loglik", counted)
    one = cli.logo_columns(xd, dt, groups, site, groups.sizes)
    assert calls == [(0, 9)]
    del calls[:]
    budget = 2 * forms * 4 * R + diagnostics.psis_workspace_bytes(2, R)
    assert report_common.logo_range_size(G, R, forms, diagnostics.psis_workspace_bytes, budget) == 2
    monkeypatch.setattr(cli, "LOO_CHUNK_BYTES", budget)
    tiled = cli.logo_columns(xd, dt, groups, site, groups.sizes)
    assert calls == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 9)]
    for a, b in zip(one[:2], tiled[:2]):
        assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True)
    assert (one[1] is None) == (site is None) and one[0].shape == (G, 8)
    empty = groups.sizes == 0
    assert np.all(np.isnan(one[0][empty])) and not np.isnan(one[0][~empty][:, 0]).any()
    assert np.array_equal(one[2].cpu().numpy(), tiled[2].cpu().numpy())


@pytest.mark.parametrize("lo, hi", [(0, 37), (7, 44)])
def test_block_of_chains_read_in_place_is_bitwise_its_copy(gpu, lo, hi):
    """row_stride > n_chains * D: a leading and an inner block of chains of a wider trace."""
    from autoreparam_amd import _lib
    c = cases.case(1)
    D = c.x3.shape[2]
    wide = torch.as_tensor((0.5 * np.random.RandomState(11).randn(4, 50, D)).astype(np.float32), device=gpu)
    block = wide[:, lo:hi]
    x, S, Cn, _, stride = _lib.trace_view(block, "test")
    assert x.data_ptr() == block.data_ptr() and stride == 50 * D and stride > Cn * D
    a, b = run_logo(gpu, c, block), run_logo(gpu, c, block.contiguous())
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    assert np.array_equal(a[2], b[2]) and a[3] == b[3] == 0 and np.isfinite(a[0]).all() and np.isfinite(a[1]).all()


def test_refusals(gpu):
    from autoreparam_amd import _lib, diagnostics
    L = _lib.lib()
    c = cases.case(1)
    D, N, G = c.x3.shape[2], c.table.y.size, c.G
    _, dt, groups, site = upload(gpu, c)
    x = torch.zeros(2, 3, D, device=gpu)
    lc = torch.full((G, 6), -7.0, dtype=torch.float32, device=gpu)
    lm = torch.full((G, 6), -7.0, dtype=torch.float32, device=gpu)
    mask = torch.full((6,), 9, dtype=torch.uint8, device=gpu)
    cnt = torch.zeros((), dtype=torch.int64, device=gpu)
    p = _lib.ptr

    def call(x_=x, S=2, Cn=3, D_=D, stride=3 * D, kind=0, T=3, idx=dt.idx, n_obs=N, order=groups.order, slope=groups.slope,
             n_grouped=groups.n_grouped, start=groups.group_start, elem=groups.elem, G_=G, g0=0, g1=G, loc_idx=site.loc_idx,
             log_scale0=site.log_scale0, lc_=lc, lm_=lm, out_stride=6, mask_=mask, cnt_=cnt):
        return L.arp_group_loglik(p(x_), S, Cn, D_, stride, kind, p(idx), p(dt.w), T, p(dt.y), p(dt.scale_idx), p(dt.log_scale),
                                  n_obs, p(order), p(slope), n_grouped, p(start), p(elem), G_, g0, g1, p(loc_idx), p(site.loc_w),
                                  p(site.loc0), p(site.scale_idx), p(site.scale_w), p(log_scale0), p(lc_), p(lm_), out_stride,
                                  p(mask_), p(cnt_), C.c_void_p(0))
    refused = ((dict(x_=None), b"required"), (dict(idx=None), b"required"), (dict(start=None), b"required"),
               (dict(mask_=None), b"required"), (dict(cnt_=None), b"required"), (dict(slope=None), b"slope"),
               (dict(elem=None), b"elem"), (dict(lc_=None, lm_=None), b"both outputs"), (dict(loc_idx=None), b"site table"),
               (dict(log_scale0=None), b"site table"), (dict(kind=1), b"ARP_OBS_NORMAL"), (dict(out_stride=5), b"out_stride"),
               (dict(order=None), b"order"), (dict(D_=0), b"D"), (dict(D_=256), b"D"), (dict(stride=3 * D - 1), b"row_stride"),
               (dict(kind=2), b"kind"), (dict(T=0), b"T"), (dict(T=4097), b"T"), (dict(S=0), b"n_samples"),
               (dict(n_obs=0), b"n_obs"), (dict(n_obs=1 << 31), b"n_obs"), (dict(n_grouped=-1), b"n_grouped"),
               (dict(G_=0, g1=0), b"n_groups"), (dict(g0=-1), b"g0"), (dict(g0=2, g1=2), b"g0"), (dict(g0=2, g1=1), b"g0"),
               (dict(g1=G + 1), b"g0"))
    for kwargs, word in refused:
        assert call(**kwargs) == 1, kwargs
        msg = L.arp_last_error()
        assert word in msg and b"arp_group_loglik" in msg, (kwargs, msg)
    torch.cuda.synchronize()
    # no launch was made for a refused call: the outputs still hold what they held
    assert bool((lc == -7.0).all()) and bool((lm == -7.0).all()) and bool((mask == 9).all())
    # a NULL site pointer is fine without lm, and so is Bernoulli data; either output alone
    assert call(lm_=None, loc_idx=None) == 0 and call(lm_=None, kind=1) == 0 and call(lc_=None) == 0 and call() == 0
    torch.cuda.synchronize()
    assert bool((lc != -7.0).all()) and bool((lm != -7.0).all()) and bool((mask == 0).all())
    # the uploader and the wrapper
    order, start = diagnostics.group_order(c.group_of, G)
    for slope, elem, word in ((c.slope[:-1], c.elem, "slope"), (np.where(np.arange(N) == 3, np.nan, c.slope), c.elem, "slope"),
                              (c.slope, c.elem[:-1], "elem"), (c.slope, c.elem + D, "elem"), (c.slope, c.elem - 3, "elem")):
        with pytest.raises(ValueError, match=word):
            diagnostics.upload_logo_groups(order, start, slope, elem, N, D, gpu)
    with pytest.raises(ValueError, match="outside the table"):
        diagnostics.upload_logo_groups(order, start, c.slope[:5], c.elem, 5, D, gpu)
    xd = torch.as_tensor(np.array(c.x3), device=gpu)
    with pytest.raises(ValueError, match="groups is required"):
        diagnostics.group_loglik(xd, dt, groups, site, 1, 1)
    with pytest.raises(ValueError, match="groups is required"):
        diagnostics.group_loglik(xd, dt, groups, site, 0, G + 1)
    with pytest.raises(ValueError, match="DeviceLogoGroups"):
        diagnostics.group_loglik(xd, dt, diagnostics.upload_groups(order, start, N, gpu))
    with pytest.raises(ValueError, match="DeviceSiteTable"):
        diagnostics.group_loglik(xd, dt, groups, c.site)
    with pytest.raises(ValueError, match="out must be"):
        diagnostics.group_loglik(xd, dt, groups, site, out=torch.empty(G, c.x3.shape[0] * c.x3.shape[1], device=gpu))
    b = cases.case(7)
    _, bdt, bgroups, _ = upload(gpu, b)
    with pytest.raises(RuntimeError, match="ARP_OBS_NORMAL"):
        diagnostics.group_loglik(torch.as_tensor(np.array(b.x3), device=gpu), bdt, bgroups, diagnostics.upload_site_table(b.site, 88, gpu))
