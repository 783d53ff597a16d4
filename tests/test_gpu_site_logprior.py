"""GPU: arp_site_logprior (csrc/prior.hip) through diagnostics.site_logprior against the float64 evaluation of
tests/site_ref.py: every model's real site table on a strided trace with NaN padding, every element within the header's
first-order bound (evaluated in float64 from the float32-rounded table and the float32 draws) and every group within
the sum of its elements' bounds plus the accumulation term; synthetic tables at the shape edges (D = 1, 2, 254, 255; one,
seven interleaved and D groups; a group without elements); masked draws; the bitwise invariances; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import site_ref as sr
from test_site_table_host import SPECS

pytestmark = pytest.mark.gpu

MODELS = sorted(name for name in SPECS if name != "radon_PA")          # the nine models (radon at MN)


def upload(gpu, table, D):
    from autoreparam_amd import diagnostics
    return diagnostics.upload_site_table(table, D, gpu)


def run(gpu, x3, up, group_of=None, want_elements=True):
    """(group_lp [R, G], elem_lp [R, D] or None, mask [R], count) on the host for a [S, C, D] float32 array or device tensor"""
    from autoreparam_amd import diagnostics
    xd = x3 if torch.is_tensor(x3) else torch.as_tensor(np.ascontiguousarray(x3, np.float32), device=gpu)
    g, e, mask, count = diagnostics.site_logprior(xd, up, group_of, want_elements)
    return g.cpu().numpy(), (None if e is None else e.cpu().numpy()), mask.cpu().numpy(), int(count.item())


def check(gpu, table, x3, group_of, what):
    """elem_lp within the header's bound, group_lp within its elements' bounds and the accumulation term, nothing masked;
    returns the largest deviation / bound of the elements."""
    S, Cn, D = (int(v) for v in x3.shape)
    up = upload(gpu, table, D)
    groups = np.asarray(up.host.part if group_of is None else group_of)
    G = int(groups.max()) + 1
    got_g, got_e, mask, count = run(gpu, x3, up, group_of)
    x = (x3.cpu().numpy() if torch.is_tensor(x3) else np.asarray(x3, np.float32)).reshape(S * Cn, D).astype(np.float64)
    ref = sr.elements(up.host, x)
    allow = sr.bound(up.host, x)
    assert got_e.shape == (S * Cn, D) and got_e.dtype == np.float32 and got_g.shape == (S * Cn, G) and got_g.dtype == np.float64
    assert count == 0 and not mask.any(), what
    assert np.isfinite(ref).all() and np.isfinite(got_e).all(), what
    dev = np.abs(got_e.astype(np.float64) - ref)
    ratio = float((dev / allow).max())
    print("%s: elements, largest deviation / bound %.3f" % (what, ratio))
    assert (dev <= allow).all(), (what, ratio)
    dev_g = np.abs(got_g - sr.groups(ref, groups, G))
    allow_g = sr.group_bound(got_e, allow, groups, G)
    assert (dev_g <= allow_g).all(), (what, float((dev_g / allow_g).max()))
    return ratio


@pytest.mark.parametrize("name", MODELS)
def test_every_model_at_its_real_table(gpu, name):
    """[2, 65, D] of 0.7 N(0, 1): 130 draws cross the tile edge at 64, the chain count is no multiple of 64; rows
    65 D + 3 floats apart, the padding NaN (a read past a row's end would mask a draw); groups = parts."""
    from autoreparam_amd import _lib, models
    spec = SPECS[name](models)
    D = spec.D
    rs = np.random.RandomState(31)
    wide = np.full((2, 65 * D + 3), np.nan, np.float32)
    wide[:, :65 * D] = (0.7 * rs.randn(2, 65 * D)).astype(np.float32)
    x3 = torch.as_strided(torch.as_tensor(wide, device=gpu), (2, 65, D), (65 * D + 3, D, 1))
    view = _lib.trace_view(x3, "test")
    assert view[0].data_ptr() == x3.data_ptr() and view[4] == 65 * D + 3
    check(gpu, spec.site_table(), x3, None, name)


def synthetic(D, seed=0):
    """Every element's loc parent is the element before it, its scale parent element 0; the forms cycle 0, 1, 2 (a shape
    in (0.5, 1.5) for the log-Gamma rows); random normalisers."""
    from autoreparam_amd import models
    rs = np.random.RandomState(1000 * seed + D)
    form = (np.arange(D) % 3).astype(np.int32)
    loc_idx, scale_idx = np.zeros((D, 2), np.int32), np.zeros((D, 2), np.int32)
    loc_w, scale_w = np.zeros((D, 2)), np.zeros((D, 2))
    loc_idx[1:, 0] = np.arange(D - 1)
    loc_w[1:, 0] = rs.randn(D - 1)
    scale_w[1:, 0] = 0.3 * rs.randn(D - 1)
    loc0 = 0.5 * rs.randn(D)
    loc0[form == 2] = 0.5 + rs.rand(int((form == 2).sum()))
    return models.SiteTable(form, loc_idx, loc_w, loc0, scale_idx, scale_w, 0.3 * rs.randn(D), rs.randn(D), np.zeros(D, np.int32))


def draws(S, Cn, D, seed):
    return (0.7 * np.random.RandomState(seed).randn(S, Cn, D)).astype(np.float32)


def test_one_element_one_draw(gpu):
    check(gpu, synthetic(1), draws(1, 1, 1, 1), None, "D=1 R=1")


@pytest.mark.parametrize("R", (63, 64, 65))
def test_funnel_at_the_tile_edge(gpu, R):
    from autoreparam_amd import models
    table = models._spec_funnel().site_table()
    check(gpu, table, draws(1, R, 2, R), None, "funnel R=%d" % R)
    check(gpu, table, draws(1, R, 2, R), np.zeros(2, np.int64), "funnel R=%d, one group" % R)


@pytest.mark.parametrize("grouping", ("one", "each", "mod7", "with_gaps"))
def test_widest_state(gpu, grouping):
    """D = 255, 65 draws.  One group spans all four waves' quarters; D groups are runs of one element; d % 7 is not
    contiguous; `with_gaps` leaves groups 1 and 3 of five without elements (they are written as 0)."""
    D = 255
    group_of = {"one": np.zeros(D, np.int64), "each": np.arange(D), "mod7": np.arange(D) % 7,
                "with_gaps": 2 * (np.arange(D) % 3)}[grouping]
    table, x3 = synthetic(D), draws(1, 65, D, 7)
    check(gpu, table, x3, group_of, "D=255 " + grouping)
    if grouping == "with_gaps":
        got = run(gpu, x3, upload(gpu, table, D), group_of)[0]
        assert got.shape == (65, 5) and np.all(got[:, (1, 3)] == 0.0) and np.all(got[:, (0, 2, 4)] != 0.0)


def test_even_width_where_the_pitch_is_padded(gpu):
    check(gpu, synthetic(254), draws(1, 65, 254, 9), np.arange(254) % 7, "D=254")


def test_masked_draws_are_counted_and_written_as_zero(gpu):
    D = 12
    table = synthetic(D)
    up = upload(gpu, table, D)
    group_of = np.arange(D) % 5
    clean = draws(2, 65, D, 3)
    x3 = clean.copy()
    x3[0, 0, 11] = np.nan            # draw 0
    x3[0, 64, 0] = np.inf            # draw 64: the first of the second tile
    x3[1, 64, 5] = -np.inf           # draw 129: the last
    got_g, got_e, mask, count = run(gpu, x3, up, group_of)
    bad = np.array([0, 64, 129])
    assert count == 3 and np.array_equal(np.flatnonzero(mask), bad) and set(np.unique(mask)) == {0, 1}
    assert np.all(got_g[bad] == 0.0) and np.all(got_e[bad] == 0.0)
    ref_g, ref_e, ref_mask, ref_count = run(gpu, clean, up, group_of)
    keep = np.setdiff1d(np.arange(130), bad)
    assert ref_count == 0 and not ref_mask.any()
    assert np.array_equal(got_g[keep].view(np.uint64), ref_g[keep].view(np.uint64))
    assert np.array_equal(got_e[keep].view(np.uint32), ref_e[keep].view(np.uint32))


def test_bitwise_invariances(gpu):
    """Two calls; an inner block of chains read in place against its copy; the steps in two calls against one; and
    elem_lp = NULL."""
    from autoreparam_amd import _lib, models
    spec = models._spec_time_series()
    D = spec.D
    up = upload(gpu, spec.site_table(), D)
    wide = torch.as_tensor(draws(2, 50, D, 5), device=gpu)
    same = lambda a, b: np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[2], b[2]) and (
        (a[1] is None or b[1] is None) or np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))
    a = run(gpu, wide, up)
    assert same(a, run(gpu, wide, up))
    block = wide[:, 8:40]
    view = _lib.trace_view(block, "test")
    assert view[0].data_ptr() == block.data_ptr() and view[4] == 50 * D
    b = run(gpu, block, up)
    assert same(b, run(gpu, block.contiguous(), up))
    first, second = run(gpu, wide[0:1], up), run(gpu, wide[1:2], up)
    assert np.array_equal(np.concatenate([first[0], second[0]]).view(np.uint64), a[0].view(np.uint64))
    assert np.array_equal(np.concatenate([first[1], second[1]]).view(np.uint32), a[1].view(np.uint32))
    assert same(a, run(gpu, wide, up, want_elements=False))
    for group_of in (np.arange(D) % 7, np.zeros(D, np.int64)):
        assert same(run(gpu, wide, up, group_of), run(gpu, wide, up, group_of, want_elements=False))


def test_refusals(gpu):
    from autoreparam_amd import _lib, diagnostics
    L = _lib.lib()
    D = 8
    up = upload(gpu, synthetic(D), D)
    x = torch.zeros(2, 3, D, device=gpu)
    group_lp = torch.zeros(6, 2, dtype=torch.float64, device=gpu)
    elem_lp = torch.zeros(6, D, device=gpu)
    mask = torch.zeros(6, dtype=torch.uint8, device=gpu)
    cnt = torch.zeros((), dtype=torch.int64, device=gpu)
    group_of = torch.as_tensor((np.arange(D) % 2).astype(np.int32), device=gpu)
    p = _lib.ptr
    columns = ("form", "loc_idx", "loc_w", "loc0", "scale_idx", "scale_w", "log_scale0", "norm")

    def call(x_=x, S=2, Cn=3, D_=D, stride=3 * D, G=2, groups=group_of, out=group_lp, elems=elem_lp, mask_=mask, cnt_=cnt, **null):
        cols = [p(None if null.get(name) else getattr(up, name)) for name in columns]
        return L.arp_site_logprior(p(x_), S, Cn, D_, stride, *cols, p(groups), G, p(out), p(elems), p(mask_), p(cnt_), C.c_void_p(0))
    assert call() == 0 and call(elems=None) == 0
    torch.cuda.synchronize()
    cases = [(dict(x_=None), b"required"), (dict(groups=None), b"required"), (dict(out=None), b"required"),
             (dict(mask_=None), b"required"), (dict(cnt_=None), b"required")]
    cases += [({name: True}, b"required") for name in columns]
    cases += [(dict(D_=0), b"1 <= D <= 255"), (dict(D_=256), b"1 <= D <= 255"), (dict(S=0), b"n_samples"), (dict(Cn=0), b"n_chains"),
              (dict(S=1 << 20, Cn=1 << 20), b"2^31"), (dict(stride=3 * D - 1), b"row_stride"), (dict(G=0), b"1 <= G <= D"),
              (dict(G=D + 1), b"1 <= G <= D")]
    before = group_lp.clone()
    for kwargs, word in cases:
        assert call(**kwargs) != 0, kwargs
        assert word in L.arp_last_error(), (kwargs, L.arp_last_error())
    torch.cuda.synchronize()
    assert torch.equal(before, group_lp)
    with pytest.raises(ValueError, match="group_of must be"):
        diagnostics.site_logprior(x, up, np.full(D, D))
    with pytest.raises(ValueError, match="group_of must be"):
        diagnostics.site_logprior(x, up, np.zeros(D - 1, np.int64))
    with pytest.raises(ValueError, match="the table 8"):
        diagnostics.site_logprior(torch.zeros(2, 3, 9, device=gpu), up)
