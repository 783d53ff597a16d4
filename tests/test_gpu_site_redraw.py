"""GPU: arp_site_redraw (csrc/site_redraw.hip) through diagnostics.site_redraw against the float64 restatement of
tests/site_redraw_ref.py, teacher-forced on the device's own output rows: the flagged elements of every model's real site
table under its natural selection and of a synthetic table of D = 255 within the bound of arp_site_prior_draws' header
(undecided log-Gamma elements and what descends from them excluded, their share asserted), the unflagged ones equal to the
input bit for bit; the two exact invariants (every element flagged over NaN: arp_site_prior_draws; none: the input); the
shapes around the tile edge, both strides, the draw offset (above 2^32 too), blocks of steps, two calls, undrawn and NULL,
a shape that cannot be drawn; every refusal; and redraw and replication together against the closed form of 8 schools.
The inputs: tests/test_site_redraw_host.py -- recorded rows are site_prior_draws under INPUT_SEED, the redraw runs under
SEED at offset 0, whose undecided share the host test establishes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import prior_draw_ref as pr
import site_redraw_ref as rr
from test_prior_draw_host import DRAWS, KS_CRITICAL, SEED, UNDECIDED_CAP, erf, kolmogorov, one_element, synthetic_chain
from test_site_redraw_host import INPUT_SEED, parity_cases

pytestmark = pytest.mark.gpu

COLUMNS = ("form", "loc_idx", "loc_w", "loc0", "scale_idx", "scale_w", "log_scale0")
CASES = list(parity_cases())


def upload(gpu, table, D):
    from autoreparam_amd import diagnostics
    return diagnostics.upload_site_table(table, D, gpu)


def recorded(up, n, seed=INPUT_SEED):
    """[n, D] float32 on the device: rows to redraw, drawn from the table's own prior under another seed"""
    from autoreparam_amd import diagnostics
    x, undrawn = diagnostics.site_prior_draws(up, n, seed=seed)
    assert not bool(undrawn.any())
    return x


def run(up, trace, flags, seed=SEED, offset=0, out=None):
    """(rows [S C, D] float32, undrawn [S C] uint8) on the host"""
    from autoreparam_amd import diagnostics
    rows, undrawn = diagnostics.site_redraw(trace, up, flags, seed=seed, draw_offset=offset, out=out)
    return rows[:, :up.D].cpu().numpy(), undrawn.cpu().numpy()


def same(a, b):
    return a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(gpu, table, D, flags, what, n=DRAWS, shape=None, offset=0):
    """Flagged elements within the header's bound of the teacher-forced float64 value, unflagged ones the input's bits;
    returns the largest deviation / bound"""
    up = upload(gpu, table, D)
    flagged = np.asarray(flags) != 0
    x = recorded(up, n)
    S, Cn = shape or (1, n)
    assert S * Cn == n
    got, undrawn = run(up, x.view(S, Cn, D), flags, offset=offset)
    x = x.cpu().numpy()
    assert got.shape == (n, D) and got.dtype == np.float32 and not undrawn.any(), what
    assert same(got[:, ~flagged], x[:, ~flagged]), what
    ref = rr.redraw(up.host, x, flags, SEED, offset, parents=got)
    gamma = (np.asarray(up.host.form) == pr.LOG_GAMMA) & flagged
    marks = rr.undecided(up.host, ref, flags)
    out = rr.tainted(up.host, marks, flags)
    if gamma.any():
        share = float(marks[:, gamma].mean())
        print("%s: %d of %d flagged log-Gamma elements undecided (cap %g), %d elements excluded with their descendants" % (
            what, int(marks.sum()), int(gamma.sum()) * n, UNDECIDED_CAP, int(out.sum())))
        assert share <= UNDECIDED_CAP, (what, share)
    else:
        assert not out.any()
    assert not ref.undrawn.any() and np.isfinite(ref.x).all() and np.isfinite(got).all(), what
    allow = rr.bound(up.host, ref)
    assert np.isfinite(allow[:, flagged]).all() and (allow[:, flagged] >= 0).all(), what
    dev = np.abs(got.astype(np.float64) - ref.x)
    keep = flagged[None, :] & ~out
    ratio = float((dev[keep] / np.maximum(allow[keep], 2.0 ** -149)).max())
    print("%s: largest deviation / bound %.3f over %d redrawn elements" % (what, ratio, int(keep.sum())))
    assert (dev <= allow)[keep].all(), (what, ratio)
    assert not same(got[:, flagged], x[:, flagged]), what                    # (they WERE redrawn)
    return ratio


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_parity_at_every_table_and_selection(gpu, case):
    what, table, D, flags = CASES[case]
    check(gpu, table, D, flags, what)


@pytest.mark.parametrize("form,loc0", ((0, 0.3), (1, -0.2), (2, 0.5)))
def test_one_element(gpu, form, loc0):
    check(gpu, one_element(form, loc0, 0.4), 1, np.ones(1, np.uint8), "D=1 form %d" % form, n=65)


@pytest.mark.parametrize("shape", ((1, 1), (1, 63), (1, 64), (1, 65), (5, 13), (7, 9), (3, 43), (65, 1)))
def test_draw_counts_around_the_tile_edge(gpu, shape):
    """An even D, whose pitch is padded, the tail flagged, as [1, R] and as [S, C] with S C off the tile edge, at an offset
    above 2^32"""
    flags = (np.arange(12) >= 5).astype(np.uint8)
    check(gpu, synthetic_chain(12), 12, flags, "D=12 %dx%d" % shape, n=shape[0] * shape[1], shape=shape, offset=(1 << 32) + 7)


@pytest.mark.parametrize("name,D,shape", (("synthetic", 255, (2, 65)), ("synthetic", 12, (5, 13)), ("german_credit_gammascale", 125, (1, 200))))
def test_every_element_flagged_over_nan_is_the_prior_draw(gpu, name, D, shape):
    """Flagged columns of x never enter a result: over an input of NaN the rows are arp_site_prior_draws', bit for bit"""
    from autoreparam_amd import diagnostics, models
    table = synthetic_chain(D) if name == "synthetic" else models._spec_german_gammascale().site_table()
    up = upload(gpu, table, D)
    n = shape[0] * shape[1]
    nan = torch.full(shape + (D,), float("nan"), dtype=torch.float32, device=gpu)
    for offset in (0, 1000, (1 << 32) + 3):
        want, want_undrawn = diagnostics.site_prior_draws(up, n, seed=SEED, draw_offset=offset)
        got, undrawn = run(up, nan, np.ones(D, np.uint8), offset=offset)
        assert same(got, want.cpu().numpy()) and np.array_equal(undrawn, want_undrawn.cpu().numpy()) and np.isfinite(got).all()


def test_no_element_flagged_is_the_input(gpu):
    D, n = 13, 70
    up = upload(gpu, synthetic_chain(D), D)
    x = recorded(up, n)
    x[3, 4], x[3, 7], x[64, 0], x[69, 12] = float("inf"), float("nan"), float("-inf"), -0.0
    got, undrawn = run(up, x.view(1, n, D), np.zeros(D, np.uint8))
    assert same(got, x.cpu().numpy()) and not undrawn.any()
    # ... and a NaN in a recorded parent is a value like any other: its flagged descendants are NaN, the rest is drawn
    flags = (np.arange(D) >= 8).astype(np.uint8)
    got, undrawn = run(up, x.view(1, n, D), flags)
    assert same(got[:, :8], x.cpu().numpy()[:, :8]) and np.isnan(got[3, 8]) and np.isfinite(got[np.arange(n) != 3][:, 8:]).all()
    assert not undrawn.any()


def test_row_stride_leaves_the_padding_alone(gpu):
    """A leading block of chains of a wider trace is read in place: rows C D floats wide, K D apart; what lies between is
    never read (NaN there changes nothing) and never written"""
    D, S, Cn, K = 12, 5, 13, 16
    up = upload(gpu, synthetic_chain(D), D)
    flags = (np.arange(D) % 2).astype(np.uint8)
    x = recorded(up, S * Cn).view(S, Cn, D)
    wide = torch.full((S, K, D), float("nan"), dtype=torch.float32, device=gpu)
    wide[:, :Cn] = x
    block = wide[:, :Cn]
    assert not block.is_contiguous() and block.stride(0) == K * D
    before = wide.clone()
    got, _ = run(up, block, flags)
    assert same(got, run(up, x, flags)[0]) and np.isfinite(got).all()
    assert torch.equal(wide.view(torch.int32), before.view(torch.int32))


def test_out_stride_leaves_the_padding_alone(gpu):
    D, n = 13, 65
    up = upload(gpu, synthetic_chain(D), D)
    flags = (np.arange(D) >= 4).astype(np.uint8)
    x = recorded(up, n).view(5, 13, D)
    wide = torch.full((n, D + 3), -7.25, dtype=torch.float32, device=gpu)
    got, _ = run(up, x, flags, out=wide)
    assert torch.all(wide[:, D:] == -7.25) and same(got, run(up, x, flags)[0]) and np.isfinite(got).all()
    part = wide[:, :D]                                                       # rows D + 3 apart, D columns wide
    part.fill_(0.0)
    got_part, _ = run(up, x, flags, out=part)
    assert same(got_part, got) and torch.all(wide[:, D:] == -7.25)


def test_blocks_of_steps_offsets_two_calls_and_undrawn(gpu):
    from autoreparam_amd import _lib
    D, S, Cn = 40, 15, 71                                                    # 1 065 draws
    up = upload(gpu, synthetic_chain(D), D)
    flags = (np.arange(D) >= 11).astype(np.uint8)
    x = recorded(up, S * Cn).view(S, Cn, D)
    base = (1 << 32) - 500                                                   # the block below straddles 2^32
    whole, undrawn = run(up, x, flags, offset=base)
    assert not undrawn.any() and undrawn.dtype == np.uint8 and undrawn.shape == (S * Cn,)
    assert same(whole, run(up, x, flags, offset=base)[0])                    # two calls
    for s0, s1 in ((0, 1), (4, 9), (14, 15)):                                # steps [s0, s1) at offset s0 C: those rows of the whole
        assert same(run(up, x[s0:s1], flags, offset=base + s0 * Cn)[0], whole[s0 * Cn:s1 * Cn]), (s0, s1)
    assert same(run(up, x.view(1, S * Cn, D), flags, offset=base)[0], whole)  # the shape of the block does not enter
    assert not same(run(up, x[4:9], flags, offset=base + 4 * Cn + (1 << 32))[0], whole[4 * Cn:9 * Cn])     # hi32 g is in the counter
    assert not same(run(up, x, flags, seed=SEED ^ (1 << 40), offset=base)[0], whole)                       # hi32 of the seed is in the key
    # undrawn = NULL leaves out bitwise the same
    out = torch.zeros(S * Cn, D, dtype=torch.float32, device=gpu)
    dflags = torch.as_tensor(flags, device=gpu)
    cols = [_lib.ptr(getattr(up, name)) for name in COLUMNS]
    rc = _lib.lib().arp_site_redraw(_lib.ptr(x), S, Cn, D, Cn * D, *cols, _lib.ptr(dflags), SEED, base, _lib.ptr(out), D,
                                    C.c_void_p(0), C.c_void_p(0))
    torch.cuda.synchronize()
    assert rc == 0 and same(out.cpu().numpy(), whole)


def test_a_shape_that_cannot_be_drawn_is_nan_and_the_rest_is_drawn(gpu):
    """k <= 0 gives NaN there and in its flagged descendants; what does not hang on it is drawn or kept as ever"""
    table = synthetic_chain(6)
    table.loc0[2] = -1.0                                                     # element 2 is log-Gamma; 3 and 4 hang on it
    table.loc_w[5], table.scale_w[5] = 0.0, 0.0
    table.loc_idx[5], table.scale_idx[5] = 0, 0                              # (a term of weight 0 still multiplies its parent)
    up = upload(gpu, table, 6)
    x = torch.as_tensor(np.random.RandomState(6).randn(1, 70, 6).astype(np.float32), device=gpu)
    got, undrawn = run(up, x, np.array([0, 0, 1, 1, 1, 1], np.uint8))
    assert np.isnan(got[:, 2:5]).all() and np.isfinite(got[:, 5]).all() and not undrawn.any()
    assert same(got[:, :2], x.cpu().numpy()[0, :, :2])
    # with 2 kept as recorded, its descendants are drawn from the recorded value
    got, undrawn = run(up, x, np.array([0, 0, 0, 1, 1, 1], np.uint8))
    assert np.isfinite(got).all() and same(got[:, :3], x.cpu().numpy()[0, :, :3]) and not undrawn.any()


def test_refusals(gpu):
    from autoreparam_amd import _lib, diagnostics
    L = _lib.lib()
    D, S, Cn = 8, 2, 3
    n = S * Cn
    up = upload(gpu, synthetic_chain(D), D)
    x = torch.zeros(S, Cn, D, dtype=torch.float32, device=gpu)
    out = torch.full((n, D), 3.5, dtype=torch.float32, device=gpu)
    undrawn = torch.full((n,), 9, dtype=torch.uint8, device=gpu)
    dflags = torch.ones(D, dtype=torch.uint8, device=gpu)

    def call(x_=x, S_=S, C_=Cn, D_=D, stride=Cn * D, redraw=dflags, offset=0, out_=out, out_stride=D, marks=undrawn, **null):
        cols = [_lib.ptr(None if null.get(name) else getattr(up, name)) for name in COLUMNS]
        return L.arp_site_redraw(_lib.ptr(x_), S_, C_, D_, stride, *cols, _lib.ptr(redraw), SEED, offset, _lib.ptr(out_), out_stride,
                                 _lib.ptr(marks), C.c_void_p(0))
    cases = [(dict(x_=None), b"required"), (dict(redraw=None), b"required"), (dict(out_=None), b"required")]
    cases += [({name: True}, b"required") for name in COLUMNS]
    cases += [(dict(D_=0), b"1 <= D <= 255"), (dict(D_=256), b"1 <= D <= 255"), (dict(S_=0), b"n_samples > 0"),
              (dict(C_=0), b"n_chains > 0"), (dict(S_=1 << 31), b"2^31 - 1 draws"), (dict(stride=Cn * D - 1), b"row_stride"),
              (dict(S_=1 << 12, C_=(1 << 12) + 1, stride=((1 << 12) + 1) * D), b"2^24 draws"),
              (dict(out_stride=D - 1), b"out_stride"), (dict(offset=-1), b"draw_offset"), (dict(out_=x), b"out must not be x")]
    for kwargs, word in cases:
        assert call(**kwargs) == 1, kwargs
        assert word in L.arp_last_error(), (kwargs, L.arp_last_error())
    torch.cuda.synchronize()
    assert torch.all(out == 3.5) and torch.all(undrawn == 9) and torch.all(x == 0)      # nothing was launched
    assert call() == 0 and call(marks=None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.all(undrawn == 0)
    flags = np.ones(D, np.uint8)
    with pytest.raises(ValueError, match="draw_offset"):
        diagnostics.site_redraw(x, up, flags, draw_offset=-1)
    with pytest.raises(ValueError, match=r"redraw must be \[8\] flags"):
        diagnostics.site_redraw(x, up, flags[:7])
    with pytest.raises(ValueError, match="the trace has 7 elements, the table 8"):
        diagnostics.site_redraw(x[:, :, :7].contiguous(), up, flags)
    with pytest.raises(ValueError, match="float32 .n_draws, >= D. matrix"):
        diagnostics.site_redraw(x, up, flags, out=torch.zeros(n, D - 1, device=gpu))
    with pytest.raises(ValueError, match="float32 .n_draws, >= D. matrix"):
        diagnostics.site_redraw(x, up, flags, out=torch.zeros(n + 1, D, device=gpu))
    with pytest.raises(ValueError, match="out must not be the trace"):
        diagnostics.site_redraw(x, up, flags, out=x.view(n, D))
    with pytest.raises(ValueError, match="on the GPU"):
        diagnostics.site_redraw(x.cpu(), up, flags)


def test_eight_schools_redraw_and_replication_against_the_closed_form(gpu):
    """What the mixed check sees and the posterior check cannot.  Every recorded row is mu = 4, log_tau = log 10,
    theta = y; theta is redrawn and the data replicated from the rows (R = 65 536).  (theta' - mu) / tau is standard normal:
    8 R values against Phi at the 0.001 critical value.  The mixed predictive distribution of school j is
    N(mu, tau^2 + sigma_j^2): the mean PIT over the draws is within 0.01 of Phi((y_j - mu) / sqrt(tau^2 + sigma_j^2)) -- a
    PIT lies in [0, 1], so its standard error is at most 0.5 / sqrt(R) = 0.00195, and 0.01 is five of those -- and the
    predictive mean within 5 tau / sqrt(R) of mu (its standard error is tau / sqrt(R)).  On the recorded rows themselves
    theta = y and the PIT is EXACTLY 0.5 for every school, whatever y is."""
    from autoreparam_amd import diagnostics, models
    from autoreparam_amd.report_common import next_seed, replicate_tiles
    spec = models._spec_eight_schools()
    R, D = 65536, spec.D
    y, sigma = np.asarray(spec.raw["y"], np.float64).reshape(-1), np.asarray(spec.raw["sigma"], np.float64).reshape(-1)
    assert spec.part_names == ["mu", "log_tau", "theta"] and D == 10
    row = np.concatenate([[4.0, math.log(10.0)], y]).astype(np.float32)
    mu, tau = float(row[0]), math.exp(float(row[1]))
    x = torch.as_tensor(np.tile(row, (R, 1)), device=gpu)
    site = upload(gpu, spec.site_table(), D)
    table = diagnostics.upload_table(spec.observation_table(), D, gpu)
    flags = diagnostics.redraw_selection(spec.site_table(), spec.part_names, ["theta"])
    rows, undrawn = diagnostics.site_redraw(x.view(256, 256, D), site, flags, seed=SEED)
    assert not bool(undrawn.any()) and torch.equal(rows[:, :2], x[:, :2])
    z = ((rows[:, 2:].cpu().numpy().astype(np.float64) - mu) / tau).reshape(-1)
    ks = kolmogorov(z, lambda v: 0.5 * (1.0 + erf(v / math.sqrt(2.0))))
    print("8 schools: Kolmogorov distance of (theta' - mu) / tau from the normal %.5f, allowed %.5f" % (ks, KS_CRITICAL / math.sqrt(z.size)))
    assert z.size == 8 * R and ks < KS_CRITICAL / math.sqrt(z.size)
    stats, sums, mask = replicate_tiles(rows[None], table, next_seed(SEED))
    mixed = diagnostics.ppc_summary(stats.cpu().numpy(), sums.cpu().numpy(), table.y_host, table.kind, mask.cpu().numpy())
    want = 0.5 * (1.0 + erf((y - mu) / np.sqrt(tau * tau + sigma * sigma) / math.sqrt(2.0)))
    print("8 schools: mixed PIT %s against %s; predictive mean within %.4f of mu (allowed %.4f)" % (
        np.round(mixed.pit, 4), np.round(want, 4), float(np.max(np.abs(mixed.predictive_mean - mu))), 5.0 * tau / math.sqrt(R)))
    assert mixed.draws_used == R and mixed.draws_left_out == 0
    assert np.all(np.abs(mixed.pit - want) <= 0.01)
    assert np.all(np.abs(mixed.predictive_mean - mu) <= 5.0 * tau / math.sqrt(R))
    stats, sums, mask = replicate_tiles(x[None], table, next_seed(SEED))
    posterior = diagnostics.ppc_summary(stats.cpu().numpy(), sums.cpu().numpy(), table.y_host, table.kind, mask.cpu().numpy())
    assert np.all(posterior.pit == 0.5) and np.max(np.abs(want - 0.5)) > 0.25
