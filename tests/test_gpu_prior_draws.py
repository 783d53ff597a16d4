"""GPU: arp_site_prior_draws (csrc/prior_draw.hip) through diagnostics.site_prior_draws against the float64 restatement of
tests/prior_draw_ref.py, teacher-forced on the device's own float32 parents: every element of the nine models' real site
tables, of a synthetic table of D = 255 whose elements hang on the two before them through loc and scale, and of
one-element tables, within the header's first-order bound -- undecided log-Gamma elements and what descends from them
excluded, their share asserted; the shapes around the tile edge, the row stride, the draw offset (above 2^32 too), two
calls, undrawn and NULL; every refusal; and the draws against their twin arp_site_logprior and against the distribution
they are meant to have.  The inputs: tests/test_prior_draw_host.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import prior_draw_ref as pr
from test_prior_draw_host import DRAWS, KS_CRITICAL, MODELS, SEED, UNDECIDED_CAP, erf, kolmogorov, one_element, synthetic_chain
from test_site_table_host import SPECS

pytestmark = pytest.mark.gpu


def upload(gpu, table, D):
    from autoreparam_amd import diagnostics
    return diagnostics.upload_site_table(table, D, gpu)


def run(up, n, seed=SEED, offset=0, out=None):
    """(x [n, D] float32, undrawn [n] uint8) on the host"""
    from autoreparam_amd import diagnostics
    x, undrawn = diagnostics.site_prior_draws(up, n, seed=seed, draw_offset=offset, out=out)
    return x[:, :up.D].cpu().numpy(), undrawn.cpu().numpy()


def same(a, b):
    return a.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(gpu, table, D, n, what, offset=0):
    """Every element within the header's bound of the teacher-forced float64 value; returns the largest deviation / bound"""
    up = upload(gpu, table, D)
    got, undrawn = run(up, n, offset=offset)
    assert got.shape == (n, D) and got.dtype == np.float32 and not undrawn.any(), what
    ref = pr.draw(up.host, n, SEED, offset, parents=got)
    gamma = np.asarray(up.host.form) == pr.LOG_GAMMA
    marks = pr.undecided(up.host, ref)
    out = pr.tainted(up.host, marks)
    if gamma.any():
        share = float(marks[:, gamma].mean())
        print("%s: %d of %d log-Gamma elements undecided (cap %g), %d elements excluded with their descendants" % (
            what, int(marks.sum()), int(gamma.sum()) * n, UNDECIDED_CAP, int(out.sum())))
        assert share <= UNDECIDED_CAP, (what, share)
    else:
        assert not out.any()
    assert not ref.undrawn.any() and np.isfinite(ref.x).all() and np.isfinite(got).all(), what
    allow = pr.bound(up.host, ref)
    assert np.isfinite(allow).all() and (allow >= 0).all(), what             # (0: an element that is exactly 0 = 0 + 1 * 0)
    dev = np.abs(got.astype(np.float64) - ref.x)
    ratio = float((dev[~out] / np.maximum(allow[~out], 2.0 ** -149)).max())
    print("%s: largest deviation / bound %.3f over %d elements" % (what, ratio, int((~out).sum())))
    assert (dev <= allow)[~out].all(), (what, ratio)
    return ratio


@pytest.mark.parametrize("name", MODELS)
def test_every_model_at_its_real_table(gpu, name):
    from autoreparam_amd import models
    spec = SPECS[name](models)
    check(gpu, spec.site_table(), spec.D, DRAWS, name)


def test_widest_state_with_every_form_on_its_two_predecessors(gpu):
    check(gpu, synthetic_chain(255), 255, DRAWS, "synthetic D=255")


@pytest.mark.parametrize("form,loc0", ((0, 0.3), (1, -0.2), (2, 0.5)))
def test_one_element(gpu, form, loc0):
    check(gpu, one_element(form, loc0, 0.4), 1, DRAWS, "D=1 form %d" % form)


@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_draw_counts_around_the_tile_edge(gpu, n):
    """(4 096 draws: the tests above.)  An even D, whose pitch is padded, and an offset above 2^32."""
    check(gpu, synthetic_chain(12), 12, n, "D=12 n=%d" % n, offset=(1 << 32) + 7)


def test_row_stride_leaves_the_padding_alone(gpu):
    D, n = 13, 65
    up = upload(gpu, synthetic_chain(D), D)
    wide = torch.full((n, D + 3), -7.25, dtype=torch.float32, device=gpu)
    got, _ = run(up, n, out=wide)
    assert torch.all(wide[:, D:] == -7.25) and same(got, run(up, n)[0]) and np.isfinite(got).all()
    part = wide[:, :D]                                                       # rows D + 3 apart, D columns wide
    assert part.stride(0) == D + 3
    part.fill_(0.0)
    got_part, _ = run(up, n, out=part)
    assert same(got_part, got) and torch.all(wide[:, D:] == -7.25)


def test_offsets_two_calls_and_undrawn(gpu):
    from autoreparam_amd import _lib
    spec_table = synthetic_chain(40)
    up = upload(gpu, spec_table, 40)
    whole, undrawn = run(up, 1065)
    assert not undrawn.any() and undrawn.dtype == np.uint8 and undrawn.shape == (1065,)
    assert same(whole, run(up, 1065)[0])                                     # two calls
    assert same(run(up, 65, offset=1000)[0], whole[1000:1065])               # rows [0, 65) at offset 1000
    high = (1 << 32) + 1000
    far = run(up, 65, offset=high)[0]
    assert not same(far, whole[1000:1065])                                   # hi32 g is part of the counter
    assert same(run(up, 64, offset=high + 1)[0], far[1:])
    assert not same(run(up, 65, seed=SEED ^ (1 << 40), offset=1000)[0], whole[1000:1065])      # hi32 of the seed is part of the key
    # undrawn = NULL leaves x bitwise the same
    x = torch.zeros(1065, 40, dtype=torch.float32, device=gpu)
    cols = [_lib.ptr(getattr(up, name)) for name in ("form", "loc_idx", "loc_w", "loc0", "scale_idx", "scale_w", "log_scale0")]
    rc = _lib.lib().arp_site_prior_draws(40, *cols, 1065, SEED, 0, _lib.ptr(x), 40, C.c_void_p(0), C.c_void_p(0))
    torch.cuda.synchronize()
    assert rc == 0 and same(x.cpu().numpy(), whole)


def test_a_shape_that_cannot_be_drawn_is_nan_and_the_rest_is_drawn(gpu):
    """k <= 0 gives NaN without an attempt; what does not hang on it is drawn as ever"""
    table = synthetic_chain(6)
    table.loc0[2] = -1.0                                                     # element 2 is log-Gamma; 3 and 4 hang on it
    table.loc_w[5], table.scale_w[5] = 0.0, 0.0
    table.loc_idx[5], table.scale_idx[5] = 0, 0                              # (a term of weight 0 still multiplies its parent)
    up = upload(gpu, table, 6)
    got, undrawn = run(up, 70)
    assert np.isnan(got[:, 2]).all() and np.isnan(got[:, 3]).all() and np.isfinite(got[:, (0, 1)]).all() and not undrawn.any()
    assert np.isfinite(got[:, 5]).all()


def test_refusals(gpu):
    from autoreparam_amd import _lib, diagnostics
    L = _lib.lib()
    D, n = 8, 6
    up = upload(gpu, synthetic_chain(D), D)
    x = torch.full((n, D), 3.5, dtype=torch.float32, device=gpu)
    undrawn = torch.full((n,), 9, dtype=torch.uint8, device=gpu)
    columns = ("form", "loc_idx", "loc_w", "loc0", "scale_idx", "scale_w", "log_scale0")

    def call(D_=D, n_=n, offset=0, x_=x, stride=D, flags=undrawn, **null):
        cols = [_lib.ptr(None if null.get(name) else getattr(up, name)) for name in columns]
        return L.arp_site_prior_draws(D_, *cols, n_, SEED, offset, _lib.ptr(x_), stride, _lib.ptr(flags), C.c_void_p(0))
    cases = [(dict(x_=None), b"required")] + [({name: True}, b"required") for name in columns]
    cases += [(dict(D_=0), b"1 <= D <= 255"), (dict(D_=256), b"1 <= D <= 255"), (dict(n_=0), b"n_draws"),
              (dict(n_=(1 << 24) + 1), b"n_draws"), (dict(stride=D - 1), b"row_stride"), (dict(offset=-1), b"draw_offset")]
    for kwargs, word in cases:
        assert call(**kwargs) == 1, kwargs
        assert word in L.arp_last_error(), (kwargs, L.arp_last_error())
    torch.cuda.synchronize()
    assert torch.all(x == 3.5) and torch.all(undrawn == 9)                   # nothing was launched
    assert call() == 0 and call(flags=None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(x).all() and torch.all(undrawn == 0)
    with pytest.raises(ValueError, match="1 <= draws"):
        diagnostics.site_prior_draws(up, 0)
    with pytest.raises(ValueError, match="draw_offset"):
        diagnostics.site_prior_draws(up, 4, draw_offset=-1)
    with pytest.raises(ValueError, match="float32 .n_draws, >= D. matrix"):
        diagnostics.site_prior_draws(up, 4, out=torch.zeros(4, D - 1, device=gpu))
    with pytest.raises(ValueError, match="float32 .n_draws, >= D. matrix"):
        diagnostics.site_prior_draws(up, 4, out=torch.zeros(5, D, device=gpu))


def test_eight_schools_draws_against_the_twin_and_the_normal(gpu):
    """site_logprior of the kernel's draws is finite on every draw, and (theta - mu) exp(-log_tau) is standard normal:
    4 096 x 8 values against Phi at the 0.001 critical value"""
    from autoreparam_amd import diagnostics, models
    spec = models._spec_eight_schools()
    up = upload(gpu, spec.site_table(), spec.D)
    x, undrawn = diagnostics.site_prior_draws(up, DRAWS, seed=SEED)
    group_lp, elem_lp, mask, count = diagnostics.site_logprior(x[None], up, want_elements=True)
    assert int(count.item()) == 0 and not mask.any() and not undrawn.any()
    assert torch.isfinite(group_lp).all() and torch.isfinite(elem_lp).all()
    parts = dict(zip(spec.part_names, spec.unpack(x.cpu().numpy().astype(np.float64))))
    z = ((parts["theta"] - parts["mu"].reshape(-1, 1)) * np.exp(-parts["log_tau"].reshape(-1, 1))).reshape(-1)
    assert z.size == DRAWS * 8
    ks = kolmogorov(z, lambda v: 0.5 * (1.0 + erf(v / math.sqrt(2.0))))
    print("8 schools: Kolmogorov distance of (theta - mu) / tau from the normal %.5f, allowed %.5f" % (ks, KS_CRITICAL / math.sqrt(z.size)))
    assert ks < KS_CRITICAL / math.sqrt(z.size)
