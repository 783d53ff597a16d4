"""GPU: arp_pointwise_loglik (csrc/loglik.hip) through diagnostics.pointwise_loglik against the float64 model programs of
tests/loglik_ref.py: every model with data at its real dataset within twice the header's first-order bound, synthetic
tables at the shape edges, a trace read in place, the stable Bernoulli form, masked draws, refusals.

Measured on an MI355X (largest deviation / allowance over the real datasets): DESIGN.md section 6."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

import loglik_ref as lr
from test_loo_host import TABLE_SPECS, table_predictor

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
Table = collections.namedtuple("Table", ("kind", "idx", "w", "y", "scale_idx", "log_scale"))
# a plausible centre per model (trace order is the spec's): radon-like effects near 1, log-scales near 0, CO2 levels
CENTRES = {"time_series": lambda sp: _time_series_centre(sp)}


def _time_series_centre(sp):
    c = np.zeros(sp.D)
    y = np.asarray(sp.raw["y"], np.float64)
    for t in range(len(y)):
        c[sp.part_names.index("alpha%d" % t)] = y[t]
    return c


def bound(kind, T, A, eta, s, y, ll):
    """The header's first-order bound of |ll_dev - ll|, from float64 quantities."""
    if kind == lr.NORMAL:
        z = (y - eta) * np.exp(-s)
        return U * (T * A * np.exp(-s) * np.abs(z) + z * z * (5.0 + np.abs(s)) + 3.0 * np.abs(s) + np.abs(ll))
    sp = np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta)))
    return U * (T * A * (np.abs(y) + 1.0) + np.abs(y * eta) + 3.0 + sp + np.abs(ll))


def run(gpu, x3, table, n0=0, n1=None, D=None):
    """(ll [n1 - n0, R], mask [R], count) on the host for a [S, C, D] float32 numpy trace or device tensor."""
    from autoreparam_amd import diagnostics
    xd = x3 if torch.is_tensor(x3) else torch.as_tensor(np.ascontiguousarray(x3, np.float32), device=gpu)
    dt = diagnostics.upload_table(table, int(xd.shape[2]) if D is None else D, gpu)
    ll, mask, count = diagnostics.pointwise_loglik(xd, dt, n0, n1)
    return ll.cpu().numpy(), mask.cpu().numpy(), int(count.item())


def check_table(gpu, table, x3, n0=0, n1=None, what=""):
    """Device ll of observations [n0, n1) within twice the bound of the float64 value of the same table; returns the
    largest deviation / allowance."""
    S, Cn, D = x3.shape
    N, T = table.idx.shape
    n1 = N if n1 is None else n1
    got, mask, count = run(gpu, x3, table, n0, n1)
    x = np.asarray(x3, np.float32).reshape(S * Cn, D).astype(np.float64)
    eta, s = table_predictor(table, x)
    A = np.einsum("nt,rnt->rn", np.abs(table.w.astype(np.float64)), np.abs(x[:, table.idx]))
    y = table.y.astype(np.float64)
    ref = lr.loglik_from(table.kind, eta, s, y)
    allow = 2.0 * bound(table.kind, T, A, eta, s, y[None, :], ref)
    assert got.shape == (n1 - n0, S * Cn) and count == 0 and not mask.any(), what
    assert np.isfinite(got).all(), what
    dev = np.abs(got.T.astype(np.float64) - ref[:, n0:n1])
    assert (dev <= allow[:, n0:n1]).all(), (what, float((dev / allow[:, n0:n1]).max()))
    return float((dev / allow[:, n0:n1]).max())


@pytest.mark.parametrize("name", sorted(TABLE_SPECS))
def test_every_model_at_its_real_dataset(gpu, name):
    """Draw counts 1, 63, 64, 65 and 300 as 1 ... 5 steps of a few chains, states N(0, 0.5) around a plausible point; the
    reference is loglik_ref's model program on the frozen data (not the table), the allowance twice the header's bound
    evaluated with the table's T and sum |w x|."""
    from autoreparam_amd import models
    spec = TABLE_SPECS[name](models)
    table = spec.observation_table()
    N, T = table.idx.shape
    centre = CENTRES[name](spec) if name in CENTRES else np.zeros(spec.D)
    worst = 0.0
    for S, Cn in ((1, 1), (1, 63), (2, 32), (5, 13), (5, 60)):
        rs = np.random.RandomState(1000 * S + Cn)
        x3 = (centre + 0.5 * rs.randn(S, Cn, spec.D)).astype(np.float32)
        got, mask, count = run(gpu, x3, table)
        x = x3.reshape(S * Cn, spec.D).astype(np.float64)
        kind, eta, s, y = lr.predictor(spec, x)
        ref = lr.loglik_from(kind, eta, s, y)
        A = np.einsum("nt,rnt->rn", np.abs(table.w.astype(np.float64)), np.abs(x[:, table.idx]))
        allow = 2.0 * bound(kind, T, A, eta, s, y[None, :], ref)
        assert got.shape == (N, S * Cn) and count == 0 and not mask.any()
        dev = np.abs(got.T.astype(np.float64) - ref)
        ratio = float((dev / allow).max())
        print("%s R=%d: largest deviation / allowance %.3f" % (name, S * Cn, ratio))
        assert (dev <= allow).all(), (name, S, Cn, ratio)
        worst = max(worst, ratio)
    print("%s: worst %.3f" % (name, worst))


def synthetic(N, T, D, kind, seed, scale):
    """A table whose idx hits 0 and D - 1, with padding terms, and a scale latent on every other observation."""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, D, size=(N, T)).astype(np.int32)
    idx[0, 0], idx[-1, -1] = 0, D - 1
    idx[:, T // 2] = D - 1
    w = rs.randn(N, T).astype(np.float32)
    if T > 2:
        w[1::3, -1] = 0.0
        idx[1::3, -1] = 0
    y = rs.randn(N).astype(np.float32) if kind == lr.NORMAL else (rs.rand(N) < 0.5).astype(np.float32)
    si = np.full(N, -1, np.int32)
    if scale:
        si[::2] = rs.randint(0, D, size=si[::2].shape)
        si[0] = D - 1
    return Table(kind, idx, w, y, si, (0.3 * rs.randn(N)).astype(np.float32))


@pytest.mark.parametrize("T", (1, 62, 65))
@pytest.mark.parametrize("D", (1, 33, 125, 255))
def test_synthetic_tables_at_the_shape_edges(gpu, T, D):
    """T below, at and past German credit's; D = 1, odd, German credit's and the widest; both likelihoods; the scale latent
    set and unset; an observation range with ragged ends; 130 draws = two full tiles and a ragged one."""
    for kind in (lr.NORMAL, lr.BERNOULLI):
        for scale in (False, True):
            table = synthetic(23, T, D, kind, 100 * T + D, scale)
            rs = np.random.RandomState(T + D)
            x3 = (0.5 * rs.randn(2, 65, D)).astype(np.float32)
            check_table(gpu, table, x3, what=(T, D, kind, scale, "all"))
            check_table(gpu, table, x3, 3, 20, what=(T, D, kind, scale, "ragged"))
            check_table(gpu, table, x3, 22, 23, what=(T, D, kind, scale, "last"))


def test_block_of_chains_read_in_place_is_bitwise_its_copy(gpu):
    """row_stride > n_chains * D: an inner block of chains of a wider trace, at an odd offset."""
    from autoreparam_amd import _lib
    table = synthetic(17, 5, 33, lr.NORMAL, 9, True)
    rs = np.random.RandomState(11)
    wide = torch.as_tensor((0.5 * rs.randn(4, 50, 33)).astype(np.float32), device=gpu)
    block = wide[:, 7:44]
    x, S, Cn, D, stride = _lib.trace_view(block, "test")
    assert x.data_ptr() == block.data_ptr() and stride == 50 * 33 and stride > Cn * D
    a, mask_a, _ = run(gpu, block, table)
    b, mask_b, _ = run(gpu, block.contiguous(), table)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(mask_a, mask_b)
    check_table(gpu, table, block.contiguous().cpu().numpy(), what="block")


def test_bernoulli_is_stable_at_large_logits(gpu):
    """eta = +-80: exp(80) overflows no float32 here because the form is max(eta, 0) + log1p(exp(-|eta|))."""
    table = Table(lr.BERNOULLI, np.zeros((4, 1), np.int32), np.array([[1.0], [1.0], [-1.0], [-1.0]], np.float32),
                  np.array([1.0, 0.0, 1.0, 0.0], np.float32), np.full(4, -1, np.int32), np.zeros(4, np.float32))
    x3 = np.full((1, 3, 1), 80.0, np.float32)
    got, mask, count = run(gpu, x3, table)
    ref = lr.loglik_from(lr.BERNOULLI, np.array([80.0, 80.0, -80.0, -80.0]), 0.0, table.y.astype(np.float64))
    assert np.isfinite(got).all() and count == 0
    assert np.all(np.abs(got[:, 0] - ref) <= 2.0 * U * (2.0 * 80.0 + 3.0 + np.abs(ref))), (got[:, 0], ref)
    assert np.array_equal(got[:, 0], got[:, 2])


def test_masked_draws_are_counted_and_written_as_zero(gpu):
    table = synthetic(9, 3, 12, lr.NORMAL, 4, True)
    rs = np.random.RandomState(2)
    x3 = (0.5 * rs.randn(3, 70, 12)).astype(np.float32)
    x3[0, 5, 11] = np.nan            # draw 5: a column no term of observation 0 need read
    x3[1, 69, 0] = np.inf            # draw 139
    x3[2, 69, 3] = -np.inf           # draw 209, the last
    x3[2, 0, 7] = np.nan             # draw 140
    got, mask, count = run(gpu, x3, table)
    bad = np.array([5, 139, 140, 209])
    assert count == 4 and np.array_equal(np.flatnonzero(mask), bad) and set(np.unique(mask)) == {0, 1}
    assert np.all(got[:, bad] == 0.0) and np.isfinite(got).all()
    clean = x3.copy().reshape(-1, 12)
    clean[bad] = 0.0
    ref, _, _ = run(gpu, clean.reshape(3, 70, 12), table)
    keep = np.setdiff1d(np.arange(210), bad)
    assert np.array_equal(got[:, keep], ref[:, keep])


def test_refusals(gpu):
    from autoreparam_amd import _lib, diagnostics
    L = _lib.lib()
    table = synthetic(5, 2, 8, lr.NORMAL, 1, False)
    dt = diagnostics.upload_table(table, 8, gpu)
    x = torch.zeros(2, 3, 8, device=gpu)
    ll = torch.zeros(5, 6, device=gpu)
    mask = torch.zeros(6, dtype=torch.uint8, device=gpu)
    cnt = torch.zeros((), dtype=torch.int64, device=gpu)
    p = _lib.ptr

    def call(x_=x, S=2, Cn=3, D=8, stride=24, kind=0, T=2, n0=0, n1=5, ll_=ll, ll_stride=6, idx=dt.idx):
        return L.arp_pointwise_loglik(p(x_), S, Cn, D, stride, kind, p(idx), p(dt.w), T, p(dt.y), p(dt.scale_idx),
                                      p(dt.log_scale), n0, n1, p(ll_), ll_stride, p(mask), p(cnt), C.c_void_p(0))
    assert call() == 0
    torch.cuda.synchronize()
    for kwargs, word in ((dict(x_=None), b"required"), (dict(ll_=None), b"required"), (dict(idx=None), b"required"),
                         (dict(D=0), b"D"), (dict(D=256), b"D"), (dict(stride=23), b"row_stride"), (dict(kind=2), b"kind"),
                         (dict(T=0), b"T"), (dict(n0=5, n1=5), b"n0"), (dict(n0=-1), b"n0"), (dict(ll_stride=5), b"ll_stride"),
                         (dict(S=0), b"n_samples")):
        assert call(**kwargs) != 0, kwargs
        assert word in L.arp_last_error(), (kwargs, L.arp_last_error())
    with pytest.raises(ValueError, match="outside the state"):
        diagnostics.upload_table(table._replace(idx=table.idx + 7), 8, gpu)
    with pytest.raises(ValueError, match="observations is required"):
        diagnostics.pointwise_loglik(x, dt, 0, 6)
