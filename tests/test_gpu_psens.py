"""GPU: the device pieces of the power-scaling sensitivity report (csrc/psens.hip) against tests/psens_ref.py.
arp_element_order: the order EQUALS the reference's stable argsort on the uint32 key and the sorted values are bitwise
its, at the sort-tile and key-tile edges, with long tie runs, +-0, +-inf, denormals and a NaN of each sign, in place in a
wider trace and twice over.  arp_cjs_sums: the count exact, every float column within the header's first-order bound
computed from the reference's own absolute terms, bitwise repeatable, a row's sums independent of its neighbours.
arp_loglik_total: exact against float64 sequential addition; tiles compose bit for bit.  The prior decomposition: the
centred log joint minus the summed pointwise log-likelihood against the float64 oracle minus tests/loglik_ref.py."""

import numpy as np
import pytest
import torch

import loglik_ref as lr
import psens_ref as pr
from test_gpu_loglik import CENTRES
from test_loo_host import TABLE_SPECS

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 4095, 4096, 4097, 8193)          # 4 096 is the sort tile, 64 the key-pass tile's rows, 256 a cjs chunk


def pool(N, D, seed):
    """Pooled draws [N, D] float32 whose columns cycle through: normal values; values quantised to 16 levels (long tie
    runs); an all-equal column; +-0 mixed with a few values; +-inf, denormals and a NaN of each sign among normals."""
    rs = np.random.RandomState(seed)
    x = rs.randn(N, D).astype(np.float32)
    for d in range(D):
        kind = d % 5
        if kind == 1:
            x[:, d] = np.floor(rs.rand(N) * 16.0) / 4.0 - 2.0
        elif kind == 2:
            x[:, d] = 1.25
        elif kind == 3:
            x[:, d] = np.where(rs.rand(N) < 0.4, 0.0, np.where(rs.rand(N) < 0.5, -0.0, x[:, d])).astype(np.float32)
        elif kind == 4:
            special = np.array([np.inf, -np.inf, 1e-45, -1e-45, 3e-39, -3e-39, np.nan, -np.nan, 0.0, -0.0], np.float32)
            special[7] = np.array([0xffc00000], np.uint32).view(np.float32)[0]           # a NaN with the sign bit set
            at = rs.permutation(N)[:min(N, special.size)]
            x[at, d] = special[:at.size]
    return x


def shape_of(N):
    return (7, N // 7) if N % 7 == 0 and N >= 14 else (1, N)


def order_case(gpu, N, D, seed):
    from autoreparam_amd import diagnostics
    x = pool(N, D, seed)
    S, Cn = shape_of(N)
    want_order, want_sorted = pr.element_order(x)
    xd = torch.as_tensor(x.reshape(S, Cn, D), device=gpu)
    order, values = diagnostics.element_order(xd)
    again, values2 = diagnostics.element_order(xd)
    got = order.cpu().numpy().view(np.uint32)
    assert got.shape == (D, N) and np.array_equal(got, want_order)
    assert np.array_equal(values.cpu().numpy().view(np.uint32), want_sorted.view(np.uint32))
    assert torch.equal(order, again) and np.array_equal(values2.cpu().numpy().view(np.uint32), want_sorted.view(np.uint32))
    only_order, none = diagnostics.element_order(xd, want_sorted=False)
    assert none is None and torch.equal(only_order, order)
    # a block of chains taken in place: row_stride > n_chains * D, NaN poison around it
    wide = torch.full((S, Cn + 3, D), float("nan"), dtype=torch.float32, device=gpu)
    wide[:, 1:1 + Cn] = xd
    block_order, block_values = diagnostics.element_order(wide[:, 1:1 + Cn])
    assert torch.equal(block_order, order) and torch.equal(block_values.view(torch.int32), values.view(torch.int32))


@pytest.mark.parametrize("D", (1, 129))
@pytest.mark.parametrize("N", SIZES)
def test_element_order(gpu, N, D):
    order_case(gpu, N, D, 100 * D + N)


def test_element_order_many_tiles(gpu):
    order_case(gpu, 70000, 3, 5)


@pytest.mark.parametrize("D", (2, 127, 128, 255))
def test_element_order_key_tile_widths(gpu, D):
    order_case(gpu, 257, D, D)


def test_element_order_refusals(gpu):
    from autoreparam_amd import _lib, diagnostics
    L = _lib.lib()
    assert L.arp_element_order_workspace_bytes(1 << 20, 1 << 11, 1) == 0 and b"2^31" in L.arp_last_error()
    x = torch.zeros(2, 3, 4, dtype=torch.float32, device=gpu)
    order = torch.empty(4, 6, dtype=torch.int32, device=gpu)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=gpu)
    call = lambda *a: L.arp_element_order(*a, _lib.stream())
    assert call(_lib.ptr(x), 2, 3, 4, 11, _lib.ptr(order), None, _lib.ptr(ws), ws.numel()) == 1          # row_stride < C D
    assert call(None, 2, 3, 4, 12, _lib.ptr(order), None, _lib.ptr(ws), ws.numel()) == 1
    assert call(_lib.ptr(x), 2, 3, 4, 12, None, None, _lib.ptr(ws), ws.numel()) == 1
    assert call(_lib.ptr(x), 2, 3, 4, 12, _lib.ptr(order), None, _lib.ptr(ws), 16) == 1 and b"workspace" in L.arp_last_error()
    assert call(_lib.ptr(x), 2, 3, 4, 12, _lib.ptr(order), None, None, 0) == 1
    assert L.arp_cjs_sums(_lib.ptr(x), _lib.ptr(order), 6, 4, _lib.ptr(ws), 6, 9, None, _lib.ptr(ws), _lib.stream()) == 1
    assert L.arp_cjs_sums(_lib.ptr(x), _lib.ptr(order), 6, 4, _lib.ptr(ws), 5, 1, None, _lib.ptr(ws), _lib.stream()) == 1
    assert L.arp_cjs_sums(_lib.ptr(x), None, 6, 4, _lib.ptr(ws), 6, 1, None, _lib.ptr(ws), _lib.stream()) == 1
    assert L.arp_loglik_total(_lib.ptr(x), 2, 12, 11, _lib.ptr(ws), _lib.stream()) == 1
    assert L.arp_loglik_total(_lib.ptr(x), 0, 12, 12, _lib.ptr(ws), _lib.stream()) == 1
    with pytest.raises(ValueError):
        diagnostics.cjs_sums(x[0], order[:3], torch.zeros(9, 4, dtype=torch.float64, device=gpu))
    torch.cuda.synchronize()


def weight_rows(N, x0, seed):
    """Eight rows of log weights [8, N]: uniform; smooth 0.01 x; spanning 0 ... -745 (Q underflows to 0 on a stretch); all
    weight on one draw (the others underflow to 0 but are kept); -inf scattered; -inf on all but one draw (n' = 1); -inf
    throughout (n' = 0); smooth with two draws kept (n' = 2 at most)."""
    rs = np.random.RandomState(seed)
    lw = np.zeros((8, N))
    lw[1] = 0.01 * x0.astype(np.float64)
    lw[2] = -745.0 * rs.permutation(N) / max(N - 1, 1)
    lw[3] = -800.0
    lw[3, rs.randint(N)] = 0.0
    lw[4] = np.where(rs.rand(N) < 0.3, -np.inf, -rs.rand(N))
    lw[5] = -np.inf
    lw[5, rs.randint(N)] = -0.5
    lw[6] = -np.inf
    lw[7] = -np.inf
    two = rs.permutation(N)[:2]
    lw[7, two] = np.array([-0.1, -2.0])[:two.size]
    return lw


def check_sums(got, want, mag, N, what):
    assert np.array_equal(got[..., 0], want[..., 0]), what                                       # n' is exact
    gap, allow = np.abs(got[..., 1:] - want[..., 1:]), pr.bound(N, mag[..., 1:])
    worst = float(np.max(gap / np.maximum(allow, 1e-300)))
    print("cjs_sums %s: largest deviation / allowance %.3f" % (what, worst))
    assert np.all(np.isfinite(got)) and np.all(gap <= allow), (what, worst)


@pytest.mark.parametrize("D", (1, 5))
@pytest.mark.parametrize("N", SIZES)
def test_cjs_sums(gpu, N, D):
    from autoreparam_amd import diagnostics
    rs = np.random.RandomState(7 * N + D)
    x = rs.randn(N, D).astype(np.float32)
    if D > 1:
        x[:, 1] = np.floor(rs.rand(N) * 16.0) / 4.0                                              # long tie runs
        x[:, 2] = 0.5                                                                            # a constant element
    shift = x.mean(axis=0).astype(np.float32)
    order, values = pr.element_order(x)
    lw = weight_rows(N, x[:, 0], N + D)
    od = torch.as_tensor(order.view(np.int32), device=gpu)
    vd = torch.as_tensor(values, device=gpu)
    sd = torch.as_tensor(shift, device=gpu)
    lwd = torch.as_tensor(lw, device=gpu)
    want, mag = pr.cjs_sums(values, order, lw, shift)
    halves = []
    for k0 in (0, 4):                                                                            # K = 4
        out = diagnostics.cjs_sums(vd, od, lwd[k0:k0 + 4], sd)
        assert torch.equal(out, diagnostics.cjs_sums(vd, od, lwd[k0:k0 + 4], sd))                # bitwise repeat
        halves.append(out.cpu().numpy())
    got = np.concatenate(halves, axis=0)
    check_sums(got, want, mag, N, (N, D))
    if N >= 2:
        zero = pr.bound(N, mag[0, :, 4:6])                                                       # uniform weights: Q = P
        assert np.all(np.abs(want[0, :, 4:6]) <= zero) and np.all(np.abs(got[0, :, 4:6]) <= zero)
    assert np.all(got[5:7, :, 4:] == 0) and np.all(got[6] == 0)                                  # n' in {0, 1}: zeros
    for k in (1, 4):                                                                             # K = 1: a row alone is itself
        alone = diagnostics.cjs_sums(vd, od, lwd[k:k + 1], sd).cpu().numpy()
        assert np.array_equal(alone[0], got[k])
    if D == 1:                                                                                   # no shift: about 0
        bare = diagnostics.cjs_sums(vd, od, lwd[:4]).cpu().numpy()
        want0, mag0 = pr.cjs_sums(values, order, lw[:4])
        check_sums(bare, want0, mag0, N, (N, "no shift"))


def test_cjs_sums_nan_weight_carries_through(gpu):
    from autoreparam_amd import diagnostics
    N = 300
    x = np.random.RandomState(3).randn(N, 1).astype(np.float32)
    order, values = pr.element_order(x)
    lw = np.zeros((2, N))
    lw[0, int(order[0, 10])] = np.nan
    lw[1, 5] = -np.inf
    out = diagnostics.cjs_sums(torch.as_tensor(values, device=gpu), torch.as_tensor(order.view(np.int32), device=gpu),
                               torch.as_tensor(lw, device=gpu)).cpu().numpy()
    assert out[0, 0, 0] == N and np.all(np.isnan(out[0, 0, [1, 2, 3, 5, 7]]))
    assert out[1, 0, 0] == N - 1 and np.all(np.isfinite(out[1]))


@pytest.mark.parametrize("R", (1, 64, 65, 4097))
@pytest.mark.parametrize("n_obs", (1, 3, 1000))
def test_loglik_total(gpu, n_obs, R):
    from autoreparam_amd import diagnostics
    rs = np.random.RandomState(n_obs + R)
    ll = (-5.0 * rs.rand(n_obs, R) * np.exp(3.0 * rs.randn(n_obs, 1))).astype(np.float32)
    start = rs.randn(R)
    want = start.copy()
    for n in range(n_obs):
        want += ll[n].astype(np.float64)                                                         # sequential, float64
    lld = torch.as_tensor(ll, device=gpu)
    got = diagnostics.loglik_total(lld, torch.as_tensor(start, device=gpu))
    assert np.array_equal(got.cpu().numpy(), want)
    wide = torch.full((n_obs, R + 5), float("nan"), dtype=torch.float32, device=gpu)             # rows further apart than R
    wide[:, :R] = lld
    assert np.array_equal(diagnostics.loglik_total(wide[:, :R], torch.as_tensor(start, device=gpu)).cpu().numpy(), want)
    if n_obs >= 3:                                                                               # three tiles are one call
        tiled = torch.as_tensor(start, device=gpu)
        a, b = n_obs // 3, n_obs - n_obs // 2
        for lo, hi in ((0, a), (a, b), (b, n_obs)):
            diagnostics.loglik_total(lld[lo:hi], tiled)
        assert np.array_equal(tiled.cpu().numpy(), want)


def _oracle(oracle_lib, name, sp):
    if name == "german_credit_gammascale":
        import gammascale_ref
        ref = gammascale_ref.GermanRef(sp.raw["X"], sp.raw["y"])
        return lambda x, a, b: ref.logp_grad(x, a, b)[0]
    orc = oracle_lib.OracleModel(sp)
    return lambda x, a, b: orc.logp_grad(x, a, b)[0]


@pytest.mark.parametrize("name", sorted(TABLE_SPECS))
def test_prior_decomposition(gpu, oracle_lib, name):
    """At 256 random centred states (N(0, 0.5) around test_gpu_loglik's plausible point): the centred log joint of the
    engine minus the device's summed pointwise log-likelihood, differenced against state 0, against the float64 oracle's
    log joint minus loglik_ref's likelihood differenced the same way (the omitted constants are the same for every
    state).  Allowance: 8 * 2^-24 (|logp| + sum |ll|) of the two states, float32 rounding of sums of that size.  States
    left out as non-finite: 0, checked on the oracle side."""
    from autoreparam_amd import diagnostics, engine, models
    sp = TABLE_SPECS[name](models)
    centre = CENTRES[name](sp) if name in CENTRES else np.zeros(sp.D)
    x = (centre + 0.5 * np.random.RandomState(11).randn(256, sp.D)).astype(np.float32)
    x64 = x.astype(np.float64)
    a, b = sp.ab_from_reparam("CP")
    lp_ref = np.asarray(_oracle(oracle_lib, name, sp)(x64, a, b), np.float64)
    ll_ref = lr.loglik(sp, x64)                                                                  # [R, N]
    assert ll_ref.shape[0] == 256
    left_out = int(np.sum(~np.isfinite(lp_ref) | ~np.isfinite(ll_ref).all(axis=1)))
    print("%s: %d states left out as non-finite" % (name, left_out))
    assert left_out == 0
    eng = engine.Engine(sp, gpu)
    eng.set_param(0, "CP")
    xd = torch.as_tensor(x, device=gpu)
    logp = eng.logp_grad(xd, which=0)[0].to(torch.float64)
    table = diagnostics.upload_table(sp.observation_table(), sp.D, gpu)
    ll, mask, count = diagnostics.pointwise_loglik(xd.reshape(1, 256, sp.D), table)
    total = diagnostics.loglik_total(ll, torch.zeros(256, dtype=torch.float64, device=gpu))
    assert int(count.item()) == 0
    prior = (logp - total).cpu().numpy()
    prior_ref = lp_ref - ll_ref.sum(axis=1)
    size = np.abs(lp_ref) + np.abs(ll_ref).sum(axis=1)
    allow = 8.0 * 2.0 ** -24 * (size + size[0])
    gap = np.abs((prior - prior[0]) - (prior_ref - prior_ref[0]))
    worst = float(np.max(gap[1:] / allow[1:]))
    print("%s: largest deviation / allowance %.3f" % (name, worst))
    assert np.all(gap <= allow), (name, worst)
