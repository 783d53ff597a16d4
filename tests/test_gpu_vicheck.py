"""GPU: the three device stages of the variational-fit check, each against the float64 definition (tests/vicheck_ref.py)
on the SAME inputs, then diagnostics.vi_check end to end on the known answer of tests/test_vicheck_host.py.

arp_vi_draws: z within twice ppc.hip's 18 u |z|, x within one ulp of float32(scale z_dev + loc), logq within
(D + 8) 2^-53 sum |terms| of the float64 value of the device's own z; offsets are rows, bit for bit.
arp_psis_weights: out8 bitwise arp_psis_loo's; the draws whose weight differs from the raw one are the reference's tail;
raw positions EQUAL; smoothed positions within 16 x the largest deviation measured over these very cases on an MI355X
(LW_MEASURED below, relative to max(|lw|, 1); float64 predicts about M^2 2^-53, and 1e-10 or more would mean a float32
step crept in).
arp_vi_fold: within 64 2^-52 sum |terms| of the long-double sums, the bar of arp_jump_sums; the count and the minimum exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import psis_checks as pc
import vicheck_ref as vr
from psis_checks import device_weights
from vicheck_ref import Case, check_known_answer, R as R_KNOWN, SEED as SEED_KNOWN

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# largest |lw_dev - lw_ref| / max(|lw_ref|, 1) over the smoothed positions of every case of this file, measured on an
# MI355X (at R = 70 001, M = 794; 4.4e-15 at R = 4 097, below 1e-15 up to R = 257); the tests allow 16 x this, and the
# figure itself must stay below 1e-10
LW_MEASURED = 1.62e-14
FACTOR = pc.FACTOR             # 16


# ---- arp_vi_draws ----
def q_of(D, seed):
    rs = np.random.RandomState(seed)
    return (3.0 * rs.randn(D)).astype(np.float32), np.exp(rs.uniform(-3.0, 2.0, size=D)).astype(np.float32)


def check_draws(gpu, D, R, seed, offset=0, pad=0):
    from autoreparam_amd import diagnostics
    loc, scale = q_of(D, D)
    out = None
    if pad:
        out = tuple(torch.full((R, D + pad), -77.0, dtype=torch.float32, device=gpu) for _ in range(2))
    x, z, logq = diagnostics.vi_draws(loc, scale, R, seed=seed, draw_offset=offset, device=gpu, out=out)
    x, z, logq = x.cpu().numpy(), z.cpu().numpy(), logq.cpu().numpy()
    if pad:
        assert np.all(x[:, D:] == -77.0) and np.all(z[:, D:] == -77.0)               # the guard columns
        x, z = x[:, :D], z[:, :D]
    ref = vr.normals(D, np.uint64(offset) + np.arange(R, dtype=np.uint64), seed)
    assert np.all(np.abs(z - ref) <= 2 * 18 * U * np.abs(ref)), np.abs((z - ref) / ref).max()
    want = scale.astype(np.float64) * z.astype(np.float64) + loc.astype(np.float64)
    ulp = np.spacing(np.abs(want.astype(np.float32)).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(x.astype(np.float64) - want.astype(np.float32).astype(np.float64)) <= ulp)
    assert np.all(np.abs(logq - vr.logq_of(z, scale)) <= (D + 8) * 2.0 ** -53 * vr.logq_terms(z, scale))
    return x, z, logq


@pytest.mark.parametrize("D", (1, 2, 3, 4, 5, 71, 257))
def test_draws_against_the_definition(gpu, D):
    for R in (1, 63, 64, 65, 257, 1000):
        check_draws(gpu, D, R, seed=1000 * D + R)


def test_draws_stride_seed_and_offset(gpu):
    check_draws(gpu, 71, 257, seed=5, pad=9)
    check_draws(gpu, 5, 65, seed=0xFEDCBA9876543210)
    check_draws(gpu, 5, 65, seed=7, offset=(1 << 32) + 5)
    whole = check_draws(gpu, 71, 1000, seed=9)
    part = check_draws(gpu, 71, 300, seed=9, offset=411)
    for a, b in zip(whole, part):
        assert np.array_equal(a[411:711].view(np.uint8), b.view(np.uint8))
    for a, b in zip(whole, check_draws(gpu, 71, 1000, seed=9)):                       # two calls
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- arp_psis_weights ----
def rows_for(R, seed):
    """The rows of tests/test_gpu_psis.py: rows_for, rebuilt here."""
    rs = np.random.RandomState(seed)
    rows = [("exp k=%g" % k, -k * rs.exponential(size=R)) for k in (0.1, 0.5, 0.9, 1.5)]
    rows.append(("normal", -1.0 + 0.3 * rs.randn(R)))
    rows.append(("triples", rs.permutation(np.repeat(-0.5 * rs.exponential(size=(R + 2) // 3), 3)[:R])))
    rows.append(("constant", np.full(R, -1.25)))
    rows.append(("two values", np.where(rs.rand(R) < 0.3, -2.0, -0.5)))
    rows.append(("zeros of both signs", np.where(rs.rand(R) < 0.5, -0.0, 0.0)))
    a = -0.7 * rs.exponential(size=R)
    a[rs.randint(R)] = -np.inf
    rows.append(("one -inf", a))
    b = -0.7 * rs.exponential(size=R)
    b[rs.randint(R)] = np.nan
    rows.append(("one NaN", b))
    return [n for n, _ in rows], np.stack([v for _, v in rows]).astype(np.float32)


def compare_weights(lw, ll, mask, names, what):
    """psis_checks.compare_weights at this file's measured constant; the largest deviation at a smoothed position."""
    return pc.compare_weights(lw, ll, mask, names, what, LW_MEASURED)


@pytest.mark.parametrize("R", (4, 25, 26, 257, 4097, 70001))
def test_weights_against_the_definition(gpu, R):
    """Every kind of row (ties across the cut-off among them), not-fitted and non-finite rows, a stride, and the same rows
    with a tenth of the draws masked, the masked entries holding NaN."""
    names, ll = rows_for(R, R)
    _, lw = device_weights(gpu, ll, pad=13)
    worst = compare_weights(lw, ll, None, names, "R=%d" % R)
    rs = np.random.RandomState(R + 1)
    mask = (rs.rand(R) < 0.1).astype(np.uint8)
    mask[rs.randint(R)] = 0
    poisoned = ll.copy()
    poisoned[:9, mask != 0] = np.nan
    _, lwm = device_weights(gpu, poisoned, mask, pad=3)
    worst = max(worst, compare_weights(lwm, ll, mask, names, "masked R=%d" % R))
    print("R=%d: largest deviation at a smoothed position %.3g" % (R, worst))
    assert LW_MEASURED < 1e-10


def test_weights_split_a_group_of_ties_by_draw_index(gpu):
    """R = 300, every value three times, M = 52: the cut-off value has one copy inside the tail -- the one with the lowest
    draw index -- and within a group the smoothed weights descend with the draw index."""
    rs = np.random.RandomState(300)
    base = np.repeat((-0.8 * rs.exponential(size=100)).astype(np.float32), 3)
    ll = np.stack([base, base[rs.permutation(300)], base[::-1].copy()])
    _, lw = device_weights(gpu, ll)
    compare_weights(lw, ll, None, ["sorted", "shuffled", "reversed"], "ties")
    for n in range(3):
        _, _, tail = vr.weights_row(ll[n])
        cut = np.sort(ll[n])[52]
        at = np.flatnonzero(ll[n] == cut)
        assert at.size == 3 and np.array_equal(np.intersect1d(at, tail), at[:1])


def test_weights_two_calls_are_bitwise_equal(gpu):
    _, ll = rows_for(4097, 5)
    a, b = device_weights(gpu, ll, pad=5), device_weights(gpu, ll, pad=5)
    assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))


# ---- arp_vi_fold ----
def fold_case(R, D, seed):
    rs = np.random.RandomState(seed)
    z, grad, e = (rs.randn(R, D).astype(np.float32) * s for s in (1.0, 30.0, 2.0))
    ll = (5.0 * rs.randn(R)).astype(np.float32)
    lw = -rs.exponential(size=R) * 3.0
    lw[rs.rand(R) < 0.15] = -np.inf
    if R > 2:
        lw[R - 1] = -np.inf
        lw[0] = 0.0
    return z, grad, e, ll, lw, np.exp(rs.uniform(-2, 1, size=D)).astype(np.float32), rs.randn(D).astype(np.float32)


def device_fold(gpu, case):
    from autoreparam_amd import diagnostics
    dev = [torch.as_tensor(np.ascontiguousarray(v), device=gpu) for v in case]
    elem, tot = diagnostics.vi_fold(*dev)
    return elem.cpu().numpy(), tot.cpu().numpy()


@pytest.mark.parametrize("D", (1, 71, 257))
def test_fold_against_long_double(gpu, D):
    for R in (1, 255, 256, 257, 5000):
        case = fold_case(R, D, 31 * R + D)
        elem, tot = device_fold(gpu, case)
        ref_elem, ref_tot, abs_elem, abs_tot = vr.fold(*case)
        bar = 64 * 2.0 ** -52
        assert np.all(np.abs(elem.astype(np.longdouble) - ref_elem) <= bar * abs_elem), (R, D)
        assert np.all(np.abs(tot[1:4].astype(np.longdouble) - ref_tot[1:4]) <= bar * abs_tot[1:4]), (R, D)
        assert tot[0] == float(ref_tot[0]) and tot[4] == float(ref_tot[4]), (R, D, tot, ref_tot)
        again = device_fold(gpu, case)
        assert np.array_equal(elem.view(np.uint64), again[0].view(np.uint64)) and np.array_equal(tot.view(np.uint64), again[1].view(np.uint64))


def test_fold_of_no_kept_draw(gpu):
    case = list(fold_case(300, 5, 1))
    case[4] = np.full(300, -np.inf)
    case[4][7] = np.nan                                                                   # NaN does not count either
    elem, tot = device_fold(gpu, case)
    assert np.all(elem == 0.0) and np.all(tot[:4] == 0.0) and tot[4] == np.inf


# ---- refusals ----
def test_refusals(gpu):
    from autoreparam_amd import _lib, diagnostics
    L = _lib.lib()
    p, null = _lib.ptr, C.c_void_p(0)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=gpu)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=gpu)
    loc, scale, x, z, logq = f32(4), torch.ones(4, device=gpu), f32(8, 4), f32(8, 4), f64(8)

    def draws(loc_=loc, scale_=scale, D=4, R=8, offset=0, x_=x, z_=z, stride=4, logq_=logq):
        return L.arp_vi_draws(p(loc_), p(scale_), D, R, 1, offset, p(x_), p(z_), stride, p(logq_), null)
    assert draws() == 0
    for kwargs, word in ((dict(loc_=None), b"required"), (dict(scale_=None), b"required"), (dict(x_=None), b"required"),
                         (dict(z_=None), b"required"), (dict(logq_=None), b"required"), (dict(D=0), b"D >= 1"),
                         (dict(R=0), b"n_draws"), (dict(R=(1 << 24) + 1), b"2^24"), (dict(stride=3), b"row_stride"),
                         (dict(offset=-1), b"draw_offset")):
        assert draws(**kwargs) != 0, kwargs
        assert b"arp_vi_draws" in L.arp_last_error() and word in L.arp_last_error(), (kwargs, L.arp_last_error())
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="finite and positive"):
            diagnostics.vi_draws(np.zeros(3), np.array([1.0, bad, 1.0]), 8, device=gpu)

    ll = f32(2, 64)
    out, lw = f64(2, 8), f64(2, 64)
    need = int(L.arp_psis_weights_workspace_bytes(2, 64))
    assert need > int(L.arp_psis_workspace_bytes(2, 64)) and need % 256 == 0
    assert L.arp_psis_weights_workspace_bytes(1, (1 << 24) + 1) == 0 and L.arp_psis_weights_workspace_bytes(0, 64) == 0
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=gpu)

    def weights(ll_=ll, N=2, R=64, stride=64, out_=out, lw_=lw, lws=64, ws_=ws, bytes_=need):
        return L.arp_psis_weights(p(ll_), N, R, stride, null, p(out_), p(lw_), lws, p(ws_), bytes_, null)
    assert weights() == 0
    for kwargs, word in ((dict(ll_=None), b"required"), (dict(out_=None), b"required"), (dict(lw_=None), b"required"),
                         (dict(N=0), b"n_obs"), (dict(R=0), b"n_draws"), (dict(R=(1 << 24) + 1, stride=(1 << 24) + 1), b"2^24"),
                         (dict(stride=63), b"ll_stride"), (dict(lws=63), b"lw_stride"), (dict(ws_=None), b"workspace"),
                         (dict(bytes_=need - 1), b"too small"), (dict(ws_=ws[8:]), b"aligned")):
        assert weights(**kwargs) != 0, kwargs
        assert b"arp_psis_weights" in L.arp_last_error() and word in L.arp_last_error(), (kwargs, L.arp_last_error())

    g, e, l1, w1, e0, elem, tot = f32(8, 4), f32(8, 4), f32(8), f64(8), f32(4), f64(4, 9), f64(5)
    need = int(L.arp_vi_fold_workspace_bytes(8, 4))
    assert need > 0 and need % 256 == 0 and L.arp_vi_fold_workspace_bytes(0, 4) == 0 and L.arp_vi_fold_workspace_bytes(8, 0) == 0
    assert L.arp_vi_fold_workspace_bytes((1 << 24) + 1, 4) == 0
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=gpu)

    def fold(z_=z, g_=g, e_=e, stride=4, ll_=l1, lw_=w1, s_=scale, e0_=e0, R=8, D=4, elem_=elem, tot_=tot, ws_=ws, bytes_=need):
        return L.arp_vi_fold(p(z_), p(g_), p(e_), stride, p(ll_), p(lw_), p(s_), p(e0_), R, D, p(elem_), p(tot_), p(ws_), bytes_, null)
    assert fold() == 0
    torch.cuda.synchronize()
    for kwargs, word in ((dict(z_=None), b"required"), (dict(g_=None), b"required"), (dict(e_=None), b"required"),
                         (dict(ll_=None), b"required"), (dict(lw_=None), b"required"), (dict(s_=None), b"required"),
                         (dict(e0_=None), b"required"), (dict(elem_=None), b"required"), (dict(tot_=None), b"required"),
                         (dict(D=0), b"D <= 2^24"), (dict(R=0), b"n_draws"), (dict(R=(1 << 24) + 1), b"2^24"),
                         (dict(stride=3), b"row_stride"), (dict(ws_=None), b"workspace"), (dict(bytes_=need - 1), b"too small"),
                         (dict(ws_=ws[8:]), b"aligned")):
        assert fold(**kwargs) != 0, kwargs
        assert b"arp_vi_fold" in L.arp_last_error() and word in L.arp_last_error(), (kwargs, L.arp_last_error())


# ---- end to end ----
def test_vi_check_on_the_known_answer(gpu, oracle_lib):
    """diagnostics.vi_check on radon MN CP at the known-answer q: equal to the reference pipeline fed with the device's own
    draws, logp, gradient and centred rows, and within the statistical bounds of tests/test_vicheck_host.py."""
    from autoreparam_amd import diagnostics, engine
    c = Case(oracle_lib, "CP")
    eng = engine.engine_for(c.sp, gpu)
    eng.set_param(0, "CP")
    chk = diagnostics.vi_check(eng, c.loc, c.scale, which=0, draws=R_KNOWN, seed=SEED_KNOWN)
    x, z, logq = diagnostics.vi_draws(c.loc, c.scale, R_KNOWN, seed=SEED_KNOWN, device=gpu)
    logp, grad = eng.logp_grad(x, which=0)
    e = eng.transform(x, which=0)
    e0 = eng.transform(c.loc.reshape(1, -1), which=0)[0]
    host = lambda t: t.cpu().numpy()
    ref = vr.pipeline_from(host(z), host(logq), host(logp), host(grad), host(e), host(e0), c.scale)
    assert chk.left_out == 0 and ref.mask.sum() == 0
    assert np.array_equal(chk.log_ratio, -ref.ll) and np.array_equal(chk.e0, host(e0).astype(np.float64))
    assert chk.out8[4] == ref.out8[4] and chk.out8[5] == ref.out8[5] and chk.out8[7] == ref.out8[7]
    assert abs(chk.out8[1] - ref.out8[1]) <= 1e-10 and abs(chk.out8[3] - ref.out8[3]) <= 1e-9 * ref.out8[3]
    _, _, tail = vr.weights_row(ref.ll)
    rest = np.setdiff1d(np.arange(R_KNOWN), tail)
    assert np.array_equal(chk.log_weight[rest], ref.lw[rest])
    assert np.abs(chk.log_weight[tail] - ref.lw[tail]).max() <= 1e-10
    np.testing.assert_allclose(chk.elem, ref.elem, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(chk.tot, ref.tot, rtol=1e-10)
    assert chk.tot[0] == R_KNOWN and chk.tot[4] == ref.tot[4]
    assert chk.logp_const == pytest.approx(c.const, rel=1e-9)
    s = diagnostics.vi_check_summary(chk.elem, chk.tot, chk.out8, c.loc, c.scale, chk.e0, chk.logp_const)
    check_known_answer(c, s)
