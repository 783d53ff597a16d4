"""GPU: arp_psis_loo (csrc/psis.hip) through diagnostics.psis_loo against the float64 definition tests/psis_ref.py, on
float32 ll matrices handed to both sides: tail_len, cutoff and draws_used EQUAL; lppd and p_waic within the bounds of
psis.hip's header; pareto_k, gpd_sigma and elpd_loo -- for which no a-priori bound can be derived, they go through the
profile weights of the generalised Pareto fit -- within 16 x the largest deviation measured over these very cases on an
MI355X (K_MEASURED = 7.55e-15, SIGMA_MEASURED = 8.6e-15 relative, ELPD_MEASURED = 1.78e-14 below, allowed 1.2e-13,
1.4e-13 and 2.8e-13; float64 arithmetic predicts at most about M^2 2^-53 = 7e-11 at M = 768, and 1e-8 or more would
mean a float32 step crept in).  Ties across the cut-off, rows that are not fitted,
non-finite rows, masked draws, a stride, reproducibility, refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import psis_checks as pc
import psis_ref as pr
from psis_checks import device

pytestmark = pytest.mark.gpu

RS = (1, 4, 5, 24, 25, 26, 224, 225, 226, 255, 256, 257, 1024, 4097, 70001)
# largest deviations over every case of this file, measured on an MI355X: |k - k_ref|, |sigma - sigma_ref| / sigma_ref,
# |elpd_loo - ref| (all three at N = 257, R = 300; at R = 70 001, M = 794: 4.7e-15, 6.1e-15, 6.2e-15 -- float64
# throughout, four orders of magnitude below what a float32 step would leave); the tests allow 16 x these
K_MEASURED, SIGMA_MEASURED, ELPD_MEASURED = 7.55e-15, 8.6e-15, 1.78e-14
FACTOR = pc.FACTOR             # 16


def rows_for(R, seed):
    """(names, ll [11, R] float32): the data of the issue, one row each."""
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


def compare(got, ref, ll, mask, what):
    """psis_checks.compare at this file's measured constants; the largest deviations (k, sigma relative, elpd)."""
    return pc.compare(got, ref, ll, mask, what, (K_MEASURED, SIGMA_MEASURED, ELPD_MEASURED))[:3]


@pytest.mark.parametrize("R", RS)
def test_rows_against_the_definition(gpu, R):
    """Every kind of row at every R: around the no-fit threshold (24 / 25), a perfect square and its neighbours (225),
    the workgroup width (256), past what LDS could hold of a whole row (70 001); a stride larger than R; and the same
    rows with a tenth of the draws masked, the masked entries holding NaN -- they must never be read."""
    names, ll = rows_for(R, R)
    ref = pr.psis_loo(ll)
    worst = compare(device(gpu, ll, pad=13), ref, ll, None, ("R=%d" % R, names))
    rs = np.random.RandomState(R + 1)
    mask = (rs.rand(R) < 0.1).astype(np.uint8)
    mask[rs.randint(R)] = 0
    poisoned = ll.copy()
    poisoned[:9, mask != 0] = np.nan               # (the -inf and NaN rows keep their own entry wherever it fell)
    refm = pr.psis_loo(ll, mask)
    worst = np.maximum(worst, compare(device(gpu, poisoned, mask, pad=3), refm, ll, mask, ("masked R=%d" % R, names)))
    print("R=%d: largest deviation k %.3g, sigma (relative) %.3g, elpd_loo %.3g" % (R, worst[0], worst[1], worst[2]))


@pytest.mark.parametrize("N", (1, 3, 257))
def test_observation_counts(gpu, N):
    rs = np.random.RandomState(N)
    ll = (-rs.choice([0.1, 0.5, 0.9, 1.5], size=(N, 1)) * rs.exponential(size=(N, 300))).astype(np.float32)
    worst = compare(device(gpu, ll), pr.psis_loo(ll), ll, None, "N=%d" % N)
    print("N=%d: largest deviation k %.3g, sigma (relative) %.3g, elpd_loo %.3g" % (N, worst[0], worst[1], worst[2]))


def test_cut_off_splits_a_group_of_ties(gpu):
    """R = 300, every value three times: M = 52 is no multiple of three, so the cut-off value has one copy inside the tail
    and two outside.  Any order of the draws gives the same bits."""
    rs = np.random.RandomState(300)
    base = np.repeat((-0.8 * rs.exponential(size=100)).astype(np.float32), 3)
    ll = np.stack([base, base[rs.permutation(300)], base[::-1]])
    ref = pr.psis_loo(ll)
    s = np.sort(base)
    assert ref[0, 4] == 52 and s[51] == s[52] and s[50] != s[51]
    got = device(gpu, ll)
    compare(got, ref, ll, None, "ties")
    assert np.array_equal(got[0, 4:8], got[1, 4:8]) and np.array_equal(got[0, 4:8], got[2, 4:8])
    assert np.allclose(got[0], got[1], rtol=1e-12, atol=0) and np.allclose(got[0], got[2], rtol=1e-12, atol=0)


def test_two_calls_are_bitwise_equal(gpu):
    _, ll = rows_for(4097, 5)
    a, b = device(gpu, ll, pad=5), device(gpu, ll, pad=5)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_refusals(gpu):
    from autoreparam_amd import _lib
    L = _lib.lib()
    ll = torch.zeros(2, 64, device=gpu)
    out = torch.zeros(2, 8, dtype=torch.float64, device=gpu)
    need = int(L.arp_psis_workspace_bytes(2, 64))
    assert need > 0 and need % 256 == 0
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=gpu)
    p = _lib.ptr

    def call(ll_=ll, N=2, R=64, stride=64, out_=out, ws_=ws, bytes_=need):
        return L.arp_psis_loo(p(ll_), N, R, stride, C.c_void_p(0), p(out_), p(ws_), bytes_, C.c_void_p(0))
    assert call() == 0
    torch.cuda.synchronize()
    assert L.arp_psis_workspace_bytes(1, (1 << 24) + 1) == 0 and L.arp_psis_workspace_bytes(0, 64) == 0
    assert L.arp_psis_workspace_bytes(1, 1 << 24) > 0
    for kwargs, word in ((dict(ll_=None), b"required"), (dict(out_=None), b"required"), (dict(N=0), b"n_obs"),
                         (dict(R=0), b"n_draws"), (dict(R=(1 << 24) + 1, stride=(1 << 24) + 1), b"2^24"),
                         (dict(stride=63), b"ll_stride"), (dict(ws_=None), b"workspace"), (dict(bytes_=need - 1), b"too small"),
                         (dict(ws_=ws[8:]), b"aligned")):
        assert call(**kwargs) != 0, kwargs
        assert word in L.arp_last_error(), (kwargs, L.arp_last_error())
