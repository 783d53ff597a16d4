"""GPU: rank normalisation on the device (csrc/rank.hip: arp_rank_normalize) and its way up to the CLI, against the float64
yardstick tests/rank_rhat_ref.py applied to the same float32 trace.

The ranks, the median, the quantiles and (through the ranks of the folded run, which are a function of the folded values'
order and ties) the folded values are integers or order statistics: they compare with ==.  Only Phi^-1 is judged with a
tolerance, the project's float32 element tolerance 3e-5: |z - z64| <= 3e-5 max(1, |z64|).
The statistic is allowed what that and the moments' own tolerance (tests/test_gpu_rhat.py: CAP) imply through the
formulas (rhat_allowance)."""
import ctypes as C
import functools
import json
import os
import shutil

import numpy as np
import pytest

import rank_rhat_ref as ref
import rhat_ref
from test_gpu_rhat import CAP, CHAINS, SAMPLES, _packed_trace, _run, rhat_allowance

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.5, 0.95)
Z_TOL = 3e-5
RANK_KEYS = ("rank_rhat_max", "rank_rhat_bulk_max", "rank_rhat_tail_max", "rank_rhat_chains", "rank_rhat_time_sec")
RANK_FAMILIES = ("rank_rhat_bulk", "rank_rhat_tail", "posterior_median", "posterior_q05", "posterior_q95")


@functools.lru_cache(maxsize=None)
def rank_family(S, Cn, D, seed=7):
    """The AR(1) family of tests/test_gpu_rhat.py with another offset and sign per element (a leak between segments
    shows), and: 25 % of the rows repeat their predecessor within the chain, as rejections do; one chain (of two or
    more) is constant for all S; element 1 has +0.0 and -0.0 mixed in; element 2 is constant everywhere; element 3 holds magnitudes from
    subnormal to 1e30 of both signs."""
    from oracle import ess_ref
    rs = np.random.RandomState(seed)
    rho = np.resize([0.0, 0.3, 0.6, 0.9, -0.4], D)
    scale = np.resize([1.0, -10.0, 0.1, -3.0, 1.0, -2.0, 0.5], D)
    offset = np.resize([0.0, 100.0, -5.0, 1e3, 0.25, -40.0, 7.0], D)
    x = (ess_ref.ar1(S, (Cn, D), rho, seed=seed) * scale + offset).astype(np.float32)
    if D >= 4:
        x[:, :, 3] = (np.where(rs.rand(S, Cn) < 0.5, -1.0, 1.0) * 10.0 ** rs.uniform(-44.5, 30.0, (S, Cn))).astype(np.float32)
    if D >= 2:
        u = rs.rand(S, Cn)
        x[:, :, 1][u < 0.10] = np.float32(0.0)
        x[:, :, 1][u > 0.90] = np.float32(-0.0)
    for s in range(1, S):
        rep = rs.rand(Cn) < 0.25
        x[s, rep] = x[s - 1, rep]
    if Cn > 1:                                                # (a one-chain trace stays a varying one)
        x[:, Cn // 2, :] = x[0, Cn // 2, :]
    if D >= 3:
        x[:, :, 2] = np.float32(2.5)
    x.setflags(write=False)
    return x


def yardstick(x):
    """What check_exact_and_z holds a device_run of the float32 trace x [S, C, D] to, raw and folded."""
    N = x.shape[0] * x.shape[1]
    r_raw, r_fold = ref.rank2(x), ref.rank2(ref.folded(x))
    return dict(x=x, N=N, rank2=(r_raw, r_fold), z=(ref.z_scores(r_raw, N), ref.z_scores(r_fold, N)),
                median=ref.median(x), quantiles=ref.quantiles(x, PROBS))


@functools.lru_cache(maxsize=None)
def reference(S, Cn, D, lo=0, hi=None):
    """The yardstick on chains [lo, hi) of rank_family(S, Cn, D), computed once."""
    return yardstick(rank_family(S, Cn, D)[:, lo:hi])


@functools.lru_cache(maxsize=None)
def long_pool(S, Cn, D):
    """A pool of more than 2^20 draws per element, generated without a loop over S.  Element 0: normal draws of scale 3
    about -40, a quarter of the rows repeating their predecessor within the chain, one chain constant.  Element 1 (D = 2):
    the float32 values 1 + k 2^-23, k uniform in 0..255 -- every key shares its upper three bytes (in passes 2 - 4 of the
    sort one digit holds the whole segment, over all its tiles) and every value ties with N / 256 others."""
    assert D in (1, 2)
    rs = np.random.RandomState(S + Cn + D)
    x = np.empty((S, Cn, D), np.float32)
    v = (3.0 * rs.standard_normal((S, Cn)) - 40.0).astype(np.float32)
    rep = rs.rand(S, Cn) < 0.25
    rep[0] = False
    src = np.maximum.accumulate(np.where(rep, 0, np.arange(S)[:, None]), axis=0)      # the last row that moved
    v = np.take_along_axis(v, src, axis=0)
    v[:, Cn // 2] = v[0, Cn // 2]
    x[:, :, 0] = v
    if D == 2:
        x[:, :, 1] = (1.0 + rs.randint(0, 256, (S, Cn)) * 2.0 ** -23).astype(np.float32)
    x.setflags(write=False)
    return x


def device_run(xd, fold):
    """(z, rank2 as uint32, median, quantiles) numpy arrays of one arp_rank_normalize call through diagnostics."""
    import torch
    from autoreparam_amd import diagnostics
    r2 = torch.empty(tuple(xd.shape), dtype=torch.int32, device=xd.device)
    z, med, q = diagnostics.rank_normalize(xd, fold=fold, probs=PROBS, rank2=r2)
    assert z.shape == xd.shape and z.dtype == torch.float32 and med.shape == (xd.shape[2],) and q.shape == (3, xd.shape[2])
    return z.cpu().numpy(), r2.cpu().numpy().view(np.uint32), med.cpu().numpy(), q.cpu().numpy()


def check_exact_and_z(got, want, fold, label):
    z, r2, med, q = got
    assert np.array_equal(r2, want["rank2"][fold]), label
    assert np.array_equal(med, want["median"]) and np.array_equal(q, want["quantiles"]), label
    z64 = want["z"][fold]
    err = np.abs(z.astype(np.float64) - z64) / np.maximum(1.0, np.abs(z64))
    print("%s fold=%d: N = %d, max |z64| %.3f, largest |z - z64| / max(1, |z64|) %.3g (allowed %.3g)" % (
        label, fold, want["N"], np.abs(z64).max(), err.max(), Z_TOL))
    assert (err <= Z_TOL).all(), label


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 1), (601, 37, 5), (600, 40, 7), (1025, 128, 3)])
def test_ranks_and_order_statistics_are_exact_and_z_meets_the_element_tolerance(gpu, shape):
    """rank2, median, quantiles == the yardstick, raw and folded; z within 3e-5 max(1, |z64|) everywhere (a float32 p
    fails that at N = 131 200 by two orders of magnitude); two calls give the same bits."""
    import torch
    want = reference(*shape)
    xd = torch.as_tensor(np.array(want["x"]), device=gpu)
    for fold in (0, 1):
        got = device_run(xd, fold)
        check_exact_and_z(got, want, fold, "family %s" % (shape,))
        again = device_run(xd, fold)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, again))
    if shape[2] >= 3:                                         # the constant element: every draw ties, z == 0 exactly
        assert (got[0][:, :, 2] == 0).all() and (got[1][:, :, 2] == shape[0] * shape[1]).all()


def test_chain_sub_range_view_is_bitwise_the_contiguous_result(gpu):
    """xd[:, 3:11, :] is taken in place: the bits of the same chains passed contiguously, and the yardstick's values."""
    import torch
    S, Cn, D = 600, 40, 7
    want = reference(S, Cn, D, 3, 11)
    xd = torch.as_tensor(np.array(rank_family(S, Cn, D)), device=gpu)
    view = xd[:, 3:11, :]
    assert not view.is_contiguous()
    for fold in (0, 1):
        a, b = device_run(view, fold), device_run(view.contiguous(), fold)
        assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))
        check_exact_and_z(a, want, fold, "view [:, 3:11, :] of (600, 40, 7)")


def statistic_allowance(z64_bulk, z64_tail):
    """What an error of delta = 3e-5 max(1, max |z64|) on every z and the moments' own tolerance can do to the split R-hat
    of a z trace: eps_mean = CAP sqrt(v) + delta, eps_var = CAP v + 2.1 delta sqrt(v) + 4 delta^2 per row of variance v."""
    out = []
    for z64 in (z64_bulk, z64_tail):
        D = z64.shape[-1]
        delta = Z_TOL * max(1.0, np.abs(z64).max())
        v = rhat_ref.moments(z64, True)[1].reshape(-1, D)
        out.append(rhat_allowance(z64, True, CAP * np.sqrt(v) + delta, CAP * v + 2.1 * delta * np.sqrt(v) + 4 * delta * delta)[0])
    return out


def check_statistic(got_bulk, got_tail, got_rhat, want, label):
    allow = statistic_allowance(want["z_bulk"], want["z_tail"])
    for name, got, ref_v, tol in (("bulk", got_bulk, want["bulk"], allow[0]), ("tail", got_tail, want["tail"], allow[1]),
                                  ("rhat", got_rhat, want["rhat"], np.fmax(allow[0], allow[1]))):
        got, nan = np.asarray(got, np.float64).reshape(-1), np.isnan(ref_v)
        assert np.array_equal(np.isnan(got), nan), (label, name)
        err = np.where(nan, 0.0, np.abs(got - ref_v))
        at = int(err.argmax())
        print("%s %s: max %.5f; largest |error| %.3g, allowed there %.3g" % (label, name, np.nanmax(ref_v), err[at], tol[at]))
        assert (err[~nan] <= tol[~nan]).all(), (label, name)


@pytest.mark.parametrize("which", ["family (601, 37, 5)", "table (400, 64, 3)"])
def test_rank_rhat_against_the_yardstick(gpu, which):
    import torch
    from autoreparam_amd import diagnostics
    x = np.array(rank_family(601, 37, 5)) if which.startswith("family") else ref.table_input(0)
    want = ref.rank_rhat(x)
    got = diagnostics.rank_rhat(torch.as_tensor(x, device=gpu))
    check_statistic(got.bulk, got.tail, got.rhat, want, which)
    for name in ("median", "q05", "q95"):
        assert np.array_equal(getattr(got, name), want[name]), name
    assert np.array_equal(got.rows, np.full(x.shape[2], 2 * x.shape[1]))


def both_folds(gpu, want, label, twice=True):
    """check_exact_and_z of the trace want["x"] for fold = 0 and 1 (and, twice, the same bits from a second call)."""
    import torch
    xd = torch.as_tensor(np.array(want["x"]), device=gpu)
    for fold in (0, 1):
        got = device_run(xd, fold)
        check_exact_and_z(got, want, fold, label)
        if twice:
            again = device_run(xd, fold)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, again)), label


@pytest.mark.parametrize("shape", [(1024, 1024, 1), (1025, 1024, 2), (2049, 1024, 1)])
def test_pools_that_take_the_scan_past_one_chunk(gpu, shape):
    """rank_scan_kernel walks a (segment, digit) row's tiles 256 at a time and adds `carry` to `row[j] = carry + ex`:
    256 tiles fill the one chunk exactly (N = 2^20, also `valid == kTile` in every tile of the scatter), 257 put one
    ragged tile into a second chunk, 513 take three.  A lost carry sends every key of tile 256 and later to the front of
    its digit's run.  Element 1 of the middle shape keeps the whole segment in one digit in passes 2 - 4 and ties every
    value with about 4 000 others (the galloping upper bound of rank_score_kernel over long runs).  The middle shape also
    goes through diagnostics.rank_rhat."""
    import torch
    from autoreparam_amd import diagnostics
    x = long_pool(*shape)
    N = shape[0] * shape[1]
    assert (N + 4095) // 4096 == {1024: 256, 1025: 257, 2049: 513}[shape[0]]
    if shape[2] == 1:
        both_folds(gpu, yardstick(x), "long pool %s" % (shape,), twice=False)
        return
    want = ref.rank_rhat(x)                                   # the ranks once: for the statistic and for the outputs
    both_folds(gpu, dict(x=x, N=N, rank2=(want["rank2_bulk"], want["rank2_tail"]), z=(want["z_bulk"], want["z_tail"]),
                         median=ref.median(x), quantiles=ref.quantiles(x, PROBS)), "long pool %s" % (shape,), twice=False)
    got = diagnostics.rank_rhat(torch.as_tensor(np.array(x), device=gpu))
    check_statistic(got.bulk, got.tail, got.rhat, want, "long pool %s" % (shape,))
    for name in ("median", "q05", "q95"):
        assert np.array_equal(getattr(got, name), want[name]), name


@pytest.mark.parametrize("shape", [(40, 13, 129), (33, 9, 200), (17, 5, 256), (17, 5, 257)])
def test_more_than_128_elements(gpu, shape):
    """rank_key_kernel with blockIdx.y > 0: `d0 = blockIdx.y * dt` in the load and in the store
    `keys[(d0 + dd) * N + i0 + r]`, a last block of 1, 72 or 128 elements (`cols = min(dt, D - d0)`, LDS pitch
    `cols | 1`), three blocks at D = 257 -- where rank_order_stat_kernel takes a second workgroup (`d = blockIdx.x *
    kThreads + threadIdx.x`).  Element d and element d - 128 have different pools, so a block stored to, or read from,
    the segments of another cannot pass."""
    want = reference(*shape)
    srt = np.sort(ref.pools(want["x"]), axis=1)
    assert all(not np.array_equal(srt[d], srt[d - 128]) for d in range(128, shape[2]))
    both_folds(gpu, want, "family %s" % (shape,))


def test_chain_sub_range_view_of_200_elements_is_bitwise_the_contiguous_result(gpu):
    """xd[:, 2:7, :] of (33, 9, 200) in place: rank_key_kernel's `s * stride + c * D + d0 + dd` with stride > C D and
    d0 = 128; the bits of the same chains passed contiguously, and the yardstick's values."""
    import torch
    S, Cn, D = 33, 9, 200
    want = reference(S, Cn, D, 2, 7)
    srt = np.sort(ref.pools(want["x"]), axis=1)
    assert all(not np.array_equal(srt[d], srt[d - 128]) for d in range(128, D))
    xd = torch.as_tensor(np.array(rank_family(S, Cn, D)), device=gpu)
    view = xd[:, 2:7, :]
    assert not view.is_contiguous()
    for fold in (0, 1):
        a, b = device_run(view, fold), device_run(view.contiguous(), fold)
        assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))
        check_exact_and_z(a, want, fold, "view [:, 2:7, :] of (33, 9, 200)")


@pytest.mark.parametrize("shape", [(9, 7, 3), (8, 8, 3), (13, 5, 3), (65, 63, 3), (64, 64, 3), (241, 17, 3), (128, 64, 3),
                                   (4096, 1, 2), (1, 4097, 2)])
def test_pools_at_the_edges_of_the_sort_tile_and_of_the_key_tile(gpu, shape):
    """N = 63, 64, 65: `rows = min(kRows, N - i0)` of rank_key_kernel one short of, at and one past its 64 rows.
    N = 4 095, 4 096, 4 097, 8 192: `valid = min(kTile, N - i0)` of rank_scatter_kernel with one 0xffffffff padding key,
    none, a second tile of one key, two full tiles; `i < N` of rank_hist_kernel likewise.  (4096, 1, 2): one chain
    (`s = i / C` with C = 1).  (1, 4097, 2): one row, with the row_stride = C D that diagnostics.rank_normalize passes
    for S = 1."""
    both_folds(gpu, reference(*shape), "family %s" % (shape,))


def test_infinities_order_as_numbers(gpu):
    """include/autoreparam.h: "+-inf order as numbers".  1 % of element 0 of (600, 40, 7) at +inf, 1 % at -inf: key_of
    gives them the largest and the smallest keys of the pool, the median stays finite, and folded both are
    |+-inf - median| = +inf -- one tie run at the top (ranked_value in rank_key_kernel and in rank_score_kernel)."""
    x = np.array(rank_family(600, 40, 7))
    u = np.random.RandomState(11).rand(600, 40)
    x[:, :, 0][u < 0.01] = np.float32(np.inf)
    x[:, :, 0][u > 0.99] = np.float32(-np.inf)
    assert 150 < np.isposinf(x[:, :, 0]).sum() < 350 and 150 < np.isneginf(x[:, :, 0]).sum() < 350
    want = yardstick(x)
    assert np.isfinite(want["median"]).all() and np.isinf(want["quantiles"]).sum() == 0
    n_inf = int(np.isinf(x[:, :, 0]).sum())
    assert (want["rank2"][1][:, :, 0][np.isinf(x[:, :, 0])] == 2 * 24000 - n_inf).all()      # the folded tie at the top
    both_folds(gpu, want, "(600, 40, 7) with +-inf in element 0")


def test_nan_in_one_element_leaves_the_others_specified(gpu):
    """include/autoreparam.h: "A NaN neither faults nor hangs; the results of an element that holds one are
    unspecified."  NaNs of both signs in element 1 of (600, 40, 7): both folds return and synchronise (every loop of
    rank_score_kernel halves or doubles a bounded range whatever the order of the keys), and every output of the six
    other elements is the yardstick's on those elements alone.  Nothing is asserted about element 1."""
    import torch
    x = np.array(rank_family(600, 40, 7))
    nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x7fffffff], np.uint32).view(np.float32)
    rs = np.random.RandomState(12)
    for v in nans:
        x[rs.randint(600), rs.randint(40), 1] = v
    assert np.isnan(x[:, :, 1]).sum() >= 4 and not np.isnan(np.delete(x, 1, axis=2)).any()
    keep = [0, 2, 3, 4, 5, 6]
    want = yardstick(np.ascontiguousarray(x[:, :, keep]))
    xd = torch.as_tensor(x, device=gpu)
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))      # (the payloads reach the device)
    for fold in (0, 1):
        z, r2, med, q = device_run(xd, fold)
        torch.cuda.synchronize()
        check_exact_and_z((z[:, :, keep], r2[:, :, keep], med[keep], q[:, keep]), want, fold,
                          "(600, 40, 7) with NaN in element 1, elements %s" % (keep,))


def test_argument_forms_of_the_c_api(gpu):
    """arp_rank_normalize through ctypes on (64, 64, 3), N = 4 096: fold = 1 with median == NULL (`med = median ? median
    : ws + L.med`) gives the bits of the call that passes a median; rank2 == NULL with quantiles (`if (rank2) rank2[e] =
    r2`); quantiles == NULL with n_probs > 0 (`want_q`) returns 0 with the same z; probabilities at and beyond the clamp
    `k = !(pk >= 1) ? 1 : pk >= N ? N : pk` give the yardstick's order statistics."""
    import torch
    from autoreparam_amd import _lib
    L = _lib.lib()
    S, Cn, D = 64, 64, 3
    want = reference(S, Cn, D)
    x = torch.as_tensor(np.array(want["x"]), device=gpu)
    need = int(L.arp_rank_workspace_bytes(S, Cn, D, 1))
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    assert need > 0 and ws.data_ptr() % 256 == 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    probs = (-0.1, 0.0, 1e-12, 0.5, 1.0, 1.5)
    pr = (C.c_double * len(probs))(*probs)

    def call(fold, rank2=True, median=True, quantiles=True, n_probs=len(probs)):
        z = torch.full((S, Cn, D), float("nan"), dtype=torch.float32, device=gpu)
        r2 = torch.full((S, Cn, D), -1, dtype=torch.int32, device=gpu) if rank2 else None
        med = torch.full((D,), float("nan"), dtype=torch.float32, device=gpu) if median else None
        q = torch.full((len(probs), D), float("nan"), dtype=torch.float32, device=gpu) if quantiles else None
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        rc = L.arp_rank_normalize(C.c_void_p(x.data_ptr()), S, Cn, D, Cn * D, fold, ptr(z), ptr(r2), ptr(med), pr, n_probs,
                                  ptr(q), C.c_void_p(ws.data_ptr()), need, st)
        assert rc == 0, L.arp_last_error()
        torch.cuda.synchronize()
        return [None if t is None else t.cpu().numpy() for t in (z, r2, med, q)]

    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))
    want_q = ref.quantiles(want["x"], probs)
    srt = np.sort(ref.pools(want["x"]), axis=1)
    assert np.array_equal(want_q, np.stack([srt[:, k] for k in (0, 0, 0, 2047, 4095, 4095)]))
    for fold in (0, 1):
        z, r2, med, q = call(fold)
        assert np.array_equal(r2.view(np.uint32), want["rank2"][fold]) and np.array_equal(med, want["median"])
        assert np.array_equal(q, want_q), fold
        z_a, r2_a, _, q_a = call(fold, median=False)                      # fold = 1: the median lives in the workspace
        assert same(z_a, z) and same(r2_a, r2) and same(q_a, q), fold
        z_b, _, med_b, q_b = call(fold, rank2=False)
        assert same(z_b, z) and same(med_b, med) and same(q_b, q), fold
        z_c, r2_c, med_c, _ = call(fold, quantiles=False)
        assert same(z_c, z) and same(r2_c, r2) and same(med_c, med), fold
        z_d, _, _, _ = call(fold, rank2=False, median=False, quantiles=False)
        assert same(z_d, z), fold


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sees_what_the_classic_statistic_cannot(gpu, seed):
    """64 chains x 400 draws: N(0,1); N(0,1) with 16 chains at 3 x the scale; Cauchy with 16 chains shifted by +2."""
    import torch
    from autoreparam_amd import diagnostics
    xd = torch.as_tensor(ref.table_input(seed), device=gpu)
    classic = diagnostics.rhat_from_sums(diagnostics.fold(*diagnostics.split_moments(xd, True)), 200).rhat
    r = diagnostics.rank_rhat(xd)
    print("seed %d: classic %s bulk %s tail %s" % (seed, classic, r.bulk, r.tail))
    assert (classic < 1.01).all()
    assert r.tail[1] > 1.04 and r.bulk[2] > 1.04 and r.rhat[0] < 1.01


def test_error_paths_return_1_with_a_message_and_leave_the_context_usable(gpu):
    import torch
    from autoreparam_amd import _lib
    L = _lib.lib()
    S, Cn, D = 8, 4, 3
    x = torch.randn(S, Cn, D, device=gpu)
    z = torch.empty_like(x)
    need = int(L.arp_rank_workspace_bytes(S, Cn, D, 0))
    assert need > 0 and need == int(L.arp_rank_workspace_bytes(S, Cn, D, 1))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=gpu)
    assert ws.data_ptr() % 256 == 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(trace=x.data_ptr(), s=S, c=Cn, stride=Cn * D, zp=z.data_ptr(), wp=ws.data_ptr(), wb=need):
        return L.arp_rank_normalize(C.c_void_p(trace), s, c, D, stride, 0, C.c_void_p(zp), None, None, None, 0, None,
                                    C.c_void_p(wp), wb, st)

    for label, kw, word in (("null z", dict(zp=0), b"z"), ("row_stride < C * D", dict(stride=Cn * D - 1), b"row_stride"),
                            ("workspace too small", dict(wb=need - 1), b"workspace"),
                            ("no workspace", dict(wp=0), b"workspace"),
                            ("misaligned workspace", dict(wp=ws.data_ptr() + 4), b"aligned"),
                            ("N >= 2^31", dict(s=1 << 16, c=1 << 15, stride=(1 << 15) * D), b"2^31")):
        assert call(**kw) == 1, label
        assert word in L.arp_last_error(), (label, L.arp_last_error())
    assert int(L.arp_rank_workspace_bytes(1 << 16, 1 << 15, D, 0)) == 0
    assert call() == 0
    torch.cuda.synchronize()
    want = ref.z_scores(ref.rank2(x.cpu().numpy()), S * Cn)
    assert np.abs(z.cpu().numpy() - want).max() <= Z_TOL * max(1.0, np.abs(want).max())


@pytest.fixture(scope="module")
def cli_rank_run(gpu, tmp_path_factory):
    """The 8-schools NCP flow of test_gpu_rhat.py::cli_run: VI, one tuning run, then the sampling run as it is by default
    and (in a copy of the directory made before it) with --rank_normalized_rhat; every chain's trace saved."""
    d = str(tmp_path_factory.mktemp("rank_cli"))
    plain, ranked = os.path.join(d, "plain"), os.path.join(d, "ranked")
    common = ["--model=8schools", "--method=NCP", "--num_chains=%d" % CHAINS, "--seed=4"]
    hm = ["--num_samples=%d" % SAMPLES, "--num_burnin_steps=600", "--num_adaptation_steps=400"]
    _run(common + ["--results_dir=" + plain, "--inference=VI", "--num_optimization_steps=600"])
    _run(common + ["--results_dir=" + plain, "--inference=HMCtuning", "--num_leapfrog_steps=4"] + hm)
    shutil.copytree(plain, ranked)
    _run(common + ["--results_dir=" + plain, "--inference=HMC", "--num_chains_to_save=%d" % CHAINS] + hm)
    _run(common + ["--results_dir=" + ranked, "--inference=HMC", "--num_chains_to_save=%d" % CHAINS,
                   "--rank_normalized_rhat"] + hm)
    return plain, ranked


def test_cli_end_to_end(cli_rank_run):
    plain, ranked = cli_rank_run
    r0 = json.load(open(os.path.join(plain, "NCP_tied.json")))
    r = json.load(open(os.path.join(ranked, "NCP_tied.json")))
    assert set(r) == set(r0) | set(RANK_KEYS) and not set(RANK_KEYS) & set(r0)
    for k in RANK_KEYS:
        assert isinstance(r[k], list) and len(r[k]) == 1 and k not in r["tuning_runs"][0], k
    assert r["rank_rhat_chains"] == [CHAINS] == r["split_rhat_chains"]
    assert 0 < r["rank_rhat_time_sec"][0] <= r["diagnostics_time_sec"][0] < 60
    sp, x = _packed_trace(ranked)
    assert np.array_equal(x, _packed_trace(plain)[1])
    z0, z = np.load(os.path.join(plain, "NCP_tied_rhat.npz")), np.load(os.path.join(ranked, "NCP_tied_rhat.npz"))
    assert not [f for f in z0.files if f.startswith(RANK_FAMILIES)]
    assert sorted(z.files) == sorted(z0.files + ["%s/%s" % (k, n) for k in RANK_FAMILIES for n in sp.part_names])
    for f in z0.files:
        assert np.array_equal(z[f], z0[f], equal_nan=True), f

    def flat(key):
        parts = [z["%s/%s" % (key, n)] for n in sp.part_names]
        assert [p.shape for p in parts] == [tuple(s) for s in sp.part_shapes], key
        return np.concatenate([p.reshape(-1) for p in parts])

    want = ref.rank_rhat(x)
    bulk, tail = flat("rank_rhat_bulk"), flat("rank_rhat_tail")
    check_statistic(bulk, tail, np.fmax(bulk, tail), want, "cli")
    for key, name in (("posterior_median", "median"), ("posterior_q05", "q05"), ("posterior_q95", "q95")):
        assert np.array_equal(flat(key), want[name]), key
    allow = statistic_allowance(want["z_bulk"], want["z_tail"])
    for key, ref_v, tol in (("rank_rhat_bulk_max", want["bulk"], allow[0]), ("rank_rhat_tail_max", want["tail"], allow[1]),
                            ("rank_rhat_max", want["rhat"], np.fmax(allow[0], allow[1]))):
        assert abs(r[key][0] - np.nanmax(ref_v)) <= np.nanmax(tol), key
