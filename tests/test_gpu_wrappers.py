"""The Python wrappers of the diagnostics entry points against a raw ctypes call of the same entry point.

Every wrapper goes through _lib.call; the raw call here does not: it allocates its own outputs and its own workspace,
sized by the library's sizing function, and passes (pointer, bytes, stream) itself.  Same input, same entry point, so the
outputs must agree bit for bit -- compared as integers, so that NaN is a result like any other.  The shapes are the
smallest at which the library's host-only sizing functions change from "no workspace" to "a workspace" (asserted), one
shape each for the entry points that always take one, and an inner block of chains of a wider trace (the row_stride
path) for one wrapper with a workspace and one without."""
import numpy as np
import pytest
import torch

import helpers
from autoreparam_amd import _lib, diagnostics, engine

pytestmark = pytest.mark.gpu


def bits(t):
    """An integer view of a float tensor: equal bits, not equal values."""
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}.get(t.element_size(), t.dtype)) if t.is_floating_point() else t


def same(got, want, label):
    assert got.shape == want.shape and got.dtype == want.dtype and got.device == want.device, label
    assert torch.equal(bits(got), bits(want)), label


def raw(dev, fn, *args, need=None):
    """fn(*args[, workspace, bytes], stream) with a workspace of `need` bytes allocated here (NULL for 0)."""
    with torch.cuda.device(dev):
        if need is not None:
            ws = torch.empty(need, dtype=torch.uint8, device=dev) if need > 0 else None
            args += (_lib.ptr(ws), need)
        _lib.check(fn(*args, _lib.stream()))
        torch.cuda.synchronize(dev)                    # (the workspace outlives the kernels that use it)


def trace(gpu, S, Cn, D, seed=0, nonfinite=False):
    """float32 [S, Cn, D] noise with a column far from zero; nonfinite: and a NaN and an inf, for the entry points that
    promise what they do with them (their results then hold NaN, which the comparison takes like any other value)."""
    x = np.random.RandomState(seed).randn(S, Cn, D).astype(np.float32)
    x[:, :, 0] += 100.0
    if nonfinite:
        x[S // 2, Cn // 2, D - 1] = np.nan
        x[S - 1, 0, 1 % D] = np.inf
    return torch.as_tensor(x, device=gpu)


def raw_split_moments(x, row_stride, S, Cn, D, split):
    L = _lib.lib()
    P = 2 if split else 1
    mean, var = (torch.empty(P, Cn, D, dtype=torch.float32, device=x.device) for _ in range(2))
    need = int(L.arp_moments_workspace_bytes(S, Cn * D, int(split)))
    raw(x.device, L.arp_split_moments, _lib.ptr(x), S, Cn * D, row_stride, int(split), _lib.ptr(mean), _lib.ptr(var), need=need)
    return mean, var, need


@pytest.mark.parametrize("S,split,workspace", [(513, True, False), (514, True, True), (256, False, False), (257, False, True)])
def test_split_moments(gpu, S, split, workspace):
    x = trace(gpu, S, 1, 3, seed=S, nonfinite=True)
    mean, var, need = raw_split_moments(x, 3, S, 1, 3, split)
    assert (need > 0) == workspace
    got = diagnostics.split_moments(x, split=split)
    same(got[0], mean, "mean")
    same(got[1], var, "var")


def test_fold_and_nested_fold(gpu):
    """The plain calls (no workspace): the flattening of the leading axes included."""
    L = _lib.lib()
    mean, var = diagnostics.split_moments(trace(gpu, 8, 6, 3, seed=1), split=True)            # [2, 6, 3]
    var[1, 2, 0] = float("nan")
    m, v = mean.reshape(-1, 3).contiguous(), var.reshape(-1, 3).contiguous()
    want = torch.empty(5, 3, dtype=torch.float64, device=gpu)
    raw(gpu, L.arp_moments_fold, _lib.ptr(m), _lib.ptr(v), 12, 3, _lib.ptr(want))
    same(diagnostics.fold(mean, var), want, "fold")
    for vv in (v, None):
        want = torch.empty(6, 3, dtype=torch.float64, device=gpu)
        raw(gpu, L.arp_moments_fold_nested, _lib.ptr(m), _lib.ptr(vv), 12, 3, 2, _lib.ptr(want))
        same(diagnostics.nested_fold(mean, None if vv is None else var, 2), want, "nested_fold")


def raw_nested_step_sums(x, row_stride, S, Cn, D, M):
    L = _lib.lib()
    sums = torch.zeros(4, S, D, dtype=torch.float64, device=x.device)
    need = int(L.arp_nested_step_workspace_bytes(S, Cn, D, M))
    raw(x.device, L.arp_nested_step_sums, _lib.ptr(x), S, Cn, D, row_stride, M, _lib.ptr(sums), need=need)
    return sums, need


@pytest.mark.parametrize("Cn,workspace", [(21846, False), (21848, True)])
def test_nested_step_sums(gpu, Cn, workspace):
    S, D, M = 4, 3, 2
    x = trace(gpu, S, Cn, D, seed=Cn, nonfinite=True)
    want, need = raw_nested_step_sums(x, Cn * D, S, Cn, D, M)
    assert (need > 0) == workspace
    same(diagnostics.nested_step_sums(x, M), want, "sums")


@pytest.mark.parametrize("n,workspace", [(256, False), (257, True)])
def test_trajectory_sums(gpu, n, workspace):
    """Engine.trajectory_sums in one chunk: the probe and the transform are the engine's own, arp_jump_sums is called raw."""
    sp = helpers.spec("8schools")
    eng = engine.Engine(sp, gpu)
    eng.set_param(0, helpers.params(sp, "VIP"))
    L, D, Lmax, lanes = _lib.lib(), sp.D, 1, 1
    x = helpers.states(sp, n, seed=n, scale=0.1)
    eps = np.full(D, 1e-2, np.float32)
    kap = np.linspace(0.5, 1.5, n).astype(np.float32)
    got_sums, got_energy = eng.trajectory_sums(x, eps, Lmax, which=0, kappa=kap, seed=7, row_offset=3, lanes=lanes)
    x0 = eng.transform(x, which=0, to_centered=True)
    e, path = eng.trajectory_probe(x, eps, Lmax, which=0, kappa=kap, seed=7, row_offset=3, lanes=lanes, want_path=True,
                                   path_centred=True)
    part = torch.empty(Lmax, 5 + D, dtype=torch.float64, device=gpu)
    need = int(L.arp_jump_workspace_bytes(n, D, Lmax))
    assert (need > 0) == workspace
    raw(gpu, L.arp_jump_sums, _lib.ptr(x0), _lib.ptr(path), _lib.ptr(e), n, D, Lmax, _lib.ptr(part), need=need)
    want = torch.zeros_like(part)
    want += part                                           # (the wrapper adds its chunks to zeros)
    same(got_sums, want, "sums")
    same(got_energy, e, "energy")
    assert float(got_sums[0, 0]) == n


def raw_gram_sums(x, row_stride, S, Cn, D, shift):
    L = _lib.lib()
    sums = torch.zeros(D + 2, D, dtype=torch.float64, device=x.device)
    need = int(L.arp_gram_workspace_bytes(S, Cn, D))
    assert need > 0
    raw(x.device, L.arp_gram_sums, _lib.ptr(x), S, Cn, D, row_stride, _lib.ptr(shift), _lib.ptr(sums), need=need)
    return sums


def test_gram_sums(gpu):
    x = trace(gpu, 4, 2, 3, seed=2, nonfinite=True)
    shift = torch.as_tensor([100.0, 0.5, -0.5], dtype=torch.float32, device=gpu)
    for sh in (None, shift):
        same(diagnostics.gram_sums(x, sh), raw_gram_sums(x, 6, 4, 2, 3, sh), "sums")


@pytest.mark.parametrize("fold", [False, True])
def test_rank_normalize(gpu, fold):
    import ctypes as C
    L = _lib.lib()
    S, Cn, D = 4, 2, 3
    x = trace(gpu, S, Cn, D, seed=3)
    probs = (0.05, 0.95)
    z = torch.empty(S, Cn, D, dtype=torch.float32, device=gpu)
    rank2 = torch.zeros(S, Cn, D, dtype=torch.int32, device=gpu)
    median = torch.full((D,), float("nan"), dtype=torch.float32, device=gpu)
    q = torch.full((2, D), float("nan"), dtype=torch.float32, device=gpu)
    need = int(L.arp_rank_workspace_bytes(S, Cn, D, int(fold)))
    assert need > 0
    raw(gpu, L.arp_rank_normalize, _lib.ptr(x), S, Cn, D, Cn * D, int(fold), _lib.ptr(z), _lib.ptr(rank2), _lib.ptr(median),
        (C.c_double * 2)(*probs), 2, _lib.ptr(q), need=need)
    got_rank2 = torch.zeros_like(rank2)
    got = diagnostics.rank_normalize(x, fold=fold, probs=probs, rank2=got_rank2)
    for g, w, label in zip(got + (got_rank2,), (z, median, q, rank2), ("z", "median", "quantiles", "rank2")):
        same(g, w, label)
    got = diagnostics.rank_normalize(x, fold=fold)                             # no probs, no rank2: NULL operands
    raw(gpu, L.arp_rank_normalize, _lib.ptr(x), S, Cn, D, Cn * D, int(fold), _lib.ptr(z), None, _lib.ptr(median), None, 0, None,
        need=need)
    same(got[0], z, "z")
    same(got[1], median, "median")
    assert got[2] is None


def test_ess_multichain(gpu):
    L = _lib.lib()
    S, Cn, D, n_rho = 8, 2, 3, 3
    x = trace(gpu, S, Cn, D, seed=4)
    threshold = torch.as_tensor([100.0, 0.0, 0.25], dtype=torch.float32, device=gpu)
    for split in (True, False):
        for th in (None, threshold):
            ess = torch.full((D,), float("nan"), dtype=torch.float32, device=gpu)
            max_t = torch.zeros(D, dtype=torch.int32, device=gpu)
            rho = torch.full((n_rho, D), float("nan"), dtype=torch.float32, device=gpu)
            need = int(L.arp_ess_multichain_workspace_bytes(S, Cn, D, int(split)))
            assert need > 0
            raw(gpu, L.arp_ess_multichain, _lib.ptr(x), S, Cn, D, Cn * D, int(split), _lib.ptr(th), _lib.ptr(ess),
                _lib.ptr(max_t), _lib.ptr(rho), n_rho, need=need)
            got = diagnostics.ess_multichain(x, split=split, threshold=th, n_rho=n_rho)
            for g, w, label in zip(got, (ess, max_t, rho), ("ess", "max_t", "rho")):
                same(g, w, "%s split=%s threshold=%s" % (label, split, th is not None))


def test_psis_loo(gpu):
    L = _lib.lib()
    N, R = 3, 7
    ll = torch.as_tensor(-np.abs(np.random.RandomState(5).randn(N, R)).astype(np.float32), device=gpu)
    mask = torch.as_tensor([0, 0, 1, 0, 0, 0, 0], dtype=torch.uint8, device=gpu)
    need = int(L.arp_psis_workspace_bytes(N, R))
    assert need > 0
    for m in (None, mask):
        want = torch.empty(N, 8, dtype=torch.float64, device=gpu)
        raw(gpu, L.arp_psis_loo, _lib.ptr(ll), N, R, R, _lib.ptr(m), _lib.ptr(want), need=need)
        same(diagnostics.psis_loo(ll, m), want, "columns mask=%s" % (m is not None))


def test_inner_block_of_chains(gpu):
    """x[:, 1:3] of [S, 4, 3] is read in place, rows 12 floats apart: with a workspace (gram_sums) and without (split_moments
    of a short trace)."""
    S, D = 6, 3
    wide = trace(gpu, S, 4, D, seed=6, nonfinite=True)
    block = wide[:, 1:3]
    assert not block.is_contiguous() and _lib.trace_view(block, "test")[0] is block
    same(diagnostics.gram_sums(block), raw_gram_sums(block, 4 * D, S, 2, D, None), "gram sums")
    mean, var, need = raw_split_moments(block, 4 * D, S, 2, D, True)
    assert need == 0
    got = diagnostics.split_moments(block, split=True)
    same(got[0], mean, "mean")
    same(got[1], var, "var")
