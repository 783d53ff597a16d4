"""What the PSIS GPU tests share (tests/test_gpu_psis.py, test_gpu_vicheck.py and the two *_shapes files): the calls of
diagnostics.psis_loo / psis_weights on a float32 matrix with a stride, and the comparison of their outputs with the
float64 definition (tests/psis_ref.py, tests/vicheck_ref.py: weights_row).  The exact columns and the a-priori bounds
stand here once; the measured constants belong to the calling file, which hands them in."""
import numpy as np
import torch

import vicheck_ref as vr

FACTOR = 16.0                  # a measured constant is allowed this many times over
U53 = 2.0 ** -53


def device(gpu, ll, mask=None, pad=0):
    """out [N, 8] of diagnostics.psis_loo on ll, its rows R + pad apart."""
    from autoreparam_amd import diagnostics
    N, R = ll.shape
    buf = torch.full((N, R + pad), float("nan"), dtype=torch.float32, device=gpu)      # (the padding is never read)
    buf[:, :R] = torch.as_tensor(ll, device=gpu)
    md = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask, np.uint8), device=gpu)
    view = buf[:, :R] if pad else buf
    assert pad == 0 or (view.stride(0) == R + pad and not view.is_contiguous()) or N == 1
    return diagnostics.psis_loo(view, md).cpu().numpy()


def device_weights(gpu, ll, mask=None, pad=0):
    """(out [N, 8], lw [N, R]) of diagnostics.psis_weights; out is held to psis_loo's on the same view, bit for bit."""
    from autoreparam_amd import diagnostics
    N, R = ll.shape
    buf = torch.full((N, R + pad), float("nan"), dtype=torch.float32, device=gpu)
    buf[:, :R] = torch.as_tensor(ll, device=gpu)
    md = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask, np.uint8), device=gpu)
    view = buf[:, :R] if pad else buf
    out, lw = diagnostics.psis_weights(view, md)
    loo = diagnostics.psis_loo(view, md)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), loo.cpu().numpy().view(np.uint64))       # bit for bit
    return out.cpu().numpy(), lw.cpu().numpy()


def compare(got, ref, ll, mask, what, measured, offset_rows=None, offset_multiple=8.0):
    """The columns against the definition.  measured = (k, sigma relative, elpd): the caller's recorded deviations, of
    which FACTOR times is allowed.  offset_rows: per row, whether elpd_loo gets offset_multiple 2^-53 max|ll| on top (both
    sides form lw + ll and add a shift of the size of max|ll| back, a few roundings each at that magnitude).
    Returns the largest deviations {k, sigma relative, elpd of the rows without that term, elpd of the rows with it in
    units of 2^-53 max|ll|}, for the record."""
    k_measured, sigma_measured, elpd_measured = measured
    keep = np.ones(ll.shape[1], bool) if mask is None else np.asarray(mask) == 0
    worst = np.zeros(4)
    for n in range(ll.shape[0]):
        g, r, row = got[n], ref[n], ll[n][keep].astype(np.float64)
        tag = (what, n)
        assert g[4] == r[4] and g[7] == r[7], (tag, g, r)                              # tail_len, draws_used
        assert g[5] == r[5] or (np.isnan(g[5]) and np.isnan(r[5])), (tag, g[5], r[5])   # cutoff
        for c in (0, 1, 2, 3, 6):                                                      # the same kind of non-finite value
            assert np.isfinite(g[c]) == np.isfinite(r[c]), (tag, c, g, r)
            if not np.isfinite(r[c]):
                assert (np.isnan(g[c]) and np.isnan(r[c])) or g[c] == r[c], (tag, c, g[c], r[c])
        Rk = row.size
        if np.isfinite(r[2]):
            big = np.abs(row).max()
            assert abs(g[2] - r[2]) <= (Rk + 32) * U53 + 4 * U53 * big, (tag, "lppd", g[2], r[2])
        if np.isfinite(r[3]):
            big = np.abs(row).max()
            assert abs(g[3] - r[3]) <= (Rk + 8) * 2.0 ** -52 * r[3] + Rk * (2.0 ** -52 * big) ** 2, (tag, "p_waic", g[3], r[3])
        if np.isfinite(r[1]):
            dk, ds = abs(g[1] - r[1]), abs(g[6] - r[6]) / abs(r[6])
            worst[0], worst[1] = max(worst[0], dk), max(worst[1], ds)
            assert dk <= FACTOR * k_measured, (tag, "pareto_k", g[1], r[1], dk)
            assert ds <= FACTOR * sigma_measured, (tag, "gpd_sigma", g[6], r[6], ds)
        if np.isfinite(r[0]):
            de = abs(g[0] - r[0])
            if offset_rows is not None and offset_rows[n]:
                unit = U53 * np.abs(row).max()
                worst[3] = max(worst[3], de / unit)
                assert de <= FACTOR * elpd_measured + offset_multiple * unit, (tag, "elpd_loo", g[0], r[0], de, de / unit)
            else:
                worst[2] = max(worst[2], de)
                assert de <= FACTOR * elpd_measured, (tag, "elpd_loo", g[0], r[0], de)
    return worst


def compare_weights(lw, ll, mask, names, what, lw_measured, refs=None):
    """Every row against the definition; returns the largest deviation at a smoothed position.  refs: the rows'
    vicheck_ref.weights_row(ll[n], mask), where the caller has them already."""
    worst = 0.0
    for n in range(ll.shape[0]):
        tag = (what, names[n])
        _, ref, tail = vr.weights_row(ll[n], mask) if refs is None else refs[n]
        keep = np.ones(ll.shape[1], bool) if mask is None else np.asarray(mask) == 0
        got = lw[n]
        assert np.all(np.isneginf(got[~keep])), tag
        if np.isnan(ref[keep]).any():
            assert np.isnan(got[keep]).all(), tag
            continue
        kept = ll[n][keep].astype(np.float64)
        raw = np.full(ll.shape[1], -np.inf)
        if kept.size:
            raw[keep] = kept.min() - kept
        differs = np.flatnonzero(keep & (got != raw))
        ref_differs = np.flatnonzero(keep & (ref != raw))
        assert set(differs) <= set(tail) and set(ref_differs) <= set(tail), (tag, differs.size, ref_differs.size, tail.size)
        # (a smoothed weight may coincide with the raw one -- the truncation at 0 of the largest -- on either side: such
        # a position is held to the tolerance below like every other member of the tail)
        clear = ref_differs[np.abs(ref[ref_differs] - raw[ref_differs]) > 1e-9]
        assert set(clear) <= set(differs), tag
        rest = np.setdiff1d(np.flatnonzero(keep), tail)
        assert np.array_equal(got[rest], ref[rest]), tag                                  # raw positions: exact
        if tail.size:
            dev = np.abs(got[tail] - ref[tail]) / np.maximum(np.abs(ref[tail]), 1.0)
            worst = max(worst, float(dev.max()))
            assert dev.max() <= FACTOR * lw_measured, (tag, dev.max())
    return worst


def api_workspace(gpu, N, R):
    """A workspace large enough for either entry point at [N, R], filled with a pattern."""
    from autoreparam_amd import _lib
    need = int(_lib.lib().arp_psis_weights_workspace_bytes(N, R))
    assert need >= int(_lib.lib().arp_psis_workspace_bytes(N, R)) > 0
    return torch.full((need,), 0xA5, dtype=torch.uint8, device=gpu)


def api_call(gpu, ll, mask, ws, weights=False):
    """arp_psis_loo (out [N, 8]) or arp_psis_weights ((out, lw [N, R])) through the C API on the caller's workspace `ws`,
    which a test may so hand from one call to the next; out and lw start from a pattern."""
    from autoreparam_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    N, R = ll.shape
    lld = torch.as_tensor(np.ascontiguousarray(ll, np.float32), device=gpu)
    md = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask, np.uint8), device=gpu)
    out = torch.full((N, 8), -77.0, dtype=torch.float64, device=gpu)
    if not weights:
        _lib.check(L.arp_psis_loo(p(lld), N, R, R, p(md), p(out), p(ws), ws.numel(), _lib.stream()))
        return out.cpu().numpy()
    lw = torch.full((N, R), -77.0, dtype=torch.float64, device=gpu)
    _lib.check(L.arp_psis_weights(p(lld), N, R, R, p(md), p(out), p(lw), R, p(ws), ws.numel(), _lib.stream()))
    return out.cpu().numpy(), lw.cpu().numpy()
