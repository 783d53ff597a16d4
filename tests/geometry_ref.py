"""Float64 yardstick of the posterior geometry report (autoreparam_amd/diagnostics.py: gram_sums, geometry_from_sums,
scale_coupling, coupling_from_sums; csrc/gram.hip), written from the definitions with numpy alone: no shared code with
the product path."""
import numpy as np

W = 256     # kGramWindow of csrc/gram.hip, restated: the bound below is the header's


def u_rows(x, shift=None):
    """(u, keep): the float32 u = x - shift of every row (one rounding) and which rows have no non-finite element."""
    x = np.asarray(x, np.float32).reshape(-1, np.shape(x)[-1])
    sh = np.zeros(x.shape[1], np.float32) if shift is None else np.asarray(shift, np.float32)
    keep = np.isfinite(x).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x - sh[None, :]).astype(np.float32)
    return u, keep


def gram_ref(x, shift=None):
    """The [D + 2, D] float64 sums arp_gram_sums defines, from float64 sums of the float32 u."""
    u, keep = u_rows(x, shift)
    D = u.shape[1]
    a = u[keep].astype(np.float64)
    out = np.zeros((D + 2, D))
    out[:D] = a.T @ a
    out[D] = a.sum(axis=0)
    out[D + 1, 0] = keep.sum()
    if D > 1:
        out[D + 1, 1] = (~keep).sum()
    return out


def gram_allowance(x, shift=None, factor=2.0):
    """factor x the header's bound, per entry of G: factor (W + 1) 2^-24 sum_r |u_ri u_rj| (the doubling covers the
    bound's second-order terms)."""
    u, keep = u_rows(x, shift)
    a = np.abs(u[keep].astype(np.float64))
    return factor * (W + 1) * 2.0 ** -24 * (a.T @ a)


def geometry_ref(x, eps0=None):
    """dict of the report's figures straight from the rows of x (float64): mean, sd, correlation, eigenvalues (ascending),
    condition_number, max_abs_correlation, pair, step_scaled_eigenvalues, step_scaled_condition_number.  Every column of
    x must vary."""
    a = np.asarray(x, np.float64).reshape(-1, np.shape(x)[-1])
    a = a[np.isfinite(a).all(axis=1)]
    mean = a.mean(axis=0)
    c = np.cov(a, rowvar=False).reshape(a.shape[1], a.shape[1])
    sd = np.sqrt(np.diag(c))
    R = c / np.outer(sd, sd)
    eig = np.linalg.eigvalsh(R)
    off = np.abs(R - np.diag(np.diag(R)))
    i, j = np.unravel_index(int(off.argmax()), off.shape)
    out = dict(mean=mean, sd=sd, cov=c, correlation=R, eigenvalues=eig, condition_number=eig[-1] / eig[0],
               max_abs_correlation=off[i, j], pair=(min(i, j), max(i, j)))
    if eps0 is not None:
        e = np.asarray(eps0, np.float64)
        se = np.linalg.eigvalsh(c / np.outer(e, e))
        out.update(step_scaled_eigenvalues=se, step_scaled_condition_number=se[-1] / se[0])
    return out


def coupling_ref(x, mean=None, sd=None, floor=1e-12):
    """K [D, D] float64: the correlation of u_i with 0.5 log(u_j^2 + floor), u = (x - mean) / sd, diagonal 0."""
    a = np.asarray(x, np.float64).reshape(-1, np.shape(x)[-1])
    mean = a.mean(axis=0) if mean is None else np.asarray(mean, np.float64)
    sd = a.std(axis=0, ddof=1) if sd is None else np.asarray(sd, np.float64)
    u = (a - mean) / sd
    v = 0.5 * np.log(u * u + floor)
    D = a.shape[1]
    K = np.corrcoef(np.concatenate([u, v], axis=1), rowvar=False)[:D, D:].copy()
    np.fill_diagonal(K, 0.0)
    return K
