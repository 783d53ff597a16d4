"""Yardstick of the trajectory probe (arp_trajectory_probe, arp_jump_sums): `replay_path` is energy_ref.replay returning
the log density, the kinetic energy and the state after EVERY leapfrog step l = 1 ... Lmax -- the kernel's order: half kick,
drift, then per step gradient, (closing half kick into a temporary, for the kinetic energy only), full kick, drift -- in a
chosen dtype; `jump_sums` is the fold in numpy float64.  The cases, row counts, step multipliers and bars are energy_ref's;
the bars are applied at every l.

Step fractions: energy_ref.frac for every model.  The float32 numpy replay stays inside energy_ref.bars at l = 5 for every
model at those fractions (tests/test_trajectory_host.py checks it before the device is asked to), so none is shortened
here (FRAC_L5 is empty; a model that needed it would get its own, smaller fraction there, never a wider bar)."""
import numpy as np

import energy_ref as er

LEAPFROGS_MAX = (1, 5)        # Lmax of the parity cases: 1 (no interior step) and 5
FRAC_L5 = {}                  # model -> step fraction where energy_ref's does not fit at l = 5 (none does not)
DIVERGENCE = 1000.0           # diagnostics.DIVERGENCE_THRESHOLD
JUMP_HEAD = 5                 # rows, divergent, nonfinite, sum of alpha, left_out
JUMP_TILE = 256               # rows of a fold workgroup's tile (csrc/jump.hip: kRows), doubled up to 4 x for large shapes
# allowance of a float64 sum of the fold against numpy's, in units of the sum of |terms|: two ulps of exp, one rounding
# per operation, a tree of at most 32 levels -- not measured (the measured ratio: DESIGN.md section 5)
FOLD_ALLOWANCE = 64.0 * 2.0 ** -52


def jump_tile(n, Lmax):
    """Rows of a fold workgroup's tile for n rows and Lmax steps (csrc/jump.hip: tile_rows): JUMP_TILE, doubled up to
    4 x JUMP_TILE while the launch keeps 2 048 workgroups."""
    rows = JUMP_TILE
    while rows < 4 * JUMP_TILE and (n * Lmax) // (2 * rows) >= 2048:
        rows *= 2
    return rows


def frac(mname):
    return FRAC_L5.get(mname, er.frac(mname))


def replay_path(orc, a, b, x, p, eps, kappa, Lmax, dtype=np.float64):
    """One leapfrog trajectory of Lmax steps per row of x [N, D] from the momenta p [N, D], steps eps[d] * kappa[r] (kappa
    None: 1), every operation in `dtype`.  Returns lp [Lmax + 1, N], ke [Lmax + 1, N] (l = 0: the start; l >= 1: after the
    half kick that would close a trajectory of l steps) and q [Lmax, N, D], the state after step l."""
    dt = np.dtype(dtype).type
    q = np.array(x, dtype)
    p = np.array(p, dtype)
    e = np.asarray(eps, dtype)[None, :] * (dt(1) if kappa is None else np.asarray(kappa, dtype)[:, None])
    half = dt(0.5)
    n, D = q.shape
    lp = np.empty((Lmax + 1, n), dtype)
    ke = np.empty((Lmax + 1, n), dtype)
    path = np.empty((Lmax, n, D), dtype)
    with np.errstate(all="ignore"):
        lp[0], g = orc.logp_grad(q, a, b, dtype=dtype)
        ke[0] = half * (p * p).sum(axis=1, dtype=dtype)
        p = p + half * e * g
        q = q + e * p
        for l in range(1, int(Lmax) + 1):
            lp[l], g = orc.logp_grad(q, a, b, dtype=dtype)
            pe = p + half * e * g
            ke[l] = half * (pe * pe).sum(axis=1, dtype=dtype)
            path[l - 1] = q
            if l < Lmax:
                p = p + e * g
                q = q + e * p
    return lp, ke, path


def ratios_by_step(got, ref, p):
    """Largest deviation / tolerance per quantity of energy_ref.bars over every l = 1 ... Lmax of `got` = (lp, ke, path)
    against the replay `ref`: lp0 and ke0, the energy error of a trajectory of l steps, the state after step l."""
    worst = {}
    for l in range(1, ref[0].shape[0]):
        r = er.ratios((got[0][0], got[1][0], got[0][l], got[1][l], got[2][l - 1]),
                      (ref[0][0], ref[1][0], ref[0][l], ref[1][l], ref[2][l - 1]), p)
        for key, v in r.items():
            worst[key] = max(worst.get(key, 0.0), v) if v == v and worst.get(key, 0.0) == worst.get(key, 0.0) else float("nan")
    return worst


def alphas(energy):
    """(alpha [Lmax, N] float64, divergent, nonfinite [Lmax, N] bool) from energy [Lmax + 1, N, 2] = {lp, ke}: the energy
    error in float64 from the four values as stored, as diagnostics.energy_sums forms it."""
    e = np.asarray(energy).astype(np.float64)
    with np.errstate(all="ignore"):
        dh = (e[0, :, 0][None] - e[1:, :, 0]) + (e[1:, :, 1] - e[0, :, 1][None])
        nonfinite = ~np.isfinite(dh)
        divergent = nonfinite | (dh > DIVERGENCE)
        alpha = np.where(divergent, 0.0, np.minimum(1.0, np.exp(-np.where(divergent, 0.0, dh))))
    return alpha, divergent, nonfinite


def jump_sums(x0, path, energy):
    """The fold in numpy float64: sums [Lmax, 5 + D] -- rows, divergent, nonfinite, sum of alpha, left_out, then
    J[d] = sum over rows of alpha (x_l,d - x_0,d)^2; a row with alpha = 0 is skipped, a term with alpha > 0 that is not
    finite is left out and counted.  The terms are float64; the two sums over rows are accumulated in numpy's long double
    (numpy adds down a column one row after the other: over 10^5 rows a float64 accumulator would itself be off by more
    than the allowance the device is held to)."""
    x0 = np.asarray(x0).astype(np.float64)
    path = np.asarray(path).astype(np.float64)
    Lmax, n, D = path.shape
    alpha, divergent, nonfinite = alphas(energy)
    out = np.zeros((Lmax, JUMP_HEAD + D))
    with np.errstate(all="ignore"):
        for l in range(Lmax):
            diff = path[l] - x0
            term = alpha[l][:, None] * (diff * diff)
            use = (alpha[l] > 0)[:, None] & np.ones((1, D), bool)
            bad = use & ~np.isfinite(term)
            out[l, :JUMP_HEAD] = (n, divergent[l].sum(), nonfinite[l].sum(), alpha[l].sum(dtype=np.longdouble), bad.sum())
            out[l, JUMP_HEAD:] = np.where(use & ~bad, term, 0.0).sum(axis=0, dtype=np.longdouble)
    return out


def sampler_pair(q_before, q_after, alpha, path_l):
    """The statistics of the agreement test.  q_before, q_after [n, D]: centred states before and after one transition of
    the sampler; alpha [n], path_l [n, D]: acceptance probability and centred end state of a fresh-momentum trajectory of
    the sampler's length from q_before.  Returns (z [D], z_total): per element the difference of the mean Metropolis-weighted
    squared jump and the mean realised squared jump in units of sigma, sigma^2 = (var of alpha d^2 + var of realised
    d^2) / n; and the same for the rows' totals with every element standardised by its variance over the rows."""
    q0 = np.asarray(q_before, np.float64)
    n = q0.shape[0]
    w = np.asarray(alpha, np.float64)[:, None] * (np.asarray(path_l, np.float64) - q0) ** 2
    r = (np.asarray(q_after, np.float64) - q0) ** 2
    z = (w.mean(axis=0) - r.mean(axis=0)) / np.sqrt((w.var(axis=0, ddof=1) + r.var(axis=0, ddof=1)) / n)
    v = q0.var(axis=0, ddof=1)
    wt, rt = (w / v).sum(axis=1), (r / v).sum(axis=1)
    z_total = (wt.mean() - rt.mean()) / np.sqrt((wt.var(ddof=1) + rt.var(ddof=1)) / n)
    return z, float(z_total)
