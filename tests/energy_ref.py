"""Yardstick of the energy probe (arp_energy_probe): a float64 replay in plain numpy around the oracle's log density
and gradient -- the kernel's half-kick / drift / kick-drift order, with the momenta the device drew (its `p_out`) -- and
the same replay in numpy float32, which exists only to calibrate the tolerances on the CPU: the bars of
tests/test_gpu_energy.py come from the project's existing tests, and tests/test_energy_host.py checks that a second
correct float32 implementation stays inside them for every case below BEFORE the device is asked to.

Also the cases themselves (models, lanes per chain, row counts, step sizes), shared by the two test modules."""
import numpy as np

import helpers

K_BLOCK = 256     # threads of a probe workgroup (arp_device.h: kBlock)

# (model, lanes per chain, engine options): 8 schools at 1, 2 and 8 lanes, German credit at 4 lanes in both matrix-core
# forms and at 8 lanes, the packed families (radon, election) on the generic lane model the probe instantiates
CASES = [("8schools", 1, ()), ("8schools", 2, ()), ("8schools", 8, ()), ("funnel", 1, ()), ("radon_MA", 4, ()),
         ("radon_MA", 16, ()), ("radon_sd_AZ", 8, ()), ("election", 4, ()), ("election", 16, ()), ("electric", 8, ()),
         ("time_series", 4, ()), ("time_series", 16, ()), ("german", 4, (("german_math", "f32"),)),
         ("german", 4, (("german_math", "bf16x3"),)), ("german", 8, ())]
KINDS = ("CP", "NCP", "VIP")
LEAPFROGS = (1, 4)            # 1: no interior step
BIG_KIND = "VIP"              # the parameterisation that also runs the more-than-one-workgroup row count
# fraction of 1 / sqrt(|diag Hessian| + 1) the step sizes take, per model: 0.05 is what tests/test_gpu_hmc.py runs its
# trajectories at; smaller where the float32 replay needs it to stay inside the bars (tests/test_energy_host.py).  electric
# and time_series sit at |logp| ~ 1e6 and ~ 1e9 at these states: four float32 ulps of that, the energy-error bar, is less
# than the rounding of one sequential float32 sum of the log density (electric) and than the gradient times the rounding
# of the state itself (time_series), so the replay only gets inside once the steps are so short that both ends of the
# trajectory round alike (DESIGN.md section 5 has the scan)
FRAC = {"election": 0.005, "electric": 1e-6, "time_series": 1e-5}
STATE_SCALE = 0.1             # helpers.states(scale=...), as tests/test_gpu_hmc.py
STATE_TOL = 1e-4              # of max|q| + 1: what tests/test_gpu_hmc.py holds states to, every model


def frac(mname):
    return FRAC.get(mname, 0.05)


def row_counts(lanes, kind):
    """A single row, a ragged wave (one row more than a wave64 holds) and, for one parameterisation per model, three rows
    more than a workgroup holds."""
    return (1, 64 // lanes + 1) + ((K_BLOCK // lanes + 3,) if kind == BIG_KIND else ())


def eps0(orc, sp, a, b, x, fr):
    """The rule of `_eps0` in tests/test_gpu_hmc.py: a stable per-element step, fr / sqrt(|diag Hessian| + 1), from
    finite differences of the oracle gradient at the first state."""
    x0 = x[:1].astype(np.float64)
    _, g0 = orc.logp_grad(x0, a, b)
    h = 1e-4
    diag = np.zeros(sp.D)
    for d in range(sp.D):
        xp = x0.copy(); xp[0, d] += h
        diag[d] = -(orc.logp_grad(xp, a, b)[1][0, d] - g0[0, d]) / h
    return (fr / np.sqrt(np.abs(diag) + 1.0)).astype(np.float32)


def kappas(n, seed):
    """Per-row step multipliers from [0.5, 1.5]."""
    return (0.5 + np.random.RandomState(seed).rand(n)).astype(np.float32)


def replay(orc, a, b, x, p, eps, kappa, L, dtype=np.float64):
    """One leapfrog trajectory of L steps per row of x [N, D] from the momenta p [N, D]: steps eps[d] * kappa[r] (kappa None:
    1); half kick, drift, L - 1 x (gradient, full kick, drift), gradient, closing half kick.  Every operation in `dtype`.
    Returns lp0, ke0, lp1, ke1 [N] and the end state q1 [N, D]."""
    dt = np.dtype(dtype).type
    q = np.array(x, dtype)
    p = np.array(p, dtype)
    e = np.asarray(eps, dtype)[None, :] * (dt(1) if kappa is None else np.asarray(kappa, dtype)[:, None])
    half = dt(0.5)
    with np.errstate(all="ignore"):
        lp0, g = orc.logp_grad(q, a, b, dtype=dtype)
        ke0 = half * (p * p).sum(axis=1, dtype=dtype)
        p = p + half * e * g
        q = q + e * p
        for _ in range(1, int(L)):
            _, g = orc.logp_grad(q, a, b, dtype=dtype)
            p = p + e * g
            q = q + e * p
        lp1, g = orc.logp_grad(q, a, b, dtype=dtype)
        p = p + half * e * g
        ke1 = half * (p * p).sum(axis=1, dtype=dtype)
    return lp0, ke0, lp1, ke1, q


def energy_error(lp0, ke0, lp1, ke1):
    with np.errstate(all="ignore"):
        return (np.asarray(lp0, np.float64) - np.asarray(lp1, np.float64)) + (np.asarray(ke1, np.float64) - np.asarray(ke0, np.float64))


def bars(ref, p):
    """The tolerances of one case from its float64 replay `ref` = (lp0, ke0, lp1, ke1, q1) and momenta p: dict of
    (reference, tolerance) per checked quantity -- lp0 as tests/test_gpu_density.py holds arp_logp_grad, ke0 to
    1/2 |p|^2 at a relative 2e-5 (a float32 sum of D <= 256 non-negative terms is off by at most D 2^-24 relative), the
    energy error to helpers.margin_tol of the largest energy term, the end state to STATE_TOL (max|q| + 1)."""
    lp0, ke0, lp1, ke1, q1 = ref
    escale = np.max(np.abs([lp0, lp1, ke0, ke1]), axis=0)
    half_p2 = 0.5 * (np.asarray(p, np.float64) ** 2).sum(axis=1)
    return {"lp0": (lp0, 2e-6 * max(1.0, float(np.abs(lp0).max())) + 1e-3),
            "ke0": (half_p2, 2e-5 * half_p2),
            "dh": (energy_error(lp0, ke0, lp1, ke1), helpers.margin_tol(escale)),
            "q": (q1, STATE_TOL * (float(np.abs(q1).max()) + 1.0))}


def ratios(got, ref, p):
    """Largest deviation / tolerance per checked quantity of `got` = (lp0, ke0, lp1, ke1, q1) against the replay `ref`."""
    lp0, ke0, lp1, ke1, q1 = got
    vals = {"lp0": lp0, "ke0": ke0, "dh": energy_error(lp0, ke0, lp1, ke1), "q": q1}
    out = {}
    for key, (want, tol) in bars(ref, p).items():
        dev = np.abs(np.asarray(vals[key], np.float64) - want)
        tol = np.asarray(tol, np.float64)
        out[key] = float(np.max(dev / (tol[:, None] if dev.ndim == 2 and tol.ndim == 1 else tol)))
    return out
