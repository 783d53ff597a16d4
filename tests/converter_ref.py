"""Yardstick of the state converters (to_centered / from_centered in every kernel form): the float64 oracle's
`transform`, element by element, with the error counted in units that follow the conditioning of the element.

  unit_e = 2^-24 max(|want_e|, |inp_e|, 1) + s_e

The first term is the float32 rounding of the element itself and of the input it was formed from (a CP element is
mu + (x - mu): the cancellation leaves the rounding of the larger operand behind).  s_e is the first-order movement of
want_e when EVERY input element moves by a relative 2^-24 -- what no float32 implementation can avoid, since its inputs
are rounded so -- read off the float64 oracle: the largest movement over N_PERT random-sign perturbations of relative
size PERT = 2^-20, divided by PERT / 2^-24 = 16 (fixed seed).  It covers amplification: NCP forward multiplies by
exp(log-scale), time_series sums 60 latents along the chain.

The allowance of a case is max(4 R32, 16) units, R32 being the float32 ORACLE's worst ratio on the same inputs: the
factor 4 is for the device's one-ulp exp / log against libm's half-ulp ones, fused multiply-adds and the lane-wise
order of time_series' cumulative sums; the floor of 16 is the CP-identity bar of test_gpu_density.py
(atol 8e-7 at |x| <= 1 = 13.4 x 2^-24) rounded up, where R32 = 0 because the oracle copies.
tests/test_converter_host.py keeps the float32 oracle at or below 16 units on a grid of models, parameterisations and
state scales, and shows that two deliberate slips exceed the allowance.  No element is excused anywhere.
"""
import numpy as np

U24 = 2.0 ** -24
PERT = 2.0 ** -20
N_PERT = 8
SEED = 24
FACTOR, FLOOR = 4.0, 16.0
BIG = 2.0 ** 100


def _finite(v, what):
    assert np.isfinite(v).all() and (np.abs(v) < BIG).all(), "%s: the float64 yardstick is not finite below 2^100" % what


def want_and_unit(orc, inp, a, b, to_centered, what=""):
    """(want, unit) float64 [n, D] for the float32 inputs `inp` [n, D]."""
    x = np.ascontiguousarray(inp, np.float64)
    want = orc.transform(x, a, b, to_centered, dtype=np.float64)
    _finite(want, what)
    rs = np.random.RandomState(SEED)
    s = np.zeros_like(want)
    for _ in range(N_PERT):
        sign = np.where(rs.rand(*x.shape) < 0.5, -1.0, 1.0)
        moved = orc.transform(x * (1.0 + PERT * sign), a, b, to_centered, dtype=np.float64)
        _finite(moved, what)
        np.maximum(s, np.abs(moved - want), out=s)
    unit = U24 * np.maximum(np.maximum(np.abs(want), np.abs(x)), 1.0) + s * (U24 / PERT)
    return want, unit


def ratio(got, want, unit):
    """Worst |got - want| / unit over every element; NaN if any element of `got` is not finite."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float("nan")
    return float((np.abs(got - want) / unit).max()) if got.size else 0.0


def allowance(r32):
    return max(FACTOR * r32, FLOOR)


def measure(orc, inp, a, b, to_centered, got, period=0, what=""):
    """(worst ratio of `got`, R32, allowance, index of the worst element).  `inp` / `got` are [n, D] (leading axes are
    flattened).  period > 0: row r of `inp` repeats row r % period (asserted), and the oracle is asked for the first
    `period` rows only -- every row of `got` is still compared."""
    D = np.shape(inp)[-1]
    inp = np.ascontiguousarray(inp, np.float32).reshape(-1, D)
    got = np.asarray(got).reshape(-1, D)
    n = inp.shape[0]
    assert got.shape == inp.shape, (got.shape, inp.shape)
    if period and n > period:
        idx = np.arange(n) % period
        assert np.array_equal(inp, inp[:period][idx])
        base = inp[:period]
    else:
        idx, base = None, inp
    want, unit = want_and_unit(orc, base, a, b, to_centered, what)
    r32 = ratio(orc.transform(base, a, b, to_centered, dtype=np.float32), want, unit)
    assert r32 == r32, "%s: the float32 oracle is not finite" % what
    if idx is not None:
        want, unit = want[idx], unit[idx]
    r = ratio(got, want, unit)
    if r == r:
        at = np.unravel_index(int(np.argmax(np.abs(got.astype(np.float64) - want) / unit)), want.shape)
    else:
        at = tuple(int(v[0]) for v in np.nonzero(~np.isfinite(got)))
    return r, r32, allowance(r32), at


def check(orc, inp, a, b, to_centered, got, period=0, what="", log=None):
    """Hold `got` to orc.transform(inp.astype(float64), a, b, to_centered) within max(4 R32, 16) units, every element.
    Returns the worst ratio; `log` (a dict) collects the worst (ratio, R32) seen under its key "worst"."""
    r, r32, allow, at = measure(orc, inp, a, b, to_centered, got, period, what)
    if log is not None:
        w = log.get("worst", (0.0, 0.0))
        log["worst"] = (max(w[0], r) if r == r else float("nan"), max(w[1], r32))
    assert r <= allow, "%s %s: %.4g units at element %s, allowance %.4g (R32 = %.4g)" % (
        what, "to_centered" if to_centered else "from_centered", r, at, allow, r32)
    return r


class GammaScaleOracle(object):
    """German credit with Gamma-prior scales behind OracleModel.transform's signature: gammascale_ref.GermanRef is a
    float64 restatement written from the model's formulas.  It has no float32 arithmetic of its own, so its `float32`
    answer is the float64 one rounded once (R32 <= 1/2 by construction) and the allowance of these cases is the floor."""

    def __init__(self, ref):
        self.ref = ref
        self.D = ref.D

    def transform(self, x, a, b, to_centered=True, dtype=np.float64):
        x64 = np.ascontiguousarray(x, dtype).astype(np.float64)
        out = self.ref.to_centered(x64, a, b) if to_centered else self.ref.from_centered(x64, a, b)
        return np.ascontiguousarray(out, dtype)


# ---------------------------------------------------------------------------
# The cases the CPU guard and the GPU tests share
# ---------------------------------------------------------------------------
SCALES = (0.1, 0.3, 1.5)
KINDS = (("CP", 0), ("NCP", 0), ("VIP", 0), ("VIP", 1), ("B1", 0), ("B1", 1), ("VIPEDGE", 0))


def params(sp, kind, seed=0):
    """helpers.params, plus 'VIPEDGE': a VIP vector whose `a` cycles through exact 0, exact 1, 1e-6, 1 - 1e-6 and a free
    value (the period 5 is coprime to every lane count, so every lane meets every value)."""
    import helpers
    if kind != "VIPEDGE":
        return helpers.params(sp, kind, seed)
    a, b = helpers.params(sp, "VIP", 7 + seed)
    edge = np.array([0.0, 1.0, 1e-6, 1.0 - 1e-6], np.float32)
    a = a.copy()
    for k in range(4):
        a[k::5] = edge[k]
    return a, b


def states(sp, n, seed, scale, to_centered):
    """Inputs of one direction: sampler-coordinate states are helpers.states; centred inputs are drawn the same way (every
    real vector is a centred state of these models)."""
    import helpers
    return helpers.states(sp, n, seed=seed + (0 if to_centered else 100), scale=scale)
