"""CPU: the converter yardstick of tests/converter_ref.py, before the device is held to it.

1. Guard: the float32 oracle -- a second correct float32 implementation -- stays at or below 16 units against the float64
   oracle on a grid of models, parameterisations, state scales and both directions, so the unit cannot be changed into
   one that hollows out tests/test_gpu_converters.py without this test noticing (and 16, the floor of the allowance, is
   not below what a correct implementation needs).
2. Power: a numpy float32 restatement of eight schools' converters is inside the allowance as written, and outside it
   with either of two deliberate slips (one element of `a` moved by 1e-4; the scale taken from the wrong parent)."""
import numpy as np
import pytest

import converter_ref as cr
import helpers

GRID_MODELS = ["8schools", "radon_MN", "radon_PA", "radon_MA", "radon_AZ", "election", "german", "radon_sd_MN", "radon_sd_AZ",
               "funnel", "electric", "time_series"]
GRID_KINDS = [(k, s) for k in ("CP", "NCP", "VIP", "B1") for s in (0, 1)]


@pytest.mark.parametrize("mname", GRID_MODELS)
def test_float32_oracle_stays_within_sixteen_units(oracle_lib, mname):
    sp = helpers.spec(mname)
    orc = oracle_lib.OracleModel(sp)
    worst = (0.0, None)
    for kind, seed in GRID_KINDS:
        a, b = helpers.params(sp, kind, seed)
        for scale in cr.SCALES:
            for to_centered in (True, False):
                x = cr.states(sp, 64, 3, scale, to_centered)
                want, unit = cr.want_and_unit(orc, x, a, b, to_centered, mname)
                r = cr.ratio(orc.transform(x, a, b, to_centered, dtype=np.float32), want, unit)
                assert r == r
                if r > worst[0]:
                    worst = (r, (kind, seed, scale, to_centered))
    print("converter yardstick %s: float32 oracle worst %.3g units at %s" % (mname, worst[0], worst[1]))
    assert worst[0] <= cr.FLOOR, worst


def _schools32(x, a, b, to_centered, slip=None):
    """Eight schools' converters (oracle_impl.h: schools_convert) in numpy float32, one rounding per operation.
    slip "a": a[5] moved by 1e-4; slip "parent": the scale exp((1 - b) .) read from mu, not from log tau."""
    f = np.float32
    x = np.asarray(x, f)
    a = np.array(a, f); b = np.asarray(b, f)
    if slip == "a":
        a[5] += f(1e-4)
    c0 = f(5.0) ** (f(1) - b[0]); c1 = f(5.0) ** (f(1) - b[1])
    out = np.empty_like(x)
    if to_centered:
        mu, lt = c0 * x[:, 0], c1 * x[:, 1]
        out[:, 0], out[:, 1] = mu, lt
        par = mu if slip == "parent" else lt
        out[:, 2:] = mu[:, None] + np.exp((f(1) - b[2:]) * par[:, None]) * (x[:, 2:] - a[2:] * mu[:, None])
    else:
        mu, lt = x[:, 0], x[:, 1]
        out[:, 0], out[:, 1] = mu / c0, lt / c1
        par = mu if slip == "parent" else lt
        out[:, 2:] = a[2:] * mu[:, None] + (x[:, 2:] - mu[:, None]) * np.exp(-(f(1) - b[2:]) * par[:, None])
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("to_centered", [True, False])
def test_the_bar_can_fail(oracle_lib, to_centered):
    sp = helpers.spec("8schools")
    orc = oracle_lib.OracleModel(sp)
    a, b = helpers.params(sp, "VIP", 0)
    for scale in cr.SCALES:
        x = cr.states(sp, 64, 5, scale, to_centered)
        r, r32, allow, _ = cr.measure(orc, x, a, b, to_centered, _schools32(x, a, b, to_centered))
        assert r <= allow, (scale, r, allow)
        for slip in ("a", "parent"):
            bad = _schools32(x, a, b, to_centered, slip)
            rs, _, _, _ = cr.measure(orc, x, a, b, to_centered, bad)
            print("slip %s, scale %g, %s: %.3g units (allowance %.3g; unslipped %.3g)" % (
                slip, scale, "to_centered" if to_centered else "from_centered", rs, allow, r))
            assert rs > allow, (slip, scale, rs, allow)
            with pytest.raises(AssertionError):
                cr.check(orc, x, a, b, to_centered, bad)


def test_switch_row_counts_follow_the_family_table():
    """tests/test_gpu_converters.py puts one row count on each side of every count at which the library changes its default
    instantiation; the counts come from fill_lanes and default_lanes of arp_build.hip: kFamilies, restated there.  This holds
    the restatement to the source, so a retuned table moves the test's row counts with it."""
    import os
    import re
    import test_gpu_converters as tgc
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "autoreparam_amd", "csrc", "arp_build.hip")
    rows = re.findall(r"\{ARP_MODEL_(\w+), build_\w+, \w+_ops, (?:true|false), \d+, (\d+), (\d+), \d+\},", open(src).read())
    names = {"EIGHT_SCHOOLS": "8schools", "RADON": "radon", "GERMAN_CREDIT": "german", "ELECTION": "election",
             "RADON_STDDVS": "radon_sd", "NEALS_FUNNEL": "funnel", "ELECTRIC": "electric", "TIME_SERIES": "time_series"}
    assert sorted(r[0] for r in rows) == sorted(names)
    for model, fill, default in rows:
        name = names[model]
        if name in tgc.FILL_LANES:
            assert int(default) == 0 and tgc.FILL_LANES[name][0] == int(fill), model
        else:
            assert int(default) != 0 or name == "funnel", model     # a named default, or a single instantiation
    assert tgc._switch_rows("radon_MA") == (8191, 8192, 16383, 16384) and tgc._switch_rows("german") == ()


def test_check_excuses_nothing(oracle_lib):
    """One wrong element among many, one NaN, and a yardstick that leaves float64's comfortable range: each is refused."""
    sp = helpers.spec("8schools")
    orc = oracle_lib.OracleModel(sp)
    a, b = helpers.params(sp, "VIP", 0)
    x = cr.states(sp, 300, 5, 0.3, True)
    good = orc.transform(x, a, b, True, dtype=np.float32)
    assert cr.check(orc, x, a, b, True, good) <= cr.FLOOR
    tiled = np.tile(x[:7], (40, 1))
    assert cr.check(orc, tiled, a, b, True, np.tile(good[:7], (40, 1)), period=7) <= cr.FLOOR
    for value in (good[299, 9] * np.float32(1 + 1e-4) + np.float32(1e-4), np.float32("nan")):
        bad = good.copy(); bad[299, 9] = value
        with pytest.raises(AssertionError):
            cr.check(orc, x, a, b, True, bad)
    bad = np.tile(good[:7], (40, 1)); bad[279, 2] += np.float32(1e-3)
    with pytest.raises(AssertionError):
        cr.check(orc, tiled, a, b, True, bad, period=7)
    huge = x.copy(); huge[0, 1] = 1e3          # log tau = 5e3 under NCP: exp leaves float64
    with pytest.raises(AssertionError):
        cr.check(orc, huge, *helpers.params(sp, "NCP"), True, good)
