"""GPU: the state converters in every kernel form against the float64 oracle, element by element, in the units of
tests/converter_ref.py (allowance max(4 R32, 16) units; no element excused; tests/test_converter_host.py calibrates it).

 (a) arp_transform, both directions, at the wave / workgroup edges of every lane split and on each side of every row
     count at which the library changes the default instantiation, with guard rows behind the output;
 (b) the centred row a chain kernel records: two hmc_run calls from one state and seed, one recording the sampler's
     coordinates and one the centred row -- the chains are bitwise the same, so row r of the second trace must be the
     float64 centring of row r of the first (the compile-time and packed forms, every lane split, a trace that ends
     inside a wave, German credit's two matrix-core forms whose rows are staged in LDS the next tile overwrites);
 (c) the interleaved sampler's coordinate switch: the recorded pair (x, q = from_centered<M0>(x)), each way;
 (d) the trajectory probe's centred path against the float64 centring of its sampler-coordinate path.

No trajectory parity is needed: a kernel's own (q, x) pairs are enough.  Measured ratios: NOTES_r07.md."""
import numpy as np
import pytest
import torch

import converter_ref as cr
import energy_ref as er
import gammascale_ref
import helpers
import test_gpu_density as tgd
import test_gpu_hmc as tgh
import trajectory_ref as tr

pytestmark = pytest.mark.gpu

# (a) ------------------------------------------------------------------------------------------------------------------
GAMMA = "german_gamma"
MODELS_A = tgd.MODELS + ["radon_MA", "radon_AZ", "radon_sd_AZ", GAMMA]
# chains-per-wave and chains-per-workgroup edges for 4, 8 and 16 lanes per chain
ROWS = (1, 7, 15, 16, 17, 63, 64, 65, 130, 257)
# arp_api.hip: pick -- with no lanes named, the fewest lanes per chain K of the family's table with rows * K >= fill_lanes,
# else the widest (arp_build.hip: kFamilies has fill_lanes; the tables are the inst_*.hip files').  German credit names its
# default (4) and the funnel has one instantiation: no row count changes theirs.
FILL_LANES = {"8schools": (131072, (1, 2, 4, 8)), "radon": (65536, (4, 8, 16)), "election": (131072, (4, 8, 16)),
              "radon_sd": (131072, (8, 16)), "electric": (131072, (8, 16)), "time_series": (65536, (4, 8, 16))}
PERIOD = 257      # the rows of a large case repeat with this (odd) period: the oracle is asked for one period
SENTINEL = -777.25


def _family(mname):
    return "radon_sd" if mname.startswith("radon_sd") else ("radon" if mname.startswith("radon") else mname)


def _switch_rows(mname):
    """One row count on each side of every count at which `pick` changes the default instantiation."""
    fill, ks = FILL_LANES.get(_family(mname), (0, (0,)))
    return tuple(sorted({n for k in ks[:-1] for n in (fill // k - 1, fill // k)}))


def _spec(mname):
    if mname == GAMMA:
        from autoreparam_amd import models
        if GAMMA not in helpers._cache:
            helpers._cache[GAMMA] = models._spec_german_gammascale()
        return helpers._cache[GAMMA]
    return helpers.spec(mname)


def _oracle(oracle_lib, mname):
    sp = _spec(mname)
    if mname == GAMMA:
        return cr.GammaScaleOracle(gammascale_ref.GermanRef(sp.raw["X"], sp.raw["y"]))
    return oracle_lib.OracleModel(sp)


@pytest.fixture(scope="module")
def engines(gpu):
    from autoreparam_amd import engine
    cache = {}

    def get(mname, options=()):
        key = (mname, tuple(options))
        if key not in cache:
            cache[key] = engine.Engine(_spec(mname), gpu)
            for k, v in options:
                cache[key].set_option(k, v)
        return cache[key]
    return get


def _transform_guarded(eng, x, to_centered):
    """arp_transform into a buffer with two guard rows behind row C; returns the C rows after asserting the guards."""
    from autoreparam_amd import _lib
    n, D = x.shape
    xin = torch.as_tensor(x, device=eng.device).contiguous()
    out = torch.full((n + 2, D), SENTINEL, dtype=torch.float32, device=eng.device)
    with torch.cuda.device(eng.device):
        _lib.check(eng._L.arp_transform(eng._h, 0, 0 if to_centered else 1, _lib.ptr(xin), n, _lib.ptr(out), _lib.stream()))
    out = out.cpu().numpy()
    assert (out[n:] == np.float32(SENTINEL)).all(), "arp_transform wrote behind row %d of %d" % (n, n)
    return out[:n]


@pytest.mark.parametrize("kind,seed", cr.KINDS, ids=["%s%d" % k for k in cr.KINDS])
@pytest.mark.parametrize("mname", MODELS_A)
def test_transform_matches_float64(oracle_lib, engines, mname, kind, seed):
    sp = _spec(mname)
    eng = engines(mname)
    orc = _oracle(oracle_lib, mname)
    a, b = cr.params(sp, kind, seed)
    eng.set_param(0, (a, b))
    log = {}
    for to_centered in (True, False):
        for scale in cr.SCALES:
            for n in ROWS:
                x = cr.states(sp, n, n, scale, to_centered)
                got = _transform_guarded(eng, x, to_centered)
                cr.check(orc, x, a, b, to_centered, got, what="%s %s%d scale %g rows %d" % (mname, kind, seed, scale, n), log=log)
        for n in _switch_rows(mname):
            x = cr.states(sp, PERIOD, 9, 0.3, to_centered)[np.arange(n) % PERIOD]
            got = _transform_guarded(eng, x, to_centered)
            cr.check(orc, x, a, b, to_centered, got, period=PERIOD, what="%s %s%d rows %d" % (mname, kind, seed, n), log=log)
    print("converters (a) %s %s%d: worst %.3g units, R32 %.3g" % ((mname, kind, seed) + log["worst"]))


# (b) ------------------------------------------------------------------------------------------------------------------
CHAINS, STEPS, LEAP = 70, 6, 2
KINDS_B = ("CP", "NCP", "VIP", "B1")


def _two_runs(run, gpu, q0, D, trace_chains):
    """`run(state, trace, trace_accept..., trace_centered)` twice from q0: (sampler-coordinate trace, centred trace) after
    asserting that what is recorded changed nothing -- final state, random streams and every accept flag bitwise equal."""
    from autoreparam_amd import engine
    Cn = q0.shape[0]
    out = []
    for centred in (False, True):
        st = engine.ChainState(torch.as_tensor(q0, device=gpu))
        trace = torch.full((STEPS, trace_chains or Cn, D), float("nan"), device=gpu)
        flags = [torch.full((STEPS, Cn), 7, dtype=torch.uint8, device=gpu) for _ in range(2)]
        run(st, trace, flags, centred)
        torch.cuda.synchronize()
        out.append((st, trace.cpu().numpy(), [f.cpu().numpy() for f in flags]))
    (s0, t0, f0), (s1, t1, f1) = out
    assert torch.equal(s0.q, s1.q) and torch.equal(s0.rng, s1.rng)
    assert all(np.array_equal(u, v) for u, v in zip(f0, f1))
    assert np.isfinite(t0).all() and np.isfinite(t1).all()
    return t0, t1


def _recorded_row_case(oracle_lib, engines, mname, kind, lanes, options=(), log=None):
    sp = helpers.spec(mname)
    eng = engines(mname, options)
    orc = oracle_lib.OracleModel(sp)
    a, b = helpers.params(sp, kind)
    eng.set_param(0, (a, b))
    q0 = helpers.states(sp, CHAINS, seed=2, scale=0.1)
    eps0 = tgh._eps0(oracle_lib, sp, a, b, q0, 0.05)
    for trace_chains in (0, 40):            # 40: the trace ends inside a wave at every lane split

        def run(st, trace, flags, centred):
            eng.hmc_run(st, eps0, LEAP, STEPS, n_burnin=0, thin=1, trace=trace, trace_accept=flags[0], trace_centered=centred,
                        seed=9, chain_offset=1000, lanes=lanes, trace_chains=trace_chains)
        q, x = _two_runs(run, eng.device, q0, sp.D, trace_chains)
        cr.check(orc, q, a, b, True, x, what="%s %s lanes=%d %s trace_chains=%d" % (mname, kind, lanes, dict(options), trace_chains),
                 log=log)


@pytest.mark.parametrize("kind", KINDS_B)
@pytest.mark.parametrize("mname", sorted(tgh.LANES))
def test_recorded_row_is_the_centring_of_the_state(oracle_lib, engines, mname, kind):
    log = {}
    for lanes in tgh.LANES[mname]:
        _recorded_row_case(oracle_lib, engines, mname, kind, lanes, log=log)
    print("converters (b) %s %s: worst %.3g units, R32 %.3g" % ((mname, kind) + log["worst"]))


@pytest.mark.parametrize("kind", KINDS_B)
@pytest.mark.parametrize("math", ["bf16x3", "f32"])
def test_recorded_row_german_matrix_core_forms(oracle_lib, engines, math, kind):
    log = {}
    _recorded_row_case(oracle_lib, engines, "german", kind, 4, options=(("german_math", math),), log=log)
    print("converters (b) german %s %s: worst %.3g units, R32 %.3g" % ((math, kind) + log["worst"]))


# (c) ------------------------------------------------------------------------------------------------------------------
PAIRS = {"CP-NCP": (("CP", 0), ("NCP", 0)), "NCP-CP": (("NCP", 0), ("CP", 0)), "VIP-VIP": (("VIP", 0), ("VIP", 1))}
LANES_C = dict(tgh.LANES, radon_AZ=[4, 8, 16])


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("mname", ["radon_PA", "radon_AZ", "election", "german", "time_series"])
def test_interleaved_switch(oracle_lib, engines, mname, pair):
    sp = helpers.spec(mname)
    eng = engines(mname)
    orc = oracle_lib.OracleModel(sp)
    ab0, ab1 = (helpers.params(sp, k, s) for k, s in PAIRS[pair])
    eng.set_param(0, ab0); eng.set_param(1, ab1)
    q0 = helpers.states(sp, CHAINS, seed=2, scale=0.1)
    e0 = tgh._eps0(oracle_lib, sp, ab0[0], ab0[1], q0, 0.05)
    e1 = tgh._eps0(oracle_lib, sp, ab1[0], ab1[1], q0, 0.05)
    logq, logx = {}, {}
    for lanes in LANES_C[mname]:
        for trace_chains in (0, 40):

            def run(st, trace, flags, centred):
                eng.interleaved_run(st, e0, e1, LEAP, LEAP, STEPS, n_burnin=0, thin=1, trace=trace, trace_accept0=flags[0],
                                    trace_accept1=flags[1], trace_centered=centred, seed=9, chain_offset=1000, lanes=lanes,
                                    trace_chains=trace_chains)
            q, x = _two_runs(run, eng.device, q0, sp.D, trace_chains)
            what = "%s %s lanes=%d trace_chains=%d" % (mname, pair, lanes, trace_chains)
            cr.check(orc, x, ab0[0], ab0[1], False, q, what=what, log=logq)
            cr.check(orc, q, ab0[0], ab0[1], True, x, what=what, log=logx)
    print("converters (c) %s %s: q of x worst %.3g units, R32 %.3g; x of q worst %.3g units, R32 %.3g" % (
        (mname, pair) + logq["worst"] + logx["worst"]))


# (d) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,lanes,options", er.CASES, ids=["%s-%d%s" % (m, k, "-" + o[0][1] if o else "") for m, k, o in er.CASES])
def test_probe_centred_path(oracle_lib, engines, mname, lanes, options):
    sp = helpers.spec(mname)
    eng = engines(mname, options)
    orc = oracle_lib.OracleModel(sp)
    n, Lmax = 67, 3
    x = helpers.states(sp, n, seed=6, scale=er.STATE_SCALE)
    for kind in KINDS_B:
        a, b = helpers.params(sp, kind)
        eng.set_param(0, (a, b))
        eps = er.eps0(orc, sp, a, b, x, tr.frac(mname))
        kw = dict(kappa=er.kappas(n, 1), seed=8, row_offset=2, lanes=lanes)
        e_s, path_s = eng.trajectory_probe(x, eps, Lmax, path_centred=False, **kw)
        e_c, path_c = eng.trajectory_probe(x, eps, Lmax, path_centred=True, **kw)
        assert torch.equal(e_s, e_c)
        path_s, path_c = path_s.cpu().numpy(), path_c.cpu().numpy()
        assert np.isfinite(path_s).all() and np.isfinite(path_c).all()
        log = {}
        cr.check(orc, path_s, a, b, True, path_c, what="%s lanes=%d %s %s" % (mname, lanes, dict(options), kind), log=log)
        print("converters (d) %s lanes=%d %s %s: worst %.3g units, R32 %.3g" % ((mname, lanes, dict(options), kind) + log["worst"]))
