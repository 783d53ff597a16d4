"""GPU: the energy probe (energy_probe_kernel, arp_energy_probe, Engine.energy_probe, diagnostics.energy_sums,
--energy_diagnostics) -- a fresh-momentum trajectory per state, not a replay of the sampler's own transitions -- against
the float64 replay of tests/energy_ref.py with the momenta the device drew; the momentum streams; planted divergences in
the funnel's neck; agreement with the sampler's own acceptance rate; non-interference; refusals; the CLI.

Measured on an MI355X (largest deviation / tolerance of the parity test, per quantity, over all its cases): DESIGN.md
section 5."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

import energy_ref as er
import helpers

pytestmark = pytest.mark.gpu


def _engine(gpu, mname, options=()):
    from autoreparam_amd import engine
    eng = engine.Engine(helpers.spec(mname), gpu)
    for key, value in options:
        eng.set_option(key, value)
    return eng


def _np(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------
# 1. parity with the float64 replay
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", er.KINDS)
@pytest.mark.parametrize("mname,lanes,options", er.CASES, ids=["%s-%d%s" % (m, k, "-" + o[0][1] if o else "") for m, k, o in er.CASES])
def test_probe_matches_float64_replay(oracle_lib, gpu, mname, lanes, options, kind):
    """lp0, ke0, the energy error and the end state of every probed row against energy_ref.replay in float64 from the
    momenta the device drew (p_out): L = 1 (no interior step) and 4, one row, a ragged wave and (one parameterisation per
    model) more than a workgroup, per-row step multipliers and none.  Bars: energy_ref.bars, none of them measured on the
    code under test (tests/test_energy_host.py holds a float32 numpy replay to the same bars first)."""
    sp = helpers.spec(mname)
    eng = _engine(gpu, mname, options)
    orc = oracle_lib.OracleModel(sp)
    a, b = helpers.params(sp, kind)
    eng.set_param(0, (a, b))
    worst, failed = {}, []
    for n in er.row_counts(lanes, kind):
        x = helpers.states(sp, n, seed=n, scale=er.STATE_SCALE)
        eps = er.eps0(orc, sp, a, b, x, er.frac(mname))
        for L in er.LEAPFROGS:
            for kap in (None, er.kappas(n, n)):
                out, p, q = eng.energy_probe(x, eps, L, which=0, kappa=kap, seed=11, row_offset=5, lanes=lanes,
                                             want_p=True, want_q=True)
                out, p, q = _np(out), _np(p), _np(q)
                assert np.isfinite(out).all() and np.isfinite(p).all()
                ref = er.replay(orc, a, b, x, p, eps, kap, L, np.float64)
                got = (out[:, 0], out[:, 1], out[:, 2], out[:, 3], q)
                for key, r in er.ratios(got, ref, p).items():
                    worst[key] = max(worst.get(key, 0.0), r) if r == r else float("nan")
                    if not r <= 1.0:
                        failed.append((key, n, L, kap is not None, r))
    print("energy probe %s lanes=%d %s %s: deviation / tolerance %s" % (
        mname, lanes, dict(options), kind, {k: round(v, 4) for k, v in worst.items()}))
    assert not failed, failed[:8]


# ---------------------------------------------------------------------------
# 2. the momentum draw
# ---------------------------------------------------------------------------
def test_momentum_draw(gpu):
    """p_out over 8 192 rows of election: every element standard normal (mean and variance within 5 standard errors),
    rows pairwise different, the draw a pure function of (seed, row_offset + row)."""
    sp = helpers.spec("election")
    eng = _engine(gpu, "election")
    eng.set_param(0, "CP")
    n = 8192
    x = helpers.states(sp, n, seed=1, scale=0.1)
    eps = np.full(sp.D, 1e-3, np.float32)

    def draw(rows, seed, offset):
        return _np(eng.energy_probe(x[:rows], eps, 1, seed=seed, row_offset=offset, want_p=True)[1])
    p = draw(n, 3, 0)
    assert p.shape == (n, sp.D) and np.isfinite(p).all()
    p64 = p.astype(np.float64)
    assert np.abs(p64.mean(axis=0)).max() <= 5.0 / np.sqrt(n)
    assert np.abs(p64.var(axis=0) - 1.0).max() <= 5.0 * np.sqrt(2.0 / n)
    assert len({r.tobytes() for r in p}) == n
    assert np.array_equal(p, draw(n, 3, 0))
    assert not np.array_equal(p[:64], draw(64, 4, 0)) and not np.array_equal(p[:64], draw(64, 3, 1))
    k, m = 1000, 300
    assert np.array_equal(draw(m, 3, k), p[k:k + m])


# ---------------------------------------------------------------------------
# 3. planted divergences
# ---------------------------------------------------------------------------
def test_planted_divergences_in_the_funnel(oracle_lib, gpu):
    """Neal's funnel, D = 2: half the rows in the neck (x1 = -12, x2 at that scale), half in the mouth (x1 = +2); steps
    0.1, L = 8.  Centred, every neck row diverges (energy error not finite or above 1000) and no mouth row does; the same
    states non-centred: none at all; the float64 replay classifies every row the same way, every row's float64 energy
    error at least ten tolerances from the threshold; energy_sums counts what the host counts."""
    from autoreparam_amd import diagnostics
    sp = helpers.spec("funnel")
    assert sp.D == 2
    eng = _engine(gpu, "funnel")
    orc = oracle_lib.OracleModel(sp)
    n = 600
    rs = np.random.RandomState(5)
    xc = np.zeros((n, 2), np.float32)
    xc[: n // 2, 0], xc[n // 2:, 0] = -12.0, 2.0
    xc[:, 1] = (np.exp(0.5 * xc[:, 0].astype(np.float64)) * rs.randn(n)).astype(np.float32)
    neck = np.arange(n) < n // 2
    eps = np.full(2, 0.1, np.float32)
    for kind, expect in (("CP", neck), ("NCP", np.zeros(n, bool))):
        a, b = helpers.params(sp, kind)
        eng.set_param(0, (a, b))
        x = _np(eng.transform(xc, which=0, to_centered=False))
        out, p = eng.energy_probe(x, eps, 8, seed=21, want_p=True)
        o = _np(out).astype(np.float64)
        with np.errstate(all="ignore"):
            dh = (o[:, 0] - o[:, 2]) + (o[:, 3] - o[:, 1])
        divergent = ~np.isfinite(dh) | (dh > 1000.0)
        assert np.array_equal(divergent, expect), (kind, int(divergent.sum()))
        ref = er.replay(orc, a, b, x, _np(p), eps, None, 8, np.float64)
        dh64 = er.energy_error(*ref[:4])
        tol = helpers.margin_tol(np.max(np.abs(ref[:4]), axis=0))
        clear = ~np.isfinite(dh64) | (np.abs(dh64 - 1000.0) >= 10.0 * tol)
        assert clear.all(), (kind, int((~clear).sum()))                          # (no row may be left out)
        assert np.array_equal(~np.isfinite(dh64) | (dh64 > 1000.0), expect), kind
        s = _np(diagnostics.energy_sums(out))
        assert s[0] == n and s[1] == divergent.sum() and s[2] == (~np.isfinite(dh)).sum()
        e = diagnostics.energy_from_sums(s, sp.D)
        assert e.divergent == int(expect.sum()) and e.rows == n


# ---------------------------------------------------------------------------
# 4. agreement with the sampler
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mname,kind,frac", [("8schools", "NCP", 0.1), ("radon_MA", "CP", 0.5)])
def test_probe_agrees_with_the_sampler(oracle_lib, gpu, mname, kind, frac):
    """4 096 chains, fixed step, 300 transitions; the probe of the final states with the same steps and leapfrog count:
    its expected acceptance against the sampler's acceptance rate over its last 100 transitions, within 5 sigma of the
    probe's per-row standard error and the standard error of the per-chain rates; no divergent trajectory.  Steps:
    energy_ref.eps0 at the largest of 0.5, 0.3, 0.2, 0.1 at which the float64 replay from the float32 oracle's own final
    states has no divergent row (8 schools non-centred: 183, 11, 2, 0 of 4 096 -- a fixed step meets the tail of log tau)."""
    from autoreparam_amd import diagnostics, engine
    sp = helpers.spec(mname)
    eng = _engine(gpu, mname)
    orc = oracle_lib.OracleModel(sp)
    a, b = helpers.params(sp, kind)
    eng.set_param(0, (a, b))
    Cn, L = 4096, 4
    q0 = helpers.states(sp, Cn, seed=2, scale=0.1)
    eps = er.eps0(orc, sp, a, b, q0, frac)
    st = engine.ChainState(torch.as_tensor(q0, device=gpu))
    eng.hmc_run(st, eps, L, 200, seed=9)
    before = st.accept_count.clone()
    eng.hmc_run(st, eps, L, 100, seed=9)
    rate = _np((st.accept_count - before).to(torch.float64)) / 100.0
    out = eng.energy_probe(st.q, eps, L, seed=33)
    e = diagnostics.energy_from_sums(diagnostics.energy_sums(out), sp.D)
    o = _np(out).astype(np.float64)
    acc = np.minimum(1.0, np.exp(-((o[:, 0] - o[:, 2]) + (o[:, 3] - o[:, 1]))))
    sigma = np.sqrt(acc.var(ddof=1) / Cn + rate.var(ddof=1) / Cn)
    print("energy probe vs sampler %s %s: probe %.4f, sampler %.4f, sigma %.5f" % (mname, kind, e.accept_prob, rate.mean(), sigma))
    assert e.divergent == 0 and e.rows == Cn
    assert abs(e.accept_prob - acc.mean()) < 1e-12
    assert 0.2 < rate.mean() < 0.999                                               # (a step at which the test can tell)
    assert abs(e.accept_prob - rate.mean()) <= 5.0 * sigma


# ---------------------------------------------------------------------------
# 5. non-interference
# ---------------------------------------------------------------------------
def test_probe_changes_nothing(gpu):
    """x is unchanged by a probe, and an hmc_run after a probe is bitwise the run without it."""
    from autoreparam_amd import engine
    sp = helpers.spec("radon_MA")
    eps = np.full(sp.D, 0.05, np.float32)
    q0 = helpers.states(sp, 300, seed=3, scale=0.1)

    def run(probe):
        eng = _engine(gpu, "radon_MA")
        eng.set_param(0, "NCP")
        st = engine.ChainState(torch.as_tensor(q0, device=gpu))
        eng.hmc_run(st, eps, 4, 10, seed=5)
        if probe:
            x = st.q.clone()
            eng.energy_probe(st.q, eps, 4, kappa=st.adapt[:, 0].contiguous(), seed=6, want_p=True, want_q=True)
            assert torch.equal(x, st.q)
        eng.hmc_run(st, eps, 4, 10, seed=5)
        torch.cuda.synchronize()
        return st
    a, b = run(False), run(True)
    for name in ("q", "grad", "logp", "rng", "accept_count", "adapt"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
def test_refusals(gpu):
    """A null handle, x, eps0 or out4, `which` outside 0 / 1, n_rows < 1 and n_leapfrog < 1: non-zero, a message, and
    nothing written to out4."""
    from autoreparam_amd import _lib
    sp = helpers.spec("8schools")
    eng = _engine(gpu, "8schools")
    eng.set_param(0, "CP")
    L = _lib.lib()
    n = 5
    x = torch.zeros(n, sp.D, device=gpu)
    eps = torch.full((sp.D,), 0.1, device=gpu)
    out = torch.full((n, 4), 7.0, device=gpu)
    null = C.c_void_p(0)
    good = dict(m=eng._h, which=0, x=_lib.ptr(x), n=n, L=2, eps=_lib.ptr(eps), out=_lib.ptr(out))
    bad = [dict(m=null), dict(x=null), dict(eps=null), dict(out=null), dict(which=-1), dict(which=2), dict(n=0), dict(n=-3),
           dict(L=0), dict(L=-1)]
    with torch.cuda.device(gpu):
        for change in bad:
            k = dict(good, **change)
            rc = L.arp_energy_probe(k["m"], k["which"], k["x"], k["n"], k["L"], k["eps"], null, 1, 0, k["out"], null, null, 0,
                                    _lib.stream())
            assert rc != 0 and b"arp_energy_probe" in L.arp_last_error(), change
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
        k = good
        assert L.arp_energy_probe(k["m"], k["which"], k["x"], k["n"], k["L"], k["eps"], null, 1, 0, k["out"], null, null, 0,
                                  _lib.stream()) == 0
        torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).all())
    with pytest.raises(RuntimeError):
        eng.energy_probe(_np(x), _np(eps), 2, lanes=3)


# ---------------------------------------------------------------------------
# 7. the CLI
# ---------------------------------------------------------------------------
ENERGY_KEYS = ("divergence_rate", "divergent_trajectories", "energy_probe_trajectories", "energy_nonfinite",
               "energy_error_mean", "energy_error_sd", "energy_accept_prob", "energy_kinetic_share")
# what a sampling run of the parent commit writes into <method>.json besides the VI fit and the tuning runs
PLAIN_RUN_KEYS = {"ess_min", "sem_min", "mcmc_time_sec", "ess_estimator", "ess_min_batch_means", "sem_min_batch_means",
                  "batch_means_batch", "ess_constant_chains", "ess_chains", "split_rhat_max", "split_rhat_chains",
                  "rhat_max_all_chains", "diagnostics_time_sec"}
RUN_KEYS = {"CP": PLAIN_RUN_KEYS | {"acceptance_rate"},
            "i": PLAIN_RUN_KEYS | {"acceptance_rate_cp", "acceptance_rate_ncp", "num_leapfrog_steps", "initial_step_size_cp",
                                   "initial_step_size_ncp"}}


def _cli(args):
    from autoreparam_amd import flags as flags_mod
    from autoreparam_amd import main as cli
    return cli.main(args, flags=flags_mod.FlagValues())


def test_cli_energy_diagnostics(gpu, tmp_path):
    """radon MN, --method=CP and --method=i at 256 chains with --energy_diagnostics: every key present and finite, two
    kernels under `energy_by_kernel` for the interleaved sampler, the shapes of <method>_energy.npz, the analyze report;
    and the same runs without the flag, in a copy of the directory made before them: the parent's key set, no file."""
    from autoreparam_amd import analyze
    Cn, S, R = 256, 120, 5
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    common = ["--model=radon", "--dataset=MN", "--num_chains=%d" % Cn, "--seed=3", "--num_optimization_steps=400"]
    hm = ["--num_samples=%d" % S, "--num_burnin_steps=200", "--num_adaptation_steps=150"]
    for m in ("CP", "NCP"):
        _cli(common + ["--results_dir=" + on, "--inference=VI", "--method=" + m])
        _cli(common + ["--results_dir=" + on, "--inference=HMCtuning", "--method=" + m, "--num_leapfrog_steps=4"] + hm)
    shutil.copytree(on, off)
    for m in ("CP", "i"):
        _cli(common + ["--results_dir=" + on, "--inference=HMC", "--method=" + m, "--energy_diagnostics",
                       "--energy_probe_steps=%d" % R] + hm)
        _cli(common + ["--results_dir=" + off, "--inference=HMC", "--method=" + m] + hm)
    sp = helpers.spec("radon_MN")
    for m, kernels in (("CP", 1), ("i", 2)):
        r = json.load(open(os.path.join(on, m + "_tied.json")))
        plain = json.load(open(os.path.join(off, m + "_tied.json")))
        fit = {"elbo", "variational_fit_time_secs", "actual_num_variational_steps", "estimated_elbo_std", "learning_rate",
               "initial_step_size", "learned_reparam", "learned_variational_params", "tuning_runs"}
        assert set(plain) - fit == RUN_KEYS[m], sorted(set(plain) ^ (RUN_KEYS[m] | fit))
        extra = set(ENERGY_KEYS) | {"energy_time_sec"} | ({"energy_by_kernel"} if kernels == 2 else set())
        assert set(r) - set(plain) == extra and set(plain) <= set(r)
        assert not os.path.exists(os.path.join(off, m + "_tied_energy.npz"))
        for k in ENERGY_KEYS + ("energy_time_sec",):
            assert len(r[k]) == 1 and r[k][0] is not None and np.isfinite(r[k][0]), k
        rows = (R + 1) * Cn * kernels
        assert r["energy_probe_trajectories"] == [rows] and 0 <= r["divergent_trajectories"][0] <= rows
        assert 0.3 < r["energy_accept_prob"][0] <= 1.0 and r["energy_time_sec"][0] <= r["diagnostics_time_sec"][0]
        if kernels == 2:
            two = r["energy_by_kernel"][0]
            assert len(two) == 2 and all(set(d) == set(ENERGY_KEYS) for d in two)
            assert sum(d["energy_probe_trajectories"] for d in two) == rows
            assert sum(d["divergent_trajectories"] for d in two) == r["divergent_trajectories"][0]
        z = np.load(os.path.join(on, m + "_tied_energy.npz"))
        steps = z["steps"]
        assert steps[0] == -1 and steps[1] == 0 and steps[-1] == S - 1 and len(steps) == R + 1
        assert z["energy_error"].shape == (R + 1, Cn) and z["energy_error"].dtype == np.float32
        assert ("energy_error_1" in z.files) == (kernels == 2)
        nd = min(r["divergent_trajectories"][0], 1024)
        assert z["divergent_chain"].shape == (nd,) and z["divergent_step"].shape == (nd,)
        for name, shape in zip(sp.part_names, sp.part_shapes):
            assert z["divergent_where/" + name].shape == (nd,) + tuple(shape)
        finite = np.isfinite(z["energy_error"])
        assert finite.sum() >= z["energy_error"].size - r["energy_nonfinite"][0]
    lines = analyze.report_energy(analyze.load(str(tmp_path), "on"), str(tmp_path), "on")
    assert len([l for l in lines if "trajectories divergent" in l and not l.startswith(" ")]) == 2
    assert analyze.report_energy(analyze.load(str(tmp_path), "off"), str(tmp_path), "off") == []
