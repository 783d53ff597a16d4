"""GPU: german_credit_gammascale (German credit with Gamma-prior scales; arp_model_set_option "german_prior") against
the float64 restatement in tests/gammascale_ref.py: density and gradient on every lane count and both matrix-core
likelihoods, the converters, every-step HMC trajectories, the posterior against a long CPU run
(tests/golden/german_gammascale_posterior.npz), the VI fit and the CLI flow."""
import json
import os

import numpy as np
import pytest
import torch

import gammascale_ref
import helpers

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "german_gammascale_posterior.npz")


@pytest.fixture(scope="module")
def sp():
    from autoreparam_amd import models
    return models._spec_german_gammascale()


@pytest.fixture(scope="module")
def ref(sp):
    return gammascale_ref.GermanRef(sp.raw["X"], sp.raw["y"])


@pytest.fixture(scope="module")
def eng(gpu, sp):
    from autoreparam_amd import engine
    return engine.Engine(sp, gpu)


def _tol(g):   # test_gpu_density.py: test_logp_grad_matches_oracle
    return 3e-5 * max(1.0, float(np.abs(g).max()))


def _check_density(eng, ref, a, b, x, lanes, what):
    lp_r, g_r = ref.logp_grad(x, a, b)
    lp_r = lp_r + ref.logp_const(b)
    lp, g = eng.logp_grad(x, which=0, lanes=lanes)
    lp, g = lp.cpu().numpy() + eng.logp_const(0), g.cpu().numpy()
    assert np.abs(lp - lp_r).max() <= 2e-6 * max(1.0, np.abs(lp_r).max()) + 1e-3, what
    assert np.abs(g - g_r).max() <= _tol(g_r), (what, np.abs(g - g_r).max())


@pytest.mark.parametrize("math", ["f32", "bf16x3"])
@pytest.mark.parametrize("kind", ["CP", "NCP", "VIP"])
def test_logp_grad_matches_restatement(eng, sp, ref, kind, math):
    eng.set_option("german_math", math)
    a, b = helpers.params(sp, kind)        # VIP: a and b both random
    eng.set_param(0, (a, b))
    assert abs(eng.logp_const(0) - ref.logp_const(b)) < 1e-9 * abs(ref.logp_const(b))
    for n in (1, 7, 130):
        x = helpers.states(sp, n, seed=n)
        for lanes in (4, 8, 16):
            _check_density(eng, ref, a, b, x, lanes, (kind, math, n, lanes))
    # a is inert: another a, bit for bit the same density
    x = helpers.states(sp, 33, seed=5)
    lp0, g0 = eng.logp_grad(x, lanes=4)
    eng.set_param(0, (np.random.RandomState(7).rand(sp.D).astype(np.float32), b))
    lp1, g1 = eng.logp_grad(x, lanes=4)
    assert torch.equal(lp0, lp1) and torch.equal(g0, g1)
    eng.set_option("german_math", "auto")


def test_prior_option_switches_one_handle(gpu, sp, ref):
    from autoreparam_amd import engine
    ln = engine.Engine(helpers.spec("german"), gpu)       # the log-normal model's spec: no option applied
    a, b = helpers.params(sp, "VIP", seed=2)
    ln.set_param(0, (a, b))
    x = helpers.states(sp, 70, seed=3)
    for lanes in (4, 8, 16):
        lp0, g0 = ln.logp_grad(x, lanes=lanes)
        ln.set_option("german_prior", "gamma")
        _check_density(ln, ref, a, b, x, lanes, ("switched", lanes))
        lp1, g1 = ln.logp_grad(x, lanes=lanes)
        assert not torch.equal(g0, g1)
        ln.set_option("german_prior", "lognormal")
        lp2, g2 = ln.logp_grad(x, lanes=lanes)
        assert torch.equal(lp0, lp2) and torch.equal(g0, g2)
    with pytest.raises(RuntimeError):
        ln.set_option("german_prior", "cauchy")
    with pytest.raises(RuntimeError):
        engine.Engine(helpers.spec("radon_MN"), gpu).set_option("german_prior", "gamma")


@pytest.mark.parametrize("kind", ["NCP", "VIP"])
def test_converters_match_restatement(eng, sp, ref, kind):
    a, b = helpers.params(sp, kind, seed=1)
    eng.set_param(0, (a, b))
    q = helpers.states(sp, 257, seed=4)
    xc = eng.transform(q, 0, to_centered=True).cpu().numpy()
    np.testing.assert_allclose(xc, ref.to_centered(q, a, b), rtol=2e-5, atol=2e-5)
    qn = eng.transform(xc, 0, to_centered=False).cpu().numpy()
    np.testing.assert_allclose(qn, ref.from_centered(xc, a, b), rtol=2e-5, atol=2e-5)
    np.testing.assert_array_equal(xc[:, 1:63], q[:, 1:63])          # bls maps to itself


def _eps0(ref, a, b, x, frac):
    """frac / sqrt(|diag Hessian|) at x from finite differences of the restated gradient (test_gpu_hmc.py: _eps0)"""
    x0 = x[:1].astype(np.float64)
    h = 1e-4
    diag = -(ref.logp_grad(x0 + h * np.eye(ref.D), a, b)[1].diagonal() - ref.logp_grad(x0, a, b)[1][0]) / h
    return (frac / np.sqrt(np.abs(diag) + 1.0)).astype(np.float32)


@pytest.mark.parametrize("math", ["f32", "bf16x3"])
@pytest.mark.parametrize("kind", ["NCP", "CP"])
def test_trajectories_every_step(oracle_lib, eng, sp, ref, gpu, kind, math):
    """plain fixed-step HMC at 4 lanes, every transition recorded, every chain held to helpers.explain_divergence
    against the restatement on the same random streams (the way parity.hmc_every_step holds the oracle)"""
    from autoreparam_amd import engine
    eng.set_option("german_math", math)
    a, b = sp.ab_from_reparam(kind)
    eng.set_param(0, (a, b))
    Cn, n, L = 48, 12, 4
    q0 = helpers.states(sp, Cn, seed=2, scale=0.1)
    eps0 = _eps0(ref, a, b, q0, 0.05)
    kw = dict(seed=9, chain_offset=1000, lanes=4)
    st = engine.ChainState(torch.as_tensor(q0, device=gpu))
    xs = torch.zeros(n, Cn, sp.D, device=gpu); xa = torch.zeros(n, Cn, dtype=torch.uint8, device=gpu)
    eng.hmc_run(st, eps0, L, n, n_burnin=0, thin=1, trace=xs, trace_accept=xa, trace_centered=False, **kw)
    r = ref.hmc(oracle_lib, q0, a, b, eps0, L, n, **kw)
    eng.set_option("german_math", "auto")
    acc = xa.cpu().numpy()
    scale = np.abs(r["q"]).max() + 1.0
    clean, first = helpers.explain_divergence(xs.cpu().numpy(), r["x"], acc[:, None], r["acc"][:, None],
                                              r["margin"][:, None], r["escale"][:, None], 1e-4 * scale,
                                              what="gammascale %s %s" % (kind, math))
    assert clean.mean() > 0.9
    assert 0.3 < r["acc"].mean() <= 1.0


def test_posterior_moments_against_long_cpu_run(eng, sp, gpu):
    """NCP at L = 8 from the fixture's mode, dual-averaging adaptation (test_gpu_hmc.py:
    test_posterior_moments_against_long_cpu_run): centred moments against the float64 run.  (CP does not mix in a run of
    this length: the Gamma(1/2, 1/2) scales of weakly identified features reach far into their left tail, a funnel for
    centred beta -- the fixture generator's CP run sits 70 Monte-Carlo errors off on overall_log_scale.)"""
    from autoreparam_amd import engine, _lib
    gold = np.load(GOLD)
    mean_g, sd_g, mcse_g = gold["mean"], gold["sd"], gold["mcse"]
    sc, mode = gold["NCP/step_scale"], gold["NCP/mode"]
    Cn, L, burn, S = 768, 8, 1500, 600
    eng.set_param(0, "NCP")
    q0 = (mode + 0.5 * sc * np.random.RandomState(1).randn(Cn, sp.D)).astype(np.float32)
    st = engine.ChainState(torch.as_tensor(q0, device=gpu))
    tr = torch.zeros(S, Cn, sp.D, device=gpu)
    eng.hmc_run(st, (0.5 * sc).astype(np.float32), L, 1 + burn + 2 * (S - 1), seed=77, adapt_kind=_lib.ADAPT_DUAL,
                n_adapt=burn - 200, n_burnin=burn, thin=2, trace=tr, trace_centered=True)
    acc = st.accept_count.double().mean().item() / st.step
    assert 0.55 < acc < 0.95, acc
    cm = tr.double().mean(dim=0).cpu().numpy()
    mean = cm.mean(axis=0)
    mcse = cm.std(axis=0, ddof=1) / np.sqrt(Cn)
    sd = tr.double().reshape(-1, sp.D).std(dim=0).cpu().numpy()
    z = np.abs(mean - mean_g) / (np.sqrt(mcse ** 2 + mcse_g ** 2) + 0.01 * sd_g)
    assert z.max() < 5.0, (int(z.argmax()), z.max())
    # marginal sds from finite samples of both runs, looser than the log-normal model's 10 %: the Gamma scales are heavy
    # tailed on the left and mix slowly (measured: at most 22 %, on beta[0], 12 % on the log scales)
    r = np.abs(sd / sd_g - 1)
    assert r.max() < 0.30, (int(r.argmax()), r.max())


def _vi_flags(steps, lrs):
    from autoreparam_amd import flags as flags_mod
    f = flags_mod.FlagValues()
    f.num_optimization_steps, f.learning_rates = steps, lrs
    return f


@pytest.mark.parametrize("tied", [True, False])
def test_cvip_fit(gpu, sp, ref, tied):
    """cVIP: a finite ELBO, the learned_reparam keys of the reference's learnable parametrisation (no beta_log_scales_*),
    a never moving (its gradient is identically 0), and the reported ELBO at the fit's (loc, scale) against a float64
    Monte-Carlo estimate of the restatement"""
    from autoreparam_amd import graphs, inference, models
    cfg = models.get_model_by_name("german_credit_gammascale")
    f = _vi_flags(400, [0.02, 0.05])
    _, _, elbo, vp, init = graphs.make_cvip_graph(cfg, tied_pparams=tied, flags=f)
    e, tl, lr, _, lvp, rp = inference.find_best_learning_rate(elbo, vp, None, init, flags=f)
    assert np.isfinite(e) and len(tl) == 400
    want = {"overall_log_scale_a", "beta_a"} | (set() if tied else {"overall_log_scale_b", "beta_b"})
    assert set(rp) == want
    assert rp["beta_a"].shape == (62,) and np.shape(rp["overall_log_scale_a"]) == ()
    assert (rp["beta_a"] == 0.5).all() and rp["overall_log_scale_a"] == 0.5
    if not tied:
        assert np.abs(rp["beta_b"] - 0.5).max() > 0.01              # b is what moves
    a, b = cfg.model.ab_from_reparam(rp)                 # tied: b = 1, as the target of the fit saw it
    loc = np.concatenate([np.ravel(lvp[n + "_loc"]) for n in sp.part_names])
    scale = np.concatenate([np.ravel(lvp[n + "_scale"]) for n in sp.part_names]).astype(np.float64)
    M = 20000
    z = loc + scale * np.random.RandomState(3).randn(M, sp.D)
    lp = np.concatenate([ref.logp_grad(z[i:i + 2000], a, b)[0] for i in range(0, M, 2000)]) + ref.logp_const(b)
    ent = np.sum(np.log(scale)) + sp.D * (0.5 + 0.5 * np.log(2 * np.pi))
    est, se_r = lp.mean() + ent, lp.std() / np.sqrt(M)
    se_k = np.std(tl[-32:]) / np.sqrt(32)
    assert abs(e - est) < 5 * np.sqrt(se_r ** 2 + se_k ** 2) + 0.05, (e, est, se_r, se_k)


def _run(args, out=None):
    from autoreparam_amd import flags as flags_mod
    from autoreparam_amd import main as cli
    return cli.main(args, flags=flags_mod.FlagValues(), out=out)


def test_cli_flow(gpu, tmp_path):
    """test_gpu_cli.py's flow on german_credit_gammascale at small size: VI cVIP -> HMCtuning -> HMC, CP and NCP, the
    interleaved run, dVIP; and one 16 384-chain dVIP HMC run (config 3's shape)"""
    d = str(tmp_path)
    base = ["--model=german_credit_gammascale", "--results_dir=" + d, "--num_chains=256", "--num_optimization_steps=300",
            "--learning_rates=0.02,0.05", "--seed=2"]
    hm = ["--num_samples=200", "--num_burnin_steps=200", "--num_adaptation_steps=150"]
    _run(base + ["--inference=VI", "--method=cVIP"])
    r = json.load(open(os.path.join(d, "cVIP_eig_tied.json")))
    assert set(r["learned_reparam"]) == {"overall_log_scale_a", "beta_a"} and len(r["learned_reparam"]["beta_a"]) == 62
    assert np.isfinite(r["elbo"])
    assert set(r["learned_variational_params"]) == {p + s for p in ("overall_log_scale", "beta_log_scales", "beta")
                                                    for s in ("_loc", "_scale")}
    _run(base + ["--inference=HMCtuning", "--method=cVIP", "--num_leapfrog_steps=4"] + hm)
    _run(base + ["--inference=HMC", "--method=cVIP", "--num_chains_to_save=2"] + hm)
    r = json.load(open(os.path.join(d, "cVIP_eig_tied.json")))
    assert r["tuning_runs"][0]["acceptance_rate"] > 30
    for k in ("ess_min", "sem_min", "acceptance_rate", "mcmc_time_sec"):
        assert isinstance(r[k], list) and len(r[k]) == 1
    assert np.load(os.path.join(d, "cVIP_eig_tied_ess.npz"))["beta_log_scales"].shape[-1] == 62
    assert np.load(os.path.join(d, "cVIP_eig_tied_traces.npz"))["beta"].shape == (200, 2, 62)
    for m in ("CP", "NCP"):
        _run(base + ["--inference=VI", "--method=" + m])
        _run(base + ["--inference=HMCtuning", "--method=" + m, "--num_leapfrog_steps=4"] + hm)
        assert json.load(open(os.path.join(d, "%s_tied.json" % m)))["tuning_runs"][0]["ess_min"] > 0
    _run(base + ["--inference=HMC", "--method=i"] + hm)
    r = json.load(open(os.path.join(d, "i_tied.json")))
    for k in ("initial_step_size_ncp", "initial_step_size_cp", "num_leapfrog_steps", "ess_min", "sem_min"):
        assert k in r
    _run(base + ["--inference=VI", "--method=dVIP"])
    r = json.load(open(os.path.join(d, "dVIP_eig_tied.json")))
    assert set(r["learned_reparam"]) == {"overall_log_scale_a", "beta_a"}
    big = [a for a in base if not a.startswith("--num_chains")] + ["--num_chains=16384"]
    res = _run(big + ["--inference=HMC", "--method=dVIP", "--num_leapfrog_steps=4", "--num_samples=200",
                      "--num_burnin_steps=300", "--num_adaptation_steps=200", "--num_chains_to_save=2"])
    ess_min, sem_min, acc, _ = res
    assert np.isfinite(ess_min) and ess_min > 0 and 40 < acc <= 100
    r = json.load(open(os.path.join(d, "dVIP_eig_tied.json")))
    assert len(r["ess_min"]) == 1 and np.isfinite(r["ess_min"][0])
