"""GPU: --sensitivity_prior_parts end to end, on the pipeline and helpers of tests/test_gpu_psens_cli.py (NCP, 256 chains,
200 samples, one copied VI / tuning directory): 8 schools with the priors of mu and log_tau against the run with
--sensitivity_diagnostics alone -- the flag adds exactly PSENS_SITE_KEYS and <method>_psens_sites.npz and changes nothing
else; the file's arrays are diagnostics.psens_summary of the wrappers' results on the recorded trace, bit for bit, and
agree with tests/psens_ref.py on the device's own lw to 1e-6 relative; German credit with Gamma scales at
--loo_draws=8192 (the log-Gamma form and the two-term scale); a report forced into several blocks of draws gives the
one-block arrays bit for bit; a refused name raises before the run."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import psens_ref as pr
from test_gpu_loopred_cli import HM, _cli
from test_gpu_psens_cli import flat

pytestmark = pytest.mark.gpu

PER_PART = ("prior", "mean_shift_prior", "sd_ratio_prior")


def pipeline(root, model, extra, parts, with_plain):
    """VI and one tuning run of `model` under root/sites, copied to root/plain; the sampling run with
    --sensitivity_diagnostics under plain (where asked) and with --sensitivity_prior_parts added under sites.  Returns
    (sites, plain, the flagged run's `out`)."""
    sites, plain, out = os.path.join(root, "sites"), os.path.join(root, "plain"), {}
    common = ["--model=" + model, "--num_chains=256", "--seed=3", "--num_optimization_steps=400", "--method=NCP"]
    _cli(common + ["--results_dir=" + sites, "--inference=VI"])
    _cli(common + ["--results_dir=" + sites, "--inference=HMCtuning", "--num_leapfrog_steps=4"] + HM)
    run = ["--inference=HMC", "--predictive_diagnostics", "--sensitivity_diagnostics"] + extra + HM
    if with_plain:
        shutil.copytree(sites, plain)
        _cli(common + ["--results_dir=" + plain] + run)
    _cli(common + ["--results_dir=" + sites, "--sensitivity_prior_parts=" + parts] + run, out=out)
    return sites, plain, out


def recompute(cli, diagnostics, engine, spec, out, draws, loo_draws, chosen, mean):
    """The second report from the wrappers alone, on the recorded trace: (sel, rest, left, gap, out8, lw, sums, values, order)"""
    trace = out["kernel_results"].trace
    dev, D = trace.device, spec.D
    picked = cli.loo_steps(int(trace.shape[0]), 256, loo_draws)
    assert len(picked) * 256 == draws
    x = trace[torch.as_tensor(picked, device=dev), :256].contiguous()
    table = diagnostics.upload_table(spec.observation_table(), D, dev)
    ll, mask, count = diagnostics.pointwise_loglik(x, table)
    log_lik = diagnostics.loglik_total(ll, torch.zeros(draws, dtype=torch.float64, device=dev))
    eng = engine.Engine(spec, dev)
    eng.set_param(0, "CP")
    log_prior = eng.logp_grad(x.reshape(draws, D), which=0)[0].to(torch.float64) - log_lik
    const = float(eng.logp_const(0))
    up = diagnostics.upload_site_table(spec.site_table(), D, dev)
    by_part, _, site_mask, site_count = diagnostics.site_logprior(x, up)
    assert int(count.item()) == 0 and int(site_count.item()) == 0 and torch.equal(mask, site_mask)
    sel, rest = (torch.zeros(draws, dtype=torch.float64, device=dev) for _ in range(2))
    for p, name in enumerate(spec.part_names):
        (sel if name in chosen else rest).add_(by_part[:, p])
    left = (mask != 0) | ~torch.isfinite(log_prior) | ~torch.isfinite(sel)
    gap = float(((sel + rest) - (log_prior + const)).abs()[~left].max().item())
    out8, lw = diagnostics.powerscale_lw(sel, log_lik, left)
    order, values = diagnostics.element_order(x)
    shift = np.nan_to_num(mean).astype(np.float32)
    sums = diagnostics.cjs_sums(values, order, lw, torch.as_tensor(shift, device=dev)).cpu().numpy()
    return sel, rest, left, gap, out8, lw, sums, values, order, shift


def check_file(path, spec, chosen, r, draws, loo_draws, out, definition):
    """<method>_psens_sites.npz and the JSON keys against the wrappers, psens_ref's summary and, where `definition` is set,
    the float64 definition"""
    from autoreparam_amd import diagnostics, engine, main as cli
    z = np.load(path("_psens_sites.npz"))
    names = cli.element_names(spec)
    assert sorted(z.files) == sorted(["parts", "selected", "log_prior_selected", "log_prior_rest", "left_out", "pareto_k"]
                                     + ["%s/%s" % (key, name) for key in PER_PART for name in spec.part_names])
    assert list(z["parts"]) == spec.part_names and z["selected"].dtype == bool
    assert [n for n, s in zip(spec.part_names, z["selected"]) if s] == [n for n in spec.part_names if n in chosen]
    assert z["pareto_k"].shape == (2,) and z["left_out"].shape == (draws,) and not z["left_out"].any()
    mean = flat(np.load(path("_rhat.npz")), "posterior_mean", spec)
    sel, rest, left, gap, out8, lw, sums, values, order, shift = recompute(cli, diagnostics, engine, spec, out, draws, loo_draws,
                                                                          chosen, mean)
    assert not bool(left.any())
    assert np.array_equal(z["log_prior_selected"], sel.cpu().numpy()) and np.array_equal(z["log_prior_rest"], rest.cpu().numpy())
    assert np.array_equal(z["pareto_k"], out8.cpu().numpy()[:2, 1]) and np.all(sums[:, :, 0] == draws)
    s = diagnostics.psens_summary(sums)
    for key in PER_PART:
        assert np.array_equal(flat(z, key, spec), getattr(s, key), equal_nan=True), key
    assert np.all(np.isfinite(s.prior))
    # the float64 definition on the device's own lw
    want_sums, _ = pr.cjs_sums(values.cpu().numpy(), order.cpu().numpy().view(np.uint32), lw.cpu().numpy(), shift)
    want = pr.summary(want_sums)["prior"]
    print("%s: sensitivities %.3g ... %.3g, largest relative deviation from the float64 definition %.3g" % (
        spec.name, s.prior.min(), s.prior.max(), float(np.max(np.abs(s.prior - want) / np.abs(want)))))
    if definition:
        assert np.allclose(s.prior, want, rtol=1e-6, atol=0)
    # the JSON figures are the reference's summary of the device's sums
    mine = pr.summary(sums)
    at = int(np.nanargmax(mine["prior"]))
    assert r["psens_sites"][0] == [n for n in spec.part_names if n in chosen] and r["psens_sites_draws_left_out"][0] == 0
    assert r["psens_sites_prior_max"][0] == pytest.approx(float(mine["prior"][at]), rel=1e-12)
    assert r["psens_sites_prior_max_element"][0] == names[at]
    assert r["psens_sites_conflict_elements"][0] == [names[i] for i in mine["conflict"]]
    assert r["psens_sites_weak_likelihood_elements"][0] == [names[i] for i in mine["weak_likelihood"]]
    assert r["psens_sites_pareto_k_max"][0] == pytest.approx(float(np.max(z["pareto_k"][np.isfinite(z["pareto_k"])])), rel=1e-12)
    assert np.isfinite(gap) and r["psens_sites_joint_gap_max"][0] == gap
    print("%s: psens_sites_joint_gap_max %.3g, psens_sites_time_sec %.3f, psens_time_sec %.3f" % (
        spec.name, gap, r["psens_sites_time_sec"][0], r["psens_time_sec"][0]))
    assert 0 < r["psens_sites_time_sec"][0] <= r["psens_time_sec"][0] <= r["diagnostics_time_sec"][0]
    return z


def test_eight_schools(gpu, tmp_path, capsys):
    from autoreparam_amd import analyze, main as cli, models
    spec = models._spec_eight_schools()
    capsys.readouterr()
    sites, plain, out = pipeline(str(tmp_path), "8schools", [], "mu,log_tau", True)
    text = capsys.readouterr().out
    assert text.count("power-scaling sensitivity over") == 2 and text.count("to the priors of mu, log_tau alone") == 1
    path = lambda d, suffix: os.path.join(d, "NCP_tied" + suffix)
    r, base = json.load(open(path(sites, ".json"))), json.load(open(path(plain, ".json")))
    # the flag adds its keys and its file, and changes nothing else
    assert set(r) - set(base) == set(cli.PSENS_SITE_KEYS) and set(base) <= set(r)
    for key in base:
        if "time" not in key:
            assert base[key] == r[key], key
    for suffix in ("_psens.npz", "_loo.npz", "_rhat.npz", "_ess.npz"):
        a, b = np.load(path(sites, suffix)), np.load(path(plain, suffix))
        assert sorted(a.files) == sorted(b.files), suffix
        assert all(np.array_equal(a[name], b[name], equal_nan=a[name].dtype.kind == "f") for name in a.files), suffix
    assert os.path.exists(path(sites, "_psens_sites.npz")) and not os.path.exists(path(plain, "_psens_sites.npz"))
    assert all(len(r[key]) == 1 for key in cli.PSENS_SITE_KEYS)
    with capsys.disabled():
        check_file(lambda suffix: path(sites, suffix), spec, ("mu", "log_tau"), r, 51200, 65536, out, True)
    # analyze --psens: the second line for the flagged run, not for the other
    root = os.path.dirname(sites)
    capsys.readouterr()
    analyze.main(["--results_dir=" + root, "--model=sites", "--psens"])
    shown = capsys.readouterr().out
    assert shown.count("power-scaling sensitivity:") == 1 and shown.count("to the priors of mu, log_tau alone") == 1
    assert "prior max {:.4g} ({})".format(r["psens_sites_prior_max"][0], r["psens_sites_prior_max_element"][0]) in shown
    analyze.main(["--results_dir=" + root, "--model=plain", "--psens"])
    shown = capsys.readouterr().out
    assert shown.count("power-scaling sensitivity:") == 1 and "to the priors of" not in shown


def test_german_credit_gammascale(gpu, tmp_path, capsys):
    """The log-Gamma form and the two-term scale end to end: the top-level prior N(0, 10) of overall_log_scale alone.  The
    bitwise checks of the file against the wrappers only: the sensitivities to this prior are 1.7e-5 ... 5.1e-4, a
    hundredth of the threshold and less, and a cumulative Jensen-Shannon distance that small is a difference of nearly
    equal sums -- two float64 evaluations of it agree to 1.1e-4 relative at the worst element (measured on an MI355X;
    the figure is printed), not to the 1e-6 the 8 schools test holds (1.2e-11 there)."""
    from autoreparam_amd import models
    spec = models._spec_german_gammascale()
    sites, _, out = pipeline(str(tmp_path), "german_credit_gammascale", ["--loo_draws=8192"], "overall_log_scale", False)
    path = lambda suffix: os.path.join(sites, "NCP_tied" + suffix)
    r = json.load(open(path(".json")))
    with capsys.disabled():
        z = check_file(path, spec, ("overall_log_scale",), r, 8192, 8192, out, False)
    assert list(z["selected"]) == [True, False, False] and r["psens_sites_prior_max"][0] > 0


def test_several_blocks_give_the_arrays_of_one(gpu, monkeypatch):
    """German credit with Gamma scales on a synthetic trace, 4 steps of 64 chains: a budget of two steps' [rows, P] float64
    per block (and three observations per likelihood tile) against one block -- the parts' columns are added row by
    row, so both reports' arrays are equal bit for bit."""
    from autoreparam_amd import main as cli, models
    sp = models._spec_german_gammascale()
    trace = torch.as_tensor((0.1 * np.random.RandomState(0).randn(4, 64, sp.D)).astype(np.float32), device=gpu)
    flags = type("F", (), {"loo_draws": 65536, "sensitivity_diagnostics": True, "sensitivity_prior_parts": "beta,overall_log_scale"})()
    side, side_t = {}, {}
    whole, arrays = cli._psens_report(trace, 64, sp, flags, None, side)
    monkeypatch.setattr(cli, "LOO_CHUNK_BYTES", 2 * 8 * 3 * 64)
    calls = []
    from autoreparam_amd import diagnostics
    real = diagnostics.site_logprior
    monkeypatch.setattr(diagnostics, "site_logprior", lambda *a, **k: (calls.append(int(a[0].shape[0])), real(*a, **k))[1])
    tiled, arrays_t = cli._psens_report(trace, 64, sp, flags, None, side_t)
    assert calls == [2, 2]
    assert tuple(whole) == cli.PSENS_KEYS[:-1] + cli.PSENS_SITE_KEYS + cli.PSENS_KEYS[-1:] and whole["psens_draws"] == 256
    assert whole["psens_sites"] == ["overall_log_scale", "beta"]
    for a, b in ((arrays, arrays_t), (side[cli.PSENS_SITES_ARRAYS], side_t[cli.PSENS_SITES_ARRAYS])):
        assert sorted(a) == sorted(b)
        for name in a:
            u, v = np.asarray(a[name]), np.asarray(b[name])
            assert u.shape == v.shape and (np.array_equal(u, v, equal_nan=True) if u.dtype.kind == "f" else np.array_equal(u, v)), name
    timeless = lambda keys: {k: v for k, v in keys.items() if "time" not in k}
    assert timeless(whole) == timeless(tiled)


def test_a_name_that_is_no_part_is_refused_before_the_run(gpu, tmp_path):
    with pytest.raises(ValueError, match="tau is no latent part of 8schools; its parts: mu, log_tau, theta"):
        _cli(["--model=8schools", "--num_chains=64", "--method=CP", "--inference=HMC", "--sensitivity_diagnostics",
              "--sensitivity_prior_parts=mu,tau", "--results_dir=" + str(tmp_path)] + HM)
    assert os.listdir(str(tmp_path)) == []
