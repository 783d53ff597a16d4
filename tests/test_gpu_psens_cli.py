"""GPU: --sensitivity_diagnostics end to end, on the pipeline of tests/test_gpu_loopred_cli.py (NCP, 256 chains, 200
samples): 8 schools and German credit at --loo_draws=8192, each run with --predictive_diagnostics alone and with
--sensitivity_diagnostics added, from one copied VI / tuning directory.  The flag adds exactly PSENS_KEYS and
<method>_psens.npz and changes nothing else: every other key (timing apart) and every array of _rhat.npz, _ess.npz and
_loo.npz is the unflagged run's.  The file's arrays are diagnostics.psens_summary of the kernels' sums on the recorded
trace, bit for bit; they agree with tests/psens_ref.py on the device's own lw to 1e-6 relative on the sensitivities, and
the JSON figures are psens_ref's summary.  A report forced into several observation tiles gives the one-tile arrays bit
for bit; analyze --psens prints the line for the flagged run only; neals_funnel with the flag raises before anything runs."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import psens_ref as pr
from test_gpu_loopred_cli import HM, _cli

pytestmark = pytest.mark.gpu

PER_PART = ("prior", "likelihood", "mean_shift_prior", "mean_shift_likelihood", "sd_ratio_prior", "sd_ratio_likelihood")


def pipeline(root, model, extra):
    """VI and one tuning run of `model` under root/on, copied to root/off; then the sampling run with
    --predictive_diagnostics under off and with --sensitivity_diagnostics added under on.  Returns (on, off, the flagged
    run's `out`)."""
    on, off, out = os.path.join(root, "on"), os.path.join(root, "off"), {}
    common = ["--model=" + model, "--num_chains=256", "--seed=3", "--num_optimization_steps=400", "--method=NCP"]
    _cli(common + ["--results_dir=" + on, "--inference=VI"])
    _cli(common + ["--results_dir=" + on, "--inference=HMCtuning", "--num_leapfrog_steps=4"] + HM)
    shutil.copytree(on, off)
    _cli(common + ["--results_dir=" + off, "--inference=HMC", "--predictive_diagnostics"] + extra + HM)
    _cli(common + ["--results_dir=" + on, "--inference=HMC", "--predictive_diagnostics", "--sensitivity_diagnostics"] + extra + HM,
         out=out)
    return on, off, out


def flat(z, key, spec):
    return np.concatenate([np.asarray(z["%s/%s" % (key, name)]).reshape(-1) for name in spec.part_names])


def check_run(root, capsys, model, extra, spec, draws, steps):
    from autoreparam_amd import analyze, diagnostics, engine, main as cli
    capsys.readouterr()
    on, off, out = pipeline(root, model, extra)
    text = capsys.readouterr().out
    assert text.count("power-scaling sensitivity over") == 1
    path = lambda d, suffix: os.path.join(d, "NCP_tied" + suffix)
    r, plain = json.load(open(path(on, ".json"))), json.load(open(path(off, ".json")))
    # the flag adds its keys and its file, and changes nothing else
    assert set(r) - set(plain) == set(cli.PSENS_KEYS) and set(plain) <= set(r)
    for key in plain:
        if "time" not in key:
            assert plain[key] == r[key], key
    for suffix in ("_loo.npz", "_rhat.npz", "_ess.npz"):
        a, b = np.load(path(on, suffix)), np.load(path(off, suffix))
        assert sorted(a.files) == sorted(b.files), suffix
        assert all(np.array_equal(a[name], b[name], equal_nan=a[name].dtype.kind == "f") for name in a.files), suffix
    assert os.path.exists(path(on, "_psens.npz")) and not os.path.exists(path(off, "_psens.npz"))
    assert all(len(r[key]) == 1 for key in cli.PSENS_KEYS)
    assert r["psens_draws"] == [draws] and r["psens_draws_left_out"] == [0] and r["psens_chains"] == [256]
    assert r["psens_steps"] == [steps] and r["psens_elements_left_out"] == [0]
    assert 0 < r["psens_time_sec"][0] <= r["diagnostics_time_sec"][0]
    assert r["psens_pareto_k_threshold"][0] == pytest.approx(diagnostics.pareto_k_threshold(draws))
    z = np.load(path(on, "_psens.npz"))
    D, names = spec.D, cli.element_names(spec)
    assert sorted(z.files) == sorted(["elements", "y", "model", "pareto_k", "log_prior", "log_likelihood", "left_out"]
                                     + ["%s/%s" % (key, name) for key in PER_PART for name in spec.part_names])
    assert str(z["model"]) == model and list(z["elements"]) == names and z["pareto_k"].shape == (4,)
    assert z["log_prior"].shape == z["log_likelihood"].shape == z["left_out"].shape == (draws,) and not z["left_out"].any()
    # the kernels' sums on the recorded trace ...
    trace = out["kernel_results"].trace
    dev = trace.device
    picked = cli.loo_steps(int(trace.shape[0]), 256, draws if extra else 65536)
    assert len(picked) == steps and len(picked) * 256 == draws
    x = trace[torch.as_tensor(picked, device=dev), :256].contiguous()
    table = diagnostics.upload_table(spec.observation_table(), D, dev)
    ll, mask, count = diagnostics.pointwise_loglik(x, table)
    log_lik = diagnostics.loglik_total(ll, torch.zeros(draws, dtype=torch.float64, device=dev))
    eng = engine.Engine(spec, dev)
    eng.set_param(0, "CP")
    log_prior = eng.logp_grad(x.reshape(draws, D), which=0)[0].to(torch.float64) - log_lik
    assert int(count.item()) == 0 and bool(torch.isfinite(log_prior).all())
    out8, lw = diagnostics.powerscale_lw(log_prior, log_lik, mask)
    order, values = diagnostics.element_order(x)
    mean = flat(np.load(path(on, "_rhat.npz")), "posterior_mean", spec)
    shift = np.nan_to_num(mean).astype(np.float32)
    sums = diagnostics.cjs_sums(values, order, lw, torch.as_tensor(shift, device=dev)).cpu().numpy()
    assert np.array_equal(z["log_prior"], log_prior.cpu().numpy()) and np.array_equal(z["log_likelihood"], log_lik.cpu().numpy())
    assert np.array_equal(z["pareto_k"], out8.cpu().numpy()[:, 1]) and np.all(sums[:, :, 0] == draws)
    # ... are what the file's arrays were made of, through the one host definition, bit for bit
    s = diagnostics.psens_summary(sums)
    for key in PER_PART:
        assert np.array_equal(flat(z, key, spec), getattr(s, key), equal_nan=True), key
    # ... and agree with the float64 definition on the device's own lw
    want_sums, _ = pr.cjs_sums(values.cpu().numpy(), order.cpu().numpy().view(np.uint32), lw.cpu().numpy(), shift)
    want = pr.summary(want_sums)
    assert np.all(np.isfinite(s.prior)) and np.all(np.isfinite(s.likelihood))
    assert np.allclose(s.prior, want["prior"], rtol=1e-6, atol=0) and np.allclose(s.likelihood, want["likelihood"], rtol=1e-6, atol=0)
    # the JSON figures are the reference's summary of the device's sums
    mine = pr.summary(sums)
    for key, name in (("psens_prior_max", "prior"), ("psens_likelihood_max", "likelihood")):
        at = int(np.nanargmax(mine[name]))
        assert r[key][0] == pytest.approx(float(mine[name][at]), rel=1e-12) and r[key + "_element"][0] == names[at], key
    assert r["psens_conflict_elements"][0] == [names[i] for i in mine["conflict"]]
    assert r["psens_weak_likelihood_elements"][0] == [names[i] for i in mine["weak_likelihood"]]
    assert r["psens_pareto_k_max"][0] == pytest.approx(float(np.max(z["pareto_k"][np.isfinite(z["pareto_k"])])), rel=1e-12)
    # analyze --psens: the line for the flagged run, not for the other
    base = os.path.dirname(on)
    analyze.main(["--results_dir=" + base, "--model=on", "--psens"])
    shown = capsys.readouterr().out
    assert shown.count("power-scaling sensitivity:") == 1 and "NCP_tied: power-scaling sensitivity" in shown
    assert "prior max {:.4g} ({})".format(r["psens_prior_max"][0], r["psens_prior_max_element"][0]) in shown
    analyze.main(["--results_dir=" + base, "--model=off", "--psens"])
    assert "power-scaling sensitivity" not in capsys.readouterr().out
    return r, s


def test_eight_schools(gpu, tmp_path, capsys):
    from autoreparam_amd import models
    r, s = check_run(str(tmp_path), capsys, "8schools", [], models._spec_eight_schools(), 51200, 200)
    assert r["psens_prior_max"][0] > 0 and r["psens_likelihood_max"][0] > 0


def test_german_credit(gpu, tmp_path, capsys):
    from autoreparam_amd import models
    r, s = check_run(str(tmp_path), capsys, "german_credit_lognormalcentered", ["--loo_draws=8192"], models._spec_german(), 8192, 32)
    assert r["psens_prior_max"][0] > 0 and r["psens_likelihood_max"][0] > 0


def test_several_tiles_give_the_arrays_of_one(gpu, monkeypatch):
    """German credit's table on a synthetic trace, R = 256: a budget of 100 observations per tile against one tile -- the
    likelihood total is added observation by observation, so both reports' arrays are equal bit for bit."""
    from autoreparam_amd import main as cli, models
    sp = models._spec_german()
    trace = torch.as_tensor((0.1 * np.random.RandomState(0).randn(4, 64, sp.D)).astype(np.float32), device=gpu)
    flags = type("F", (), {"loo_draws": 65536, "sensitivity_diagnostics": True})()
    whole, arrays = cli._psens_report(trace, 64, sp, flags, None)
    monkeypatch.setattr(cli, "LOO_CHUNK_BYTES", 100 * 4 * 256)
    assert cli.loo_tile_rows(1000, 256) == 100
    tiled, arrays_t = cli._psens_report(trace, 64, sp, flags, None)
    assert tuple(whole) == cli.PSENS_KEYS and sorted(arrays) == sorted(arrays_t) and whole["psens_draws"] == 256
    for name in arrays:
        a, b = np.asarray(arrays[name]), np.asarray(arrays_t[name])
        assert a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b)), name
    timeless = lambda keys: {k: v for k, v in keys.items() if "time" not in k}
    assert timeless(whole) == timeless(tiled)


def test_neals_funnel_is_refused_before_the_run(gpu, tmp_path):
    with pytest.raises(ValueError, match="neals_funnel has no observations"):
        _cli(["--model=neals_funnel", "--num_chains=64", "--method=CP", "--inference=HMC", "--sensitivity_diagnostics",
              "--results_dir=" + str(tmp_path)] + HM)
    assert os.listdir(str(tmp_path)) == []
