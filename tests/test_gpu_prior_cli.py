"""GPU: --prior_predictive_checks end to end, on the helpers of tests/test_gpu_loo_cli.py (256 chains, 200 samples, one
copied VI / tuning directory, one process): 8 schools CP at 65 536 prior draws against the same run without the flag -- the
flag adds exactly PRIOR_KEYS and <method>_prior.npz and changes nothing else; the prior of mu ~ N(0, 5) read back from
the order statistics within five of their standard errors; analyze --prior; German credit with Gamma scales at 8 192
draws (the log-Gamma form, Bernoulli data); neals_funnel refused before the run."""
import json
import math
import os
import shutil

import numpy as np
import pytest

from test_gpu_loo_cli import HM, _cli

pytestmark = pytest.mark.gpu

Z90 = 1.6448536269514722
PER_PART = ("prior_q05", "prior_median", "prior_q95", "contraction", "z_score")
SIDE_FILES = ("_rhat.npz", "_ess.npz")


def pipeline(root, model, method, extra, with_plain):
    """VI and one tuning run of `model` under root/on, copied to root/off; the sampling run without the flag under off
    (where asked) and with --prior_predictive_checks under on.  Returns (on, off)."""
    on, off = os.path.join(root, "on"), os.path.join(root, "off")
    common = ["--model=" + model, "--num_chains=256", "--seed=3", "--num_optimization_steps=400", "--method=" + method]
    _cli(common + ["--results_dir=" + on, "--inference=VI"])
    _cli(common + ["--results_dir=" + on, "--inference=HMCtuning", "--num_leapfrog_steps=4"] + HM)
    run = ["--inference=HMC"] + extra + HM
    if with_plain:
        shutil.copytree(on, off)
        _cli(common + ["--results_dir=" + off] + run)
    _cli(common + ["--results_dir=" + on, "--prior_predictive_checks"] + run)
    return on, off


def test_eight_schools(gpu, tmp_path, capsys):
    from autoreparam_amd import analyze, main as cli, models
    spec = models._spec_eight_schools()
    R = 65536
    capsys.readouterr()
    on, off = pipeline(str(tmp_path), "8schools", "CP", ["--loo_draws=%d" % R], True)
    text = capsys.readouterr().out
    assert text.count("prior predictive checks over 8 observations, %d prior draws" % R) == 1
    assert text.count("prior to posterior over 10 elements") == 1 and "WARNING: prior" not in text
    path = lambda d, suffix: os.path.join(d, "CP_tied" + suffix)
    r, base = json.load(open(path(on, ".json"))), json.load(open(path(off, ".json")))
    # the flag adds its keys and its file, and changes nothing else
    assert set(r) - set(base) == set(cli.PRIOR_KEYS) and set(base) <= set(r)
    assert not any(key.startswith("prior_") for key in base)
    for key in base:
        if not key.endswith("_time_sec"):
            assert base[key] == r[key], key
    for suffix in SIDE_FILES:
        a, b = np.load(path(on, suffix)), np.load(path(off, suffix))
        assert sorted(a.files) == sorted(b.files), suffix
        assert all(np.array_equal(a[name], b[name], equal_nan=a[name].dtype.kind == "f") for name in a.files), suffix
    assert os.path.exists(path(on, "_prior.npz")) and not os.path.exists(path(off, "_prior.npz"))
    assert sorted(f for f in os.listdir(on) if not f.endswith("_prior.npz")) == sorted(os.listdir(off))
    # every key is there, once, and finite
    for key in cli.PRIOR_KEYS:
        assert len(r[key]) == 1 and r[key][0] is not None, key
        assert isinstance(r[key][0], str) or math.isfinite(r[key][0]), key
    assert r["prior_draws"][0] + r["prior_draws_left_out"][0] == R and r["prior_draws"][0] > 0.99 * R
    assert r["prior_observations"][0] == 8 and r["prior_elements_left_out"][0] == 0
    assert 0 < r["prior_time_sec"][0] <= r["diagnostics_time_sec"][0]
    assert all(0.0 <= r["prior_p_" + s][0] <= 1.0 for s in ("mean", "sd", "min", "max", "deviance"))
    assert r["prior_rep_mean_q05"][0] <= r["prior_rep_mean_q50"][0] <= r["prior_rep_mean_q95"][0]
    assert 0 < r["prior_rep_sd_q05"][0] <= r["prior_rep_sd_q50"][0] <= r["prior_rep_sd_q95"][0]
    assert r["prior_obs_mean"][0] == pytest.approx(float(np.mean(spec.raw["y"])), rel=1e-6)
    # the file
    z = np.load(path(on, "_prior.npz"))
    assert sorted(z.files) == sorted(["elements", "y", "model", "draw_stats", "left_out", "predictive_mean", "predictive_sd"]
                                     + ["%s/%s" % (key, name) for key in PER_PART for name in spec.part_names])
    assert list(z["elements"]) == cli.element_names(spec) and str(z["model"]) == "8schools"
    assert z["draw_stats"].shape == (R, 8) and z["left_out"].shape == (R,) and int(z["left_out"].sum()) == r["prior_draws_left_out"][0]
    assert z["y"].shape == (8,) and z["predictive_mean"].shape == (8,) and z["predictive_sd"].shape == (8,)
    for key in PER_PART:
        assert z[key + "/mu"].shape == () and z[key + "/log_tau"].shape == () and z[key + "/theta"].shape == (8,)
    # mu ~ N(0, 5): an order statistic at p has the standard error sqrt(p (1 - p) / R) / f(q) (f the density at the
    # quantile q); the 5 % and 95 % ones have the covariance p^2 / (R f^2) (p = 0.05, symmetric density), so their
    # difference has the variance (2 p (1 - p) - 2 p^2) / (R f^2)
    kept = r["prior_draws"][0]
    density = lambda v: math.exp(-0.5 * (v / 5.0) ** 2) / (5.0 * math.sqrt(2.0 * math.pi))
    se_median = math.sqrt(0.25 / kept) / density(0.0)
    p = 0.05
    se_scale = math.sqrt((2 * p * (1 - p) - 2 * p * p) / kept) / density(5.0 * Z90) / (2.0 * Z90)
    median = float(z["prior_median/mu"])
    scale = (float(z["prior_q95/mu"]) - float(z["prior_q05/mu"])) / (2.0 * Z90)
    with capsys.disabled():
        print("8 schools: %d of %d prior draws kept; mu: prior median %.4f (se %.4f), robust sd %.4f (se %.4f); contraction %.4f; "
              "prior_time_sec %.3f" % (kept, R, median, se_median, scale, se_scale, float(z["contraction/mu"]), r["prior_time_sec"][0]))
    assert abs(median) <= 5.0 * se_median and abs(scale - 5.0) <= 5.0 * se_scale
    assert 0.0 < float(z["contraction/mu"]) < 1.0
    rhat = np.load(path(on, "_rhat.npz"))
    assert float(z["contraction/mu"]) == pytest.approx(1.0 - (float(rhat["posterior_sd/mu"]) / scale) ** 2, rel=1e-9)
    assert float(z["z_score/mu"]) == pytest.approx((float(rhat["posterior_mean/mu"]) - median) / scale, rel=1e-9, abs=1e-12)
    # analyze --prior prints both lines for the flagged run, nothing for the other
    root = os.path.dirname(on)
    analyze.main(["--results_dir=" + root, "--model=on", "--prior"])
    shown = capsys.readouterr().out
    lines = [l for l in shown.splitlines() if l.startswith("CP_tied:")]
    assert len(lines) == 2 and "prior predictive p-values" in lines[0] and "%d prior draws" % kept in lines[0]
    assert "least contraction {:.4g} ({})".format(r["prior_contraction_min"][0], r["prior_contraction_min_element"][0]) in lines[1]
    analyze.main(["--results_dir=" + root, "--model=off", "--prior"])
    assert "CP_tied:" not in capsys.readouterr().out


def test_german_credit_gammascale(gpu, tmp_path):
    """The log-Gamma form end to end, on Bernoulli data: sd, min and max are not defined"""
    from autoreparam_amd import main as cli
    on, _ = pipeline(str(tmp_path), "german_credit_gammascale", "NCP", ["--loo_draws=8192"], False)
    r = json.load(open(os.path.join(on, "NCP_tied.json")))
    assert all(key in r and len(r[key]) == 1 for key in cli.PRIOR_KEYS)
    for key in ("prior_p_sd", "prior_p_min", "prior_p_max", "prior_rep_sd_q05", "prior_rep_sd_q50", "prior_rep_sd_q95",
                "prior_rep_min_q05", "prior_rep_max_q95", "prior_obs_sd"):
        assert r[key][0] is None, key
    assert r["prior_draws"][0] > 0 and r["prior_draws"][0] + r["prior_draws_left_out"][0] == 8192
    assert 0.0 <= r["prior_p_mean"][0] <= 1.0 and 0.0 <= r["prior_rep_mean_q05"][0] <= r["prior_rep_mean_q95"][0] <= 1.0
    z = np.load(os.path.join(on, "NCP_tied_prior.npz"))
    assert z["draw_stats"].shape == (8192, 8) and int(z["left_out"].sum()) == r["prior_draws_left_out"][0]
    print("german_credit_gammascale: %d of 8192 prior draws left out, prior_time_sec %.3f" % (
        r["prior_draws_left_out"][0], r["prior_time_sec"][0]))


def test_the_funnel_is_refused_before_the_run(gpu, tmp_path):
    with pytest.raises(ValueError, match="--prior_predictive_checks: neals_funnel has no observations"):
        _cli(["--model=neals_funnel", "--num_chains=64", "--method=CP", "--inference=HMC", "--prior_predictive_checks",
              "--results_dir=" + str(tmp_path)] + HM)
    assert os.listdir(str(tmp_path)) == []
