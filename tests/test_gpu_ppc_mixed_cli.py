"""GPU: --predictive_checks_redraw end to end through main.main, on the helpers of tests/test_gpu_ppc.py (256 chains, 200
samples, --loo_draws=8192, one copied VI / tuning directory): radon MA, NCP, with m redrawn (Normal data, 13 counties), and
German credit with Gamma scales with beta_log_scales and beta redrawn (Bernoulli data, the log-Gamma form), each against
the run with --predictive_checks alone -- the flag adds exactly PPC_MIXED_KEYS and <method>_ppc_mixed.npz and changes nothing
else: every PPC_KEYS value but the time and every array of <method>_ppc.npz is the unflagged run's; the mixed keys are
finite where defined, null where the kind of data says so, and are recomputed here from the side file through
diagnostics.ppc_summary; analyze --ppc prints both lines; a refused selection raises before the run."""
import json
import math
import os
import shutil

import numpy as np
import pytest

from test_gpu_ppc import HM, _cli

pytestmark = pytest.mark.gpu

BERNOULLI_NULLS = ("ppc_mixed_p_sd", "ppc_mixed_p_min", "ppc_mixed_p_max", "ppc_mixed_rep_sd", "ppc_mixed_pit_ks",
                   "ppc_mixed_coverage_90", "ppc_mixed_pit_extreme_observations", "ppc_mixed_pit_min_observation")


def pipeline(root, model, extra, method, parts):
    """VI and one tuning run of `model` under root/mixed, copied to root/plain; the sampling run with --predictive_checks
    under plain and with --predictive_checks_redraw added under mixed.  Returns (mixed, plain)."""
    mixed, plain = os.path.join(root, "mixed"), os.path.join(root, "plain")
    common = ["--model=" + model, "--num_chains=256", "--seed=3", "--num_optimization_steps=400", "--method=" + method] + extra
    _cli(common + ["--results_dir=" + mixed, "--inference=VI"])
    _cli(common + ["--results_dir=" + mixed, "--inference=HMCtuning", "--num_leapfrog_steps=4"] + HM)
    shutil.copytree(mixed, plain)
    run = ["--inference=HMC", "--predictive_checks", "--loo_draws=8192"] + HM
    _cli(common + ["--results_dir=" + plain] + run)
    _cli(common + ["--results_dir=" + mixed, "--predictive_checks_redraw=" + parts] + run)
    return mixed, plain


def check_cli(tmp_path, capsys, model, extra, method, parts, chosen, elements, kind, N):
    from autoreparam_amd import analyze, diagnostics, main as cli
    capsys.readouterr()
    mixed, plain = pipeline(str(tmp_path), model, extra, method, parts)
    text = capsys.readouterr().out
    assert text.count("posterior predictive checks over %d observations" % N) == 2
    assert text.count("mixed predictive checks, %s redrawn from the conditional prior (%d elements)" % (", ".join(chosen), elements)) == 1
    path = lambda root, suffix: os.path.join(root, method + "_tied" + suffix)
    r, base = json.load(open(path(mixed, ".json"))), json.load(open(path(plain, ".json")))
    # the flag adds its keys and its file, and changes nothing else
    assert set(r) - set(base) == set(cli.PPC_MIXED_KEYS) and set(base) <= set(r) and set(cli.PPC_KEYS) <= set(base)
    for key in base:
        if "time" not in key:
            assert base[key] == r[key], key
    for suffix in ("_ppc.npz", "_rhat.npz", "_ess.npz"):
        a, b = np.load(path(mixed, suffix)), np.load(path(plain, suffix))
        assert sorted(a.files) == sorted(b.files), suffix
        for name in a.files:
            assert a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), (suffix, name)
    assert os.path.exists(path(mixed, "_ppc_mixed.npz")) and not os.path.exists(path(plain, "_ppc_mixed.npz"))
    # the keys: one value each, finite where defined, null where the kind of data says so
    normal = kind == 0
    for key in cli.PPC_MIXED_KEYS:
        assert len(r[key]) == 1, key
        value = r[key][0]
        if not normal and key in BERNOULLI_NULLS:
            assert value is None, key
        else:
            assert value is not None and (isinstance(value, list) or math.isfinite(value)), key
    for name in ("p_sd", "p_min", "p_max", "rep_sd", "pit_ks", "coverage_90", "p_mean", "p_deviance", "rep_mean"):
        assert (r["ppc_mixed_" + name][0] is None) == (r["ppc_" + name][0] is None), name
    assert r["ppc_mixed_parts"] == [list(chosen)] and r["ppc_mixed_elements"] == [elements]
    assert r["ppc_mixed_draws"][0] + r["ppc_mixed_draws_left_out"][0] == 8192 == r["ppc_draws"][0]
    assert 0 < r["ppc_mixed_time_sec"][0] < r["ppc_time_sec"][0] <= r["diagnostics_time_sec"][0]
    # the side file, and the keys recomputed from it through the one definition
    z = np.load(path(mixed, "_ppc_mixed.npz"))
    assert sorted(z.files) == ["draw_stats", "model", "parts", "pit", "predictive_mean", "predictive_sd", "redrawn", "y"]
    assert list(z["parts"]) == list(chosen) and z["redrawn"].dtype == np.uint8 and int(z["redrawn"].sum()) == elements
    assert str(z["model"]) == model and z["draw_stats"].shape == (8192, 8)
    assert all(z[k].shape == (N,) for k in ("pit", "predictive_mean", "predictive_sd", "y"))
    posterior = np.load(path(mixed, "_ppc.npz"))
    assert np.array_equal(z["y"], posterior["y"]) and not np.array_equal(z["draw_stats"], posterior["draw_stats"])
    left = z["draw_stats"][:, 7] == 0
    used = int((~left).sum())
    assert used == r["ppc_mixed_draws"][0] and used > 0.99 * 8192
    sums = np.zeros((N, 4))
    sums[:, 0], sums[:, 2] = z["predictive_mean"] * used, z["pit"] * used
    sums[:, 1] = (z["predictive_sd"] ** 2 + z["predictive_mean"] ** 2) * used
    s = diagnostics.ppc_summary(z["draw_stats"], sums, z["y"], kind, left)
    want = cli.ppc_mixed_keys(s, chosen, elements, kind)
    for key, value in want.items():
        if key in ("ppc_mixed_pit_ks", "ppc_mixed_coverage_90", "ppc_mixed_pit_extreme_observations", "ppc_mixed_pit_min_observation"):
            continue                                                         # (from the stored PIT itself, below: pit * used / used rounds)
        assert r[key][0] == value, key
    for name in diagnostics.PPC_STATISTICS:
        assert s.p[name] is None or 0.0 <= s.p[name] <= 1.0
    if normal:
        ks, coverage = diagnostics._pit_calibration(z["pit"])
        assert r["ppc_mixed_pit_ks"][0] == ks and r["ppc_mixed_coverage_90"][0] == coverage
        out = [int(n) for n in np.flatnonzero((z["pit"] < 0.01) | (z["pit"] > 0.99))]
        assert r["ppc_mixed_pit_extreme_observations"][0] == out and r["ppc_mixed_pit_min_observation"][0] == int(np.argmin(z["pit"]))
        assert np.all((z["pit"] >= 0) & (z["pit"] <= 1)) and np.all(z["predictive_sd"] > 0)
    # the warning line names exactly the statistics with an extreme mixed p-value
    extreme = [name for name in diagnostics.PPC_STATISTICS if s.p[name] is not None and not 0.01 <= s.p[name] <= 0.99]
    warned = [l for l in text.splitlines() if "WARNING: mixed predictive p-value outside" in l]
    assert len(warned) == (1 if extreme else 0) and all("for: " + ", ".join(extreme) + " --" in l for l in warned)
    # analyze --ppc: both lines for the flagged run, one for the other
    root = os.path.dirname(mixed)
    analyze.main(["--results_dir=" + root, "--model=mixed", "--ppc"])
    shown = capsys.readouterr().out
    assert shown.count("%s_tied: predictive p-values mean" % method) == 1
    assert shown.count("mixed predictive, %s redrawn (%d elements)" % (",".join(chosen), elements)) == 1
    analyze.main(["--results_dir=" + root, "--model=plain", "--ppc"])
    shown = capsys.readouterr().out
    assert shown.count("%s_tied: predictive p-values mean" % method) == 1 and "mixed predictive" not in shown
    with capsys.disabled():
        print("%s, %s redrawn: ppc_mixed_time_sec %.3f of ppc_time_sec %.3f; mixed (posterior) p sd %s (%s), p deviance %s (%s), "
              "PIT ks %s (%s), coverage %s (%s)" % (
                  model, ",".join(chosen), r["ppc_mixed_time_sec"][0], r["ppc_time_sec"][0], r["ppc_mixed_p_sd"][0], r["ppc_p_sd"][0],
                  r["ppc_mixed_p_deviance"][0], r["ppc_p_deviance"][0], r["ppc_mixed_pit_ks"][0], r["ppc_pit_ks"][0],
                  r["ppc_mixed_coverage_90"][0], r["ppc_coverage_90"][0]))
    return r, z, posterior


def test_radon_with_the_county_effects_redrawn(gpu, tmp_path, capsys):
    r, z, posterior = check_cli(tmp_path, capsys, "radon", ["--dataset=MA"], "NCP", "m", ("m",), 13, 0, 1659)
    # a new county's level is less certain than a fitted one's: the mixed predictive sd of every observation is the wider
    assert np.all(z["predictive_sd"] > posterior["predictive_sd"])


def test_german_credit_gammascale_with_both_layers_redrawn(gpu, tmp_path, capsys):
    """Bernoulli data and the log-Gamma form: the scales of the coefficients are drawn from their Gamma prior, the
    coefficients from the redrawn scales; the order the parts are named in does not matter"""
    check_cli(tmp_path, capsys, "german_credit_gammascale", [], "NCP", "beta,beta_log_scales", ("beta_log_scales", "beta"), 124, 1, 1000)


def test_a_selection_that_is_not_closed_is_refused_before_the_run(gpu, tmp_path):
    with pytest.raises(ValueError, match="--predictive_checks_redraw: m would stay as recorded .* add m; the model's parts: mua, b1, b2, m"):
        _cli(["--model=radon", "--dataset=MA", "--num_chains=64", "--method=CP", "--inference=HMC", "--predictive_checks",
              "--predictive_checks_redraw=mua", "--results_dir=" + str(tmp_path)] + HM)
    assert os.listdir(str(tmp_path)) == []
