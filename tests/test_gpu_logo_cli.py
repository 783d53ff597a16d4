"""GPU: --loo_groups end to end through main.main, following test_gpu_loo_cli.pipeline (NCP, 256 chains, 200 samples,
--loo_draws=8192, one copied VI / tuning directory).  Radon MA grouped by m (13 counties), two sampling runs:
--predictive_diagnostics alone and with the flag.  The flag adds exactly LOGO_KEYS and <method>_logo.npz and changes nothing
else, bit for bit (every LOO_KEYS value, every array of _loo.npz); the totals are the npz columns folded by
psis_ref.summary; the columns are psis_ref.psis_loo of the device's own lm and lc (diagnostics.group_loglik called here on
the draws the report takes), within test_gpu_psis's FACTOR, K_MEASURED and ELPD_MEASURED; lm itself against tests/logo_ref.py
on the trace, within twice the bound of the header of csrc/logo.hip.  Election grouped by a (Bernoulli data, 51 states of
which 3 are empty, 15 observations in no state): the conditional keys filled, the marginal ones null with the one message.
A refused part raises before the run."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import logo_ref as lg
import psis_ref as pr
from test_gpu_loo_cli import HM, _cli, pipeline
from test_gpu_ppc import FACTOR as BOUND_FACTOR
from test_gpu_psis import ELPD_MEASURED, FACTOR, K_MEASURED

pytestmark = pytest.mark.gpu

FOUR = ("elpd_logo_g", "pareto_k", "lppd_g", "p_waic_g")
FILES = sorted(["part", "groups", "group_of", "n_obs", "y", "model"] + [pre + name for pre in ("", "conditional_") for name in FOUR])
RUN = ["--predictive_diagnostics", "--loo_draws=8192"]


def path(root, suffix):
    return os.path.join(root, "NCP_tied" + suffix)


def pair(on, off, model, extra, part, out):
    """test_gpu_loo_cli.pipeline with BOTH sampling runs under --predictive_diagnostics: `off` without --loo_groups, `on` with."""
    common = ["--model=" + model, "--num_chains=256", "--seed=3", "--num_optimization_steps=400", "--method=NCP"] + extra
    _cli(common + ["--results_dir=" + on, "--inference=VI"])
    _cli(common + ["--results_dir=" + on, "--inference=HMCtuning", "--num_leapfrog_steps=4"] + HM)
    shutil.copytree(on, off)
    _cli(common + ["--results_dir=" + off, "--inference=HMC"] + RUN + HM)
    _cli(common + ["--results_dir=" + on, "--inference=HMC", "--loo_groups=" + part] + RUN + HM, out=out)


def report_draws(out):
    from autoreparam_amd import main as cli
    trace = out["kernel_results"].trace
    steps = cli.loo_steps(int(trace.shape[0]), 256, 8192)
    draws = trace[torch.as_tensor(steps, device=trace.device), :256].contiguous()
    assert draws.shape[0] * draws.shape[1] == 8192
    return draws


def check_form(r, z, prefix, key_prefix, elpd_key):
    """The JSON totals of one form are its npz columns folded by the definition's host formulas; the columns are the
    definition's on the device's own group log-likelihoods (`ref`, psis_ref.psis_loo's rows)."""
    total = pr.summary(z[prefix + "elpd_logo_g"], z[prefix + "lppd_g"], z[prefix + "p_waic_g"])
    names = list(z["groups"])
    assert r[elpd_key][0] == pytest.approx(total["elpd_loo"], rel=1e-12)
    assert r[elpd_key + "_se"][0] == pytest.approx(total["elpd_loo_se"], rel=1e-12)
    assert r["p_logo" if not prefix else "logo_conditional_p"][0] == pytest.approx(total["p_loo"], rel=1e-12)
    k = z[prefix + "pareto_k"]
    finite = np.where(np.isfinite(k), k, -np.inf)
    assert r[key_prefix + "pareto_k_max"][0] == finite.max() and r[key_prefix + "pareto_k_max_group"][0] == names[int(finite.argmax())]
    assert r[key_prefix + "pareto_k_above_threshold"][0] == int(np.sum(k > r["logo_pareto_k_threshold"][0]))


def check_columns(z, prefix, ll):
    ref = pr.psis_loo(ll)
    k_gap = np.abs(z[prefix + "pareto_k"] - ref[:, 1])
    e_gap = np.abs(z[prefix + "elpd_logo_g"] - ref[:, 0]) / np.maximum(1.0, np.abs(ref[:, 0]))
    print("%scolumns against psis_ref: k-hat within %.3g (allowed %.3g), elpd within %.3g relative (allowed %.3g); k-hat %.3g ... %.3g"
          % (prefix, k_gap.max(), FACTOR * K_MEASURED, e_gap.max(), FACTOR * ELPD_MEASURED, ref[:, 1].min(), ref[:, 1].max()))
    assert np.all(k_gap <= FACTOR * K_MEASURED)
    assert np.all(e_gap <= FACTOR * ELPD_MEASURED)
    assert np.allclose(z[prefix + "lppd_g"], ref[:, 2], rtol=1e-12) and np.allclose(z[prefix + "p_waic_g"], ref[:, 3], rtol=1e-10)


def test_radon_by_county_end_to_end(gpu, tmp_path, capsys):
    from autoreparam_amd import analyze, diagnostics, main as cli, models
    on, off, out = str(tmp_path / "on"), str(tmp_path / "off"), {}
    pair(on, off, "radon", ["--dataset=MA"], "m", out)
    text = capsys.readouterr().out
    r, plain = json.load(open(path(on, ".json"))), json.load(open(path(off, ".json")))
    # the flag adds LOGO_KEYS and the side file and changes nothing else
    assert set(r) - set(plain) == set(cli.LOGO_KEYS) and set(plain) <= set(r)
    assert os.path.exists(path(on, "_logo.npz")) and not os.path.exists(path(off, "_logo.npz"))
    for key in plain:
        if "time" not in key:
            assert plain[key] == r[key], key
    for suffix in ("_loo.npz", "_rhat.npz", "_ess.npz"):
        a, b = np.load(path(on, suffix)), np.load(path(off, suffix))
        assert sorted(a.files) == sorted(b.files), suffix
        assert all(a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes() for name in a.files), suffix
    for key in cli.LOGO_KEYS:
        assert len(r[key]) == 1 and r[key][0] is not None, key
    sp = models._spec_radon("MA")
    N = len(sp.raw["y"])
    assert r["logo_part"] == ["m"] and r["logo_groups"] == [13] and r["logo_groups_empty"] == [0] and r["logo_marginal"] == [True]
    assert r["logo_observations_left_out"] == [0] and r["logo_draws"] == [8192] and r["logo_nonfinite_groups"] == [0]
    assert r["logo_pareto_k_threshold"][0] == pytest.approx(pr.k_threshold(8192))
    assert 0 < r["logo_time_sec"][0] <= r["loo_time_sec"][0] <= r["diagnostics_time_sec"][0]
    z = np.load(path(on, "_logo.npz"))
    assert sorted(z.files) == FILES and str(z["part"]) == "m" and str(z["model"]) == "radon" and list(z["groups"])[4] == "m[4]"
    county = np.asarray(sp.raw["county"]).reshape(-1)
    assert np.array_equal(z["group_of"], county) and np.array_equal(z["n_obs"], np.bincount(county, minlength=13))
    assert np.array_equal(z["y"], np.asarray(sp.raw["y"], np.float32)) and z["y"].size == N
    check_form(r, z, "", "logo_", "elpd_logo")
    check_form(r, z, "conditional_", "logo_conditional_", "logo_conditional_elpd")
    assert r["elpd_logo"][0] < 0 and r["elpd_logo_se"][0] > 0 and r["p_logo"][0] > 0
    # the printed line sets the two forms next to each other
    line = [l for l in text.splitlines() if l.startswith("    PSIS leave-one-group-out by m: 13 groups (0 empty, 0 observations in none), 8192 draws")]
    assert len(line) == 1 and "marginal elpd_logo {:.4g} +/- {:.4g}, worst Pareto k-hat {:.4g} ({})".format(
        r["elpd_logo"][0], r["elpd_logo_se"][0], r["logo_pareto_k_max"][0], r["logo_pareto_k_max_group"][0]) in line[0]
    assert "; conditional elpd {:.4g} +/- {:.4g}, worst Pareto k-hat {:.4g}".format(
        r["logo_conditional_elpd"][0], r["logo_conditional_elpd_se"][0], r["logo_conditional_pareto_k_max"][0]) in line[0]
    with capsys.disabled():
        print("\n" + line[0].strip())
        print("elpd_loo %.6g; logo_time_sec %.3f of loo_time_sec %.3f" % (r["elpd_loo"][0], r["logo_time_sec"][0], r["loo_time_sec"][0]))
    # the columns against the definition on the device's own lm and lc of the draws the report takes
    draws = report_draws(out)
    host, site_host = sp.observation_table(), sp.site_table()
    table = diagnostics.upload_table(host, sp.D, gpu)
    group_of, names, slope, elem, ok, why = diagnostics.marginal_selection(site_host, host, sp, "m")
    assert ok and why is None and names == list(z["groups"])
    groups = diagnostics.upload_logo_groups(*diagnostics.group_order(group_of, 13), slope, elem, N, sp.D, gpu)
    site = diagnostics.upload_site_table(site_host, sp.D, gpu)
    lc, lm, mask, count = diagnostics.group_loglik(draws, table, groups, site)
    assert int(count.item()) == 0
    lc, lm = lc.cpu().numpy(), lm.cpu().numpy()
    with capsys.disabled():
        check_columns(z, "", lm)
        check_columns(z, "conditional_", lc)
    # lm against the float64 reference on the trace, at eight of the draws (a county has up to 391 observations)
    picked = np.arange(0, 8192, 1024) + 5
    x = draws.reshape(-1, sp.D)[torch.as_tensor(picked, device=gpu)].cpu().numpy()
    float_table = type(host)(host.kind, np.asarray(host.idx), np.asarray(host.w, np.float32), np.asarray(host.y, np.float32),
                             np.asarray(host.scale_idx), np.asarray(host.log_scale, np.float32))
    q = lg.quantities(float_table, site.host, x, slope, elem)
    ref = lg.marginal(float_table, q, group_of, 13, slope)
    allow = lg.bound(float_table, q, group_of, 13, ref)
    gap = np.abs(lm[:, picked].astype(np.float64) - ref)
    with capsys.disabled():
        print("lm against logo_ref on the trace: largest share of the bound used %.3f; bound up to %.3g at |lm| up to %.3g"
              % (float(np.max(gap / allow)), float(allow.max()), float(np.abs(ref).max())))
    assert np.all(gap <= BOUND_FACTOR * allow)
    # analyze --loo prints the line; a run without the flag prints none
    analyze.main(["--results_dir=" + str(tmp_path), "--model=on", "--loo"])
    shown = capsys.readouterr().out
    assert "      leave-one-group-out by m: 13 groups (0 empty, 0 observations in none); marginal elpd_logo {:.4g} +/- {:.4g}".format(
        r["elpd_logo"][0], r["elpd_logo_se"][0]) in shown
    analyze.main(["--results_dir=" + str(tmp_path), "--model=off", "--loo"])
    assert "leave-one-group-out" not in capsys.readouterr().out
    analyze.main(["--logo_compare=%s,%s" % (path(on, "_logo.npz"), path(on, "_logo.npz"))])
    assert "elpd_logo(radon) - elpd_logo(radon) = 0 +/- 0 over 13 groups of m (marginal)" in capsys.readouterr().out


def test_election_by_state_has_the_conditional_form_only(gpu, tmp_path, capsys):
    from autoreparam_amd import main as cli
    root = str(tmp_path / "election")
    pipeline(root, "election", [], RUN + ["--loo_groups=a"])
    text = capsys.readouterr().out
    r = json.load(open(path(root, ".json")))
    assert set(cli.LOGO_KEYS) <= set(r)
    for key in cli.LOGO_MARGINAL_KEYS:
        assert r[key] == [None], key
    for key in set(cli.LOGO_KEYS) - set(cli.LOGO_MARGINAL_KEYS):
        assert len(r[key]) == 1 and r[key][0] is not None, key
    assert r["logo_marginal"] == [False] and r["logo_part"] == ["a"] and r["logo_groups"] == [51]
    assert r["logo_groups_empty"] == [3] and r["logo_observations_left_out"] == [15] and r["logo_draws"] == [8192]
    assert text.count("marginal leave-one-group-out by a: not computed, the data are Bernoulli") == 1
    assert "marginal elpd_logo n/a; conditional elpd {:.4g} +/- {:.4g}".format(
        r["logo_conditional_elpd"][0], r["logo_conditional_elpd_se"][0]) in text
    for key in cli.LOO_KEYS:
        assert r[key][0] is not None, key
    z = np.load(path(root, "_logo.npz"))
    assert sorted(z.files) == FILES and z["group_of"].size == r["loo_observations"][0]
    empty = z["n_obs"] == 0
    assert int(empty.sum()) == 3 and int(np.sum(z["group_of"] < 0)) == 15
    for name in FOUR:
        assert np.all(np.isnan(z[name])), name                             # no marginal form: NaN throughout
        assert np.all(np.isnan(z["conditional_" + name][empty])) and not np.isnan(z["conditional_" + name][~empty]).any(), name
    filled = {name: z[name][~empty] for name in ["groups"] + ["conditional_" + name for name in FOUR]}
    check_form(r, filled, "conditional_", "logo_conditional_", "logo_conditional_elpd")
    with capsys.disabled():
        print("\n" + [l for l in text.splitlines() if "PSIS leave-one-group-out by a" in l][0].strip())
        print("logo_time_sec %.3f of loo_time_sec %.3f" % (r["logo_time_sec"][0], r["loo_time_sec"][0]))


def test_a_refused_part_raises_before_the_run(gpu, tmp_path):
    root = str(tmp_path / "refused")
    args = ["--model=radon", "--dataset=MA", "--num_chains=256", "--method=NCP", "--results_dir=" + root, "--inference=HMC",
            "--predictive_diagnostics"] + HM
    for part, word in (("b1", "one element"), ("county", "no latent part of radon")):
        with pytest.raises(ValueError, match="^--loo_groups: .*" + word):
            _cli(args + ["--loo_groups=" + part])
    with pytest.raises(ValueError, match="--loo_groups is read with --predictive_diagnostics only"):
        _cli([a for a in args if a != "--predictive_diagnostics"] + ["--loo_groups=m"])
    assert not os.path.exists(root)
