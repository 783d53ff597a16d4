"""GPU: --loo_predictive end to end, on the pipeline of tests/test_gpu_loo_cli.py (NCP, 256 chains, 200 samples): 8 schools
(Normal) and German credit at --loo_draws=8192 (Bernoulli), each run with --predictive_diagnostics alone and with
--loo_predictive added, from one copied VI / tuning directory.  The flag adds exactly LOO_PRED_KEYS and
<method>_loopred.npz and changes nothing else: every other key (timing apart) and every array of _loo.npz, _rhat.npz and
_ess.npz is the unflagged run's.  The new file's columns are the one host definition applied to the kernel's sums of the
recorded trace, bit for bit, those sums agree with tests/loopred_ref.py on the device's own lw within the parity
allowances of tests/test_gpu_loopred.py, and the JSON figures are loopred_ref's summary of them.  A report forced into
several tiles gives the one-tile arrays bit for bit; analyze --loo prints the new line for the flagged run only."""
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

import loopred_ref as lr
from test_gpu_loo_cli import HM, _cli
from test_gpu_loopred import allowances

pytestmark = pytest.mark.gpu

NORMAL_NULLS = ("loo_brier", "loo_accuracy", "loo_balanced_accuracy")
BERNOULLI_NULLS = ("loo_pit_ks", "loo_coverage_90", "loo_rmse", "loo_r2")


def pipeline(root, model, extra):
    """VI and one tuning run of `model` under root/on, copied to root/off; then the sampling run with
    --predictive_diagnostics under off and with --loo_predictive added under on.  Returns (on, off, the flagged run's `out`)."""
    on, off, out = os.path.join(root, "on"), os.path.join(root, "off"), {}
    common = ["--model=" + model, "--num_chains=256", "--seed=3", "--num_optimization_steps=400", "--method=NCP"]
    _cli(common + ["--results_dir=" + on, "--inference=VI"])
    _cli(common + ["--results_dir=" + on, "--inference=HMCtuning", "--num_leapfrog_steps=4"] + HM)
    shutil.copytree(on, off)
    _cli(common + ["--results_dir=" + off, "--inference=HMC", "--predictive_diagnostics"] + extra + HM)
    _cli(common + ["--results_dir=" + on, "--inference=HMC", "--predictive_diagnostics", "--loo_predictive"] + extra + HM, out=out)
    return on, off, out


def check_run(root, capsys, model, extra, spec, kind, nulls, draws, steps):
    from autoreparam_amd import analyze, diagnostics, main as cli
    capsys.readouterr()
    on, off, out = pipeline(root, model, extra)
    text = capsys.readouterr().out
    N = int(np.asarray(spec.observation_table().y).size)
    assert text.count("LOO predictive report over %d observations" % N) == 1 and text.count("PSIS-LOO over %d observations" % N) == 2
    path = lambda d, suffix: os.path.join(d, "NCP_tied" + suffix)
    r, plain = json.load(open(path(on, ".json"))), json.load(open(path(off, ".json")))
    # the flag adds its keys and its file, and changes nothing else
    assert set(r) - set(plain) == set(cli.LOO_PRED_KEYS) and set(plain) <= set(r)
    for key in plain:
        if "time" not in key:
            assert plain[key] == r[key], key
    for suffix in ("_loo.npz", "_rhat.npz", "_ess.npz"):
        a, b = np.load(path(on, suffix)), np.load(path(off, suffix))
        assert sorted(a.files) == sorted(b.files), suffix
        assert all(np.array_equal(a[name], b[name], equal_nan=a[name].dtype.kind == "f") for name in a.files), suffix
    assert os.path.exists(path(on, "_loopred.npz")) and not os.path.exists(path(off, "_loopred.npz"))
    for key in cli.LOO_PRED_KEYS:
        assert len(r[key]) == 1, key
        if key in nulls:
            assert r[key][0] is None, key
        else:
            assert r[key][0] is not None and math.isfinite(r[key][0]), key
    assert r["loo_pred_observations"] == [N] and r["loo_pred_observations_left_out"] == [0] and r["loo_draws"] == [draws]
    assert 0 < r["loo_pred_time_sec"][0] <= r["loo_time_sec"][0] <= r["diagnostics_time_sec"][0]
    z = np.load(path(on, "_loopred.npz"))
    assert sorted(z.files) == ["loo_is_ess", "loo_mean", "loo_pit", "loo_sd", "model", "y"] and str(z["model"]) == model
    assert all(z[name].shape == (N,) and np.isfinite(z[name]).all() for name in ("loo_is_ess", "loo_mean", "loo_pit", "loo_sd", "y"))
    assert np.all((z["loo_pit"] > 0) & (z["loo_pit"] < 1)) and np.all(z["loo_sd"] > 0) and np.all((z["loo_is_ess"] >= 1 - 1e-12) & (z["loo_is_ess"] <= draws))
    # the kernel's sums on the recorded trace, with the device's own lw
    trace = out["kernel_results"].trace
    picked = cli.loo_steps(int(trace.shape[0]), 256, draws if extra else 65536)
    assert len(picked) == steps and len(picked) * 256 == draws
    x = trace[torch.as_tensor(picked, device=trace.device), :256].contiguous()
    table = spec.observation_table()
    dt = diagnostics.upload_table(table, spec.D, trace.device)
    ll, mask, count = diagnostics.pointwise_loglik(x, dt)
    out8, lw = diagnostics.psis_weights(ll, mask)
    sums = diagnostics.loo_predictive(x, dt, lw).cpu().numpy()
    assert int(count.item()) == 0 and np.all(sums[:, 5] == draws)
    assert np.array_equal(out8.cpu().numpy()[:, 0], np.load(path(on, "_loo.npz"))["elpd_loo_i"])
    # ... are what the file's columns were made of, through the one host definition, bit for bit
    s = diagnostics.loo_predictive_summary(sums, table.y, kind)
    for name, col in (("loo_mean", s.loo_mean), ("loo_sd", s.loo_sd), ("loo_pit", s.loo_pit), ("loo_is_ess", s.is_ess)):
        assert np.array_equal(z[name], col), name
    assert np.array_equal(z["y"], np.asarray(table.y, np.float32))
    # ... and agree with the float64 definition within the parity allowances (in slabs of observations: [R, n, T] float64)
    xh, lwh = x.cpu().numpy().reshape(draws, spec.D), lw.cpu().numpy()
    ref_sums = np.zeros((N, 6))
    for n0 in range(0, N, 100):
        n1 = min(N, n0 + 100)
        c = lr.columns(table, xh, lwh[n0:n1], n0, n1)
        allow = allowances(table, c, n0, n1)
        gap = np.abs(sums[n0:n1, :5] - c.sums[:, :5])
        assert np.all(gap <= allow), (n0, [float(np.max(gap[:, j] / np.maximum(allow[:, j], 1e-300))) for j in range(5)])
        assert np.array_equal(sums[n0:n1, 5], c.sums[:, 5])
        ref_sums[n0:n1] = c.sums
    want = lr.summary(ref_sums, table.y, kind)
    for name in ("loo_mean", "loo_sd", "loo_pit"):                       # ratios of sums that agree to about 2^-24 relative
        assert np.allclose(z[name], want[name], rtol=1e-4, atol=1e-6), name
    assert np.allclose(z["loo_is_ess"], want["is_ess"], rtol=1e-10)
    # the JSON figures are the reference's summary of the file's sums
    mine = lr.summary(sums, table.y, kind)
    for key, name in (("loo_pit_ks", "pit_ks"), ("loo_coverage_90", "coverage_90"), ("loo_rmse", "rmse"), ("loo_r2", "r2"),
                      ("loo_brier", "brier"), ("loo_accuracy", "accuracy"), ("loo_balanced_accuracy", "balanced_accuracy"),
                      ("loo_is_ess_min", "is_ess_min")):
        if mine[name] is None:
            assert r[key][0] is None, key
        else:
            assert r[key][0] == pytest.approx(mine[name], rel=1e-12), key
    assert r["loo_is_ess_min_observation"][0] == mine["is_ess_min_observation"] == int(np.argmin(z["loo_is_ess"]))
    # analyze --loo: the new line for the flagged run, not for the other
    base = os.path.dirname(on)
    analyze.main(["--results_dir=" + base, "--model=on", "--loo"])
    shown = capsys.readouterr().out
    assert shown.count("LOO predictive:") == 1 and "NCP_tied: elpd_loo" in shown
    assert "smallest importance-sampling ESS {:.4g} (observation {})".format(r["loo_is_ess_min"][0], r["loo_is_ess_min_observation"][0]) in shown
    analyze.main(["--results_dir=" + base, "--model=off", "--loo"])
    shown = capsys.readouterr().out
    assert "LOO predictive" not in shown and "NCP_tied: elpd_loo" in shown
    return r, z


def test_eight_schools_normal(gpu, tmp_path, capsys):
    from autoreparam_amd import models
    r, z = check_run(str(tmp_path), capsys, "8schools", [], models._spec_eight_schools(), lr.NORMAL, NORMAL_NULLS, 51200, 200)
    assert 0.0 < r["loo_pit_ks"][0] < 1.0 and 0.0 <= r["loo_coverage_90"][0] <= 1.0 and r["loo_rmse"][0] > 0
    assert np.all(z["loo_sd"] > 9.0)                                      # at least the known sigma of the smallest school


def test_german_credit_bernoulli(gpu, tmp_path, capsys):
    from autoreparam_amd import models
    r, z = check_run(str(tmp_path), capsys, "german_credit_lognormalcentered", ["--loo_draws=8192"], models._spec_german(),
                     lr.BERNOULLI, BERNOULLI_NULLS, 8192, 32)
    assert 0.0 < r["loo_brier"][0] < 0.25 and 0.5 < r["loo_accuracy"][0] <= 1.0 and 0.5 < r["loo_balanced_accuracy"][0] <= 1.0
    assert np.all((z["loo_mean"] > 0) & (z["loo_mean"] < 1)) and np.allclose(z["loo_sd"] ** 2, z["loo_mean"] * (1 - z["loo_mean"]), atol=1e-6)


def test_several_tiles_give_the_arrays_of_one(gpu, monkeypatch):
    """German credit's table on a synthetic trace, R = 256: a budget of 100 rows per tile (ll and lw together) against one
    tile -- the per-observation sums do not depend on the observation range of a call, so both files' arrays are equal bit
    for bit, and the unflagged report's too."""
    from autoreparam_amd import main as cli, models
    sp = models._spec_german()
    N = 1000
    trace = torch.as_tensor((0.1 * np.random.RandomState(0).randn(4, 64, sp.D)).astype(np.float32), device=gpu)
    flagged = type("F", (), {"loo_draws": 65536, "loo_predictive": True})()
    bare = type("F", (), {"loo_draws": 65536})()
    side, side_t = {}, {}
    whole, arrays = cli._loo_report(None, trace, 64, sp, flagged, side)
    plain, arrays_p = cli._loo_report(None, trace, 64, sp, bare, {})
    monkeypatch.setattr(cli, "LOO_CHUNK_BYTES", 100 * 12 * 256)
    assert cli.loo_tile_rows(N, 256, cli.LOO_CHUNK_BYTES // 3) == 100
    tiled, arrays_t = cli._loo_report(None, trace, 64, sp, flagged, side_t)
    assert set(side) == set(side_t) == {cli.LOO_PRED_ARRAYS} and set(whole) == set(cli.LOO_KEYS + cli.LOO_PRED_KEYS)
    for name in ("loo_mean", "loo_sd", "loo_pit", "loo_is_ess", "y"):
        a, b = side[cli.LOO_PRED_ARRAYS][name], side_t[cli.LOO_PRED_ARRAYS][name]
        assert a.shape == (N,) and np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    for name in ("elpd_loo_i", "pareto_k", "lppd_i", "p_waic_i"):
        assert np.array_equal(arrays[name], arrays_t[name], equal_nan=True) and np.array_equal(arrays[name], arrays_p[name], equal_nan=True), name
    timeless = lambda keys: {k: v for k, v in keys.items() if "time" not in k}
    assert timeless(whole) == timeless(tiled) and set(plain) == set(cli.LOO_KEYS)
    assert {k: v for k, v in timeless(whole).items() if k in plain} == timeless(plain)
