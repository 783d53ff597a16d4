"""CPU: the host half of the leave-one-out predictive report -- diagnostics.loo_predictive_summary against the formulas of
tests/loopred_ref.py on synthetic sums (both kinds; a row with S0 = 0, a NaN row, constant y, a single class), the one
calibration helper behind ppc_pit_ks and loo_pit_ks, the key tuple, the flag and its refusals, the null-key path, the side
file's tag, and analyze --loo on synthetic result files with and without the new keys."""
import json
import math

import numpy as np
import pytest
import torch

import loopred_ref as lr


def synthetic_sums(kind, N, seed):
    """[N, 6] sums of R = 200 weighted draws per observation, formed directly (no table): every row is a valid set of sums."""
    rs = np.random.RandomState(seed)
    R = 200
    W = np.exp(-np.abs(3.0 * rs.randn(N, R)))
    if kind == lr.NORMAL:
        mu, var = rs.randn(N, R), np.exp(0.4 * rs.randn(N, R))
        y = mu.mean(1) + rs.randn(N)
        pit = rs.rand(N, R)
    else:
        mu = rs.rand(N, R)
        var = mu * (1.0 - mu)
        y = (rs.rand(N) < 0.5).astype(np.float64)
        pit = np.where(y[:, None] > 0.5, 1.0 - 0.5 * mu, 0.5 * (1.0 - mu))
    sums = np.stack([W.sum(1), (W * W).sum(1), (W * mu).sum(1), (W * (mu * mu + var)).sum(1), (W * pit).sum(1),
                     np.full(N, float(R))], axis=1)
    return sums, y


def same(got, ref):
    """A LooPredSummary against loopred_ref.summary's dict."""
    assert got.observations == ref["observations"] and got.left_out == ref["left_out"]
    for name, mine in (("loo_mean", got.loo_mean), ("loo_sd", got.loo_sd), ("loo_pit", got.loo_pit), ("is_ess", got.is_ess)):
        assert np.allclose(mine, ref[name], rtol=1e-13, atol=0, equal_nan=True), name
        assert np.array_equal(np.isnan(mine), np.isnan(ref[name])) and np.array_equal(np.isinf(mine), np.isinf(ref[name])), name
    for name in ("pit_ks", "coverage_90", "rmse", "r2", "brier", "accuracy", "balanced_accuracy", "is_ess_min"):
        mine = getattr(got, name)
        if ref[name] is None:
            assert mine is None, name
        else:
            assert mine is not None and mine == pytest.approx(ref[name], rel=1e-12, abs=1e-15), name
    assert got.is_ess_min_observation == ref["is_ess_min_observation"]


@pytest.mark.parametrize("kind", (lr.NORMAL, lr.BERNOULLI))
def test_summary_against_the_reference_formulas(kind):
    from autoreparam_amd import diagnostics
    sums, y = synthetic_sums(kind, 37, 5 + kind)
    got = diagnostics.loo_predictive_summary(sums, y, kind)
    same(got, lr.summary(sums, y, kind))
    assert got.observations == 37 and got.left_out == 0 and np.all(got.is_ess > 1.0) and np.all(got.is_ess <= 200.0)
    if kind == lr.NORMAL:
        assert None not in (got.pit_ks, got.coverage_90, got.rmse, got.r2) and 0.0 < got.pit_ks < 1.0
        assert (got.brier, got.accuracy, got.balanced_accuracy) == (None, None, None)
    else:
        assert None not in (got.brier, got.accuracy, got.balanced_accuracy) and 0.0 <= got.accuracy <= 1.0
        assert (got.pit_ks, got.coverage_90, got.rmse, got.r2) == (None, None, None, None)
    # device tensors' host image or plain lists: the same numbers
    again = diagnostics.loo_predictive_summary(torch.as_tensor(sums), list(y), kind)
    assert again.rmse == got.rmse and again.brier == got.brier and np.array_equal(again.loo_mean, got.loo_mean)


@pytest.mark.parametrize("kind", (lr.NORMAL, lr.BERNOULLI))
def test_rows_that_do_not_count_enter_no_total(kind):
    """An observation whose every draw was left out (S0 = 0: all six sums 0), a NaN row, an infinite sum: counted as left
    out, NaN in the arrays, and the totals are those of the other rows alone."""
    from autoreparam_amd import diagnostics
    sums, y = synthetic_sums(kind, 12, 9)
    clean = diagnostics.loo_predictive_summary(np.delete(sums, (2, 5, 7), axis=0), np.delete(y, (2, 5, 7)), kind)
    sums[2] = 0.0
    sums[5, :5] = np.nan
    sums[7, 2] = np.inf
    got = diagnostics.loo_predictive_summary(sums, y, kind)
    same(got, lr.summary(sums, y, kind))
    assert got.observations == 9 and got.left_out == 3
    assert np.isnan(got.loo_mean[2]) and np.isnan(got.is_ess[2]) and np.isnan(got.loo_pit[5]) and np.isinf(got.loo_mean[7])
    for name in ("pit_ks", "coverage_90", "rmse", "r2", "brier", "accuracy", "balanced_accuracy", "is_ess_min"):
        assert getattr(got, name) == getattr(clean, name), name
    at = got.is_ess_min_observation
    assert at not in (2, 5, 7) and got.is_ess[at] == got.is_ess_min
    # nothing counts: every figure None, no exception
    none = diagnostics.loo_predictive_summary(np.zeros((4, 6)), y[:4], kind)
    same(none, lr.summary(np.zeros((4, 6)), y[:4], kind))
    assert none.observations == 0 and none.left_out == 4 and none.is_ess_min is None and none.is_ess_min_observation == -1
    assert all(getattr(none, n) is None for n in ("pit_ks", "coverage_90", "rmse", "r2", "brier", "accuracy", "balanced_accuracy"))
    with pytest.raises(ValueError, match="one row per observation"):
        diagnostics.loo_predictive_summary(np.zeros((4, 6)), y[:3], kind)


def test_constant_y_one_observation_and_a_single_class():
    from autoreparam_amd import diagnostics
    sums, y = synthetic_sums(lr.NORMAL, 6, 3)
    flat = diagnostics.loo_predictive_summary(sums, np.full(6, 1.25), lr.NORMAL)
    same(flat, lr.summary(sums, np.full(6, 1.25), lr.NORMAL))
    assert flat.r2 is None and flat.rmse is not None and flat.pit_ks is not None
    one = diagnostics.loo_predictive_summary(sums[:1], y[:1], lr.NORMAL)
    same(one, lr.summary(sums[:1], y[:1], lr.NORMAL))
    assert one.r2 is None and one.rmse == pytest.approx(abs(y[0] - sums[0, 2] / sums[0, 0]), rel=1e-13)
    sums, y = synthetic_sums(lr.BERNOULLI, 6, 4)
    for value in (0.0, 1.0):
        only = diagnostics.loo_predictive_summary(sums, np.full(6, value), lr.BERNOULLI)
        same(only, lr.summary(sums, np.full(6, value), lr.BERNOULLI))
        assert only.balanced_accuracy is None and only.accuracy is not None and only.brier is not None
    # two observations, one of each class, one right and one wrong
    two = np.array([[1.0, 1.0, 0.9, 0.9, 0.5, 1.0], [1.0, 1.0, 0.8, 0.8, 0.5, 1.0]])
    s = diagnostics.loo_predictive_summary(two, [1.0, 0.0], lr.BERNOULLI)
    assert s.accuracy == 0.5 and s.balanced_accuracy == 0.5 and s.brier == pytest.approx(0.5 * (0.01 + 0.64))
    assert np.allclose(s.loo_sd, np.sqrt([0.9 - 0.81, 0.8 - 0.64])) and np.array_equal(s.is_ess, [1.0, 1.0])


def test_one_calibration_definition_for_the_posterior_and_the_loo_pit():
    """ppc_pit_ks / ppc_coverage_90 and loo_pit_ks / loo_coverage_90 are one helper on two inputs: the same PIT values
    through ppc_from_counts and through loo_predictive_summary give the same two floats."""
    from autoreparam_amd import diagnostics
    rs = np.random.RandomState(8)
    N, R = 50, 64
    pit = rs.rand(N) ** 1.3
    y = rs.randn(N)
    obs4 = np.stack([np.zeros(N), np.full(N, float(R)), pit * R, np.zeros(N)], axis=1)
    counts = np.zeros(diagnostics.PPC_COUNTS)
    counts[0] = R
    ppc = diagnostics.ppc_from_counts(counts, obs4, y, lr.NORMAL)
    sums6 = np.stack([np.full(N, float(R)), np.full(N, float(R)), np.zeros(N), np.full(N, float(R)), pit * R, np.full(N, float(R))], axis=1)
    loo = diagnostics.loo_predictive_summary(sums6, y, lr.NORMAL)
    assert np.array_equal(ppc.pit, loo.loo_pit)
    assert (ppc.pit_ks, ppc.coverage_90) == (loo.pit_ks, loo.coverage_90) == diagnostics._pit_calibration(ppc.pit)
    ref = lr.summary(sums6, y, lr.NORMAL)
    assert loo.pit_ks == pytest.approx(ref["pit_ks"], rel=1e-13) and loo.coverage_90 == pytest.approx(ref["coverage_90"], rel=1e-13)


def test_the_reference_weights_are_psis_rows_in_draw_order():
    """loopred_ref.psis_log_weights against psis_ref.psis_row: sorted, they are its `lws`, hence its elpd_loo; a tie group
    across the cut-off is split by draw index; masked draws take -inf; a non-finite row is NaN."""
    import psis_ref as pr
    from scipy.special import logsumexp
    rs = np.random.RandomState(4)
    ll = (-1.0 - rs.gamma(2.0, 1.0, size=(3, 700))).astype(np.float32)
    ll[1, ::3] = ll[1, 0]                                                   # many ties
    mask = (rs.rand(700) < 0.1).astype(np.uint8)
    lw = lr.psis_log_weights(ll, mask)
    keep = mask == 0
    assert np.all(lw[:, ~keep] == -np.inf) and np.isfinite(lw[:, keep]).all() and lw[:, keep].max() <= 0.0
    for n in range(3):
        row = ll[n, keep].astype(np.float64)
        out = pr.psis_row(row)
        elpd = logsumexp(lw[n, keep] + row) - logsumexp(lw[n, keep])
        assert elpd == pytest.approx(out[0], rel=1e-12)
        M = int(out[4])
        order = np.argsort(row, kind="stable")
        tail, rest = order[:M], order[M:]
        assert np.array_equal(lw[n, keep][rest], row.min() - row[rest])          # raw outside the tail
        assert np.all(np.diff(lw[n, keep][tail]) <= 0.0)                          # descending along the stable order
    ll[2, 5] = np.nan
    assert np.isnan(lr.psis_log_weights(ll)[2]).all() and np.isfinite(lr.psis_log_weights(ll)[:2]).all()
    few = lr.psis_log_weights(ll[:1, :20])                                        # M = 4: not fitted, raw weights
    assert np.array_equal(few[0], ll[0, :20].astype(np.float64).min() - ll[0, :20].astype(np.float64))


def test_keys_flag_and_refusals():
    from autoreparam_amd import diagnostics, main
    from autoreparam_amd.flags import FlagValues
    assert main.LOO_PRED_KEYS == ("loo_pred_observations", "loo_pred_observations_left_out", "loo_pit_ks", "loo_coverage_90",
                                  "loo_rmse", "loo_r2", "loo_brier", "loo_accuracy", "loo_balanced_accuracy", "loo_is_ess_min",
                                  "loo_is_ess_min_observation", "loo_pred_time_sec")
    assert not set(main.LOO_PRED_KEYS) & set(main.LOO_KEYS) and "loo_time_sec" in main.LOO_KEYS
    assert diagnostics.LOO_PRED_COLUMNS == lr.COLUMNS and len(diagnostics.LOO_PRED_COLUMNS) == 6
    for kind in (lr.NORMAL, lr.BERNOULLI):
        sums, y = synthetic_sums(kind, 9, 1)
        keys = main.loo_pred_keys(diagnostics.loo_predictive_summary(sums, y, kind))
        assert tuple(keys) + ("loo_pred_time_sec",) == main.LOO_PRED_KEYS
        nulls = {k for k, v in keys.items() if v is None}
        assert nulls == ({"loo_brier", "loo_accuracy", "loo_balanced_accuracy"} if kind == lr.NORMAL else
                         {"loo_pit_ks", "loo_coverage_90", "loo_rmse", "loo_r2"})
    empty = main.loo_pred_keys(diagnostics.loo_predictive_summary(np.zeros((3, 6)), np.zeros(3), lr.NORMAL))
    assert empty["loo_pred_observations"] == 0 and empty["loo_pred_observations_left_out"] == 3
    assert empty["loo_is_ess_min"] is None and empty["loo_is_ess_min_observation"] is None
    f = FlagValues()
    assert f.loo_predictive is False
    f.parse(["--loo_predictive", "--model=radon"])
    assert f.loo_predictive is True
    with pytest.raises(ValueError, match="--loo_predictive: --predictive_diagnostics is required"):
        main.check_predictive(f)
    with pytest.raises(ValueError, match="--predictive_diagnostics is required"):
        main.main([], flags=f)                                             # before the model is loaded or anything runs
    f.parse(["--predictive_diagnostics"])
    main.check_predictive(f)
    f.parse(["--model=neals_funnel"])
    with pytest.raises(ValueError, match="neals_funnel has no observations"):
        main.main([], flags=f)
    f.parse(["--noloo_predictive", "--nopredictive_diagnostics"])
    main.check_predictive(f)


def test_null_report_carries_the_new_keys_as_null(monkeypatch, capsys):
    from autoreparam_amd import diagnostics, main, models, parallel
    from autoreparam_amd.flags import FlagValues

    def never(*a, **k):
        raise AssertionError("the device functions must not be called")
    for name in ("pointwise_loglik", "psis_loo", "psis_weights", "loo_predictive"):
        monkeypatch.setattr(diagnostics, name, never)
    f = FlagValues()
    f.parse(["--predictive_diagnostics", "--loo_predictive"])
    spec = models._spec_eight_schools()
    both = main.LOO_KEYS + main.LOO_PRED_KEYS
    side = {}
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    keys, arrays = main._loo_report(None, torch.zeros(4, 3, spec.D), 3, spec, f, side)
    assert arrays is None and side == {} and tuple(keys) == both and all(v is None for v in keys.values())
    text = capsys.readouterr().out
    assert text.count("not computed") == 1 and "LOO predictive" not in text        # one message, none of its own
    monkeypatch.setattr(parallel, "world", lambda: (0, 1))
    keys, arrays = main._loo_report(None, torch.zeros(4, 0, spec.D), 0, spec, f, side)
    assert arrays is None and side == {} and tuple(keys) == both and all(v is None for v in keys.values())
    keys, arrays = main._loo_report(None, torch.zeros(4, 2, 300), 2, spec, f, side)
    assert arrays is None and tuple(keys) == both and all(v is None for v in keys.values())
    assert capsys.readouterr().out.count("not computed") == 2

    class Results(object):
        trace = None
    cfg = type("Cfg", (), {"model": spec})()
    keys, arrays = main._convergence_report(Results(), cfg, f, None)
    assert arrays is None and tuple(keys) == both and all(v is None for v in keys.values())
    f.parse(["--predictive_checks"])
    keys, arrays = main._convergence_report(Results(), cfg, f, None)
    assert tuple(keys) == both + main.PPC_KEYS and all(v is None for v in keys.values())
    f.parse(["--noloo_predictive", "--nopredictive_checks"])
    keys, _ = main._convergence_report(Results(), cfg, f, None)
    assert tuple(keys) == main.LOO_KEYS                                   # as before without the flag


def test_side_file_under_its_own_tag(tmp_path):
    from autoreparam_amd import main
    assert main.LOO_PRED_ARRAYS not in (main.LOO_ARRAYS, main.PPC_ARRAYS) and main.LOO_PRED_ARRAYS.endswith("/")
    arrays = {"split_rhat/x": np.ones(3),
              main.LOO_ARRAYS: {"elpd_loo_i": np.zeros(2), "model": np.asarray("m")},
              main.LOO_PRED_ARRAYS: {"loo_mean": np.arange(2.0), "loo_sd": np.ones(2), "loo_pit": np.full(2, 0.5),
                                     "loo_is_ess": np.full(2, 7.0), "y": np.zeros(2, np.float32), "model": np.asarray("m")}}
    base = str(tmp_path / "CP_tied")
    main._save_diagnostics(base, arrays)
    z = np.load(base + "_loopred.npz")
    assert sorted(z.files) == ["loo_is_ess", "loo_mean", "loo_pit", "loo_sd", "model", "y"] and np.array_equal(z["loo_mean"], [0.0, 1.0])
    assert np.load(base + "_rhat.npz").files == ["split_rhat/x"] and np.load(base + "_loo.npz").files == ["elpd_loo_i", "model"]
    main._save_diagnostics(str(tmp_path / "NCP_tied"), {"split_rhat/x": np.ones(3)})
    assert not (tmp_path / "NCP_tied_loopred.npz").exists()


LOO_RUN = {"loo_draws": 8192, "loo_draws_left_out": 0, "loo_chains": 256, "loo_steps": 32, "loo_observations": 919,
           "elpd_loo": -1036.2, "elpd_loo_se": 28.1, "p_loo": 31.4, "elpd_waic": -1036.1, "elpd_waic_se": 28.1, "p_waic": 31.2,
           "pareto_k_max": 0.41, "pareto_k_max_observation": 17, "pareto_k_threshold": 0.7, "pareto_k_above_threshold": 0,
           "loo_nonfinite_observations": 0, "loo_time_sec": 0.5}
PRED_NORMAL = {"loo_pred_observations": 919, "loo_pred_observations_left_out": 0, "loo_pit_ks": 0.0312, "loo_coverage_90": 0.8912,
               "loo_rmse": 0.7654, "loo_r2": 0.1234, "loo_brier": None, "loo_accuracy": None, "loo_balanced_accuracy": None,
               "loo_is_ess_min": 1234.5, "loo_is_ess_min_observation": 17, "loo_pred_time_sec": 0.125}
PRED_BERNOULLI = dict(PRED_NORMAL, loo_pit_ks=None, loo_coverage_90=None, loo_rmse=None, loo_r2=None, loo_brier=0.1777,
                      loo_accuracy=0.7431, loo_balanced_accuracy=0.6543)


def test_analyze_prints_the_line_when_the_keys_are_there(tmp_path, capsys):
    from autoreparam_amd import analyze, main
    assert set(LOO_RUN) == set(main.LOO_KEYS) and set(PRED_NORMAL) == set(main.LOO_PRED_KEYS)
    d = tmp_path / "radon_MN"
    d.mkdir()
    lists = lambda run: {k: [v] for k, v in run.items()}
    ppc = {"ppc_observations": 919, "ppc_pit_ks": 0.0205, "ppc_coverage_90": 0.9021}
    (d / "CP_tied.json").write_text(json.dumps(lists(dict(LOO_RUN, **PRED_NORMAL))))                 # flagged, no PPC keys
    (d / "NCP_tied.json").write_text(json.dumps(lists(LOO_RUN)))                                     # not flagged
    (d / "cVIP_eig_tied.json").write_text(json.dumps(lists(dict(LOO_RUN, **dict(PRED_NORMAL, **ppc)))))      # both reports
    (d / "dVIP_eig_tied.json").write_text(json.dumps(lists(dict(LOO_RUN, **PRED_BERNOULLI))))
    (d / "i_tied.json").write_text(json.dumps(lists({k: None for k in main.LOO_KEYS + main.LOO_PRED_KEYS})))   # null report
    analyze.main(["--results_dir", str(tmp_path), "--model", "radon_MN", "--loo"])
    out = capsys.readouterr().out.splitlines()

    def block(method):
        at = [i for i, l in enumerate(out) if l.startswith(method + ":")]
        assert len(at) == 1, method
        nxt = out[at[0] + 1] if at[0] + 1 < len(out) else ""
        return out[at[0]], nxt if nxt.startswith("      LOO predictive:") else None
    head, line = block("CP_tied")
    assert "elpd_loo -1036" in head and line is not None
    assert "LOO-PIT Kolmogorov distance 0.0312," in line and "90 % coverage 0.8912," in line and "RMSE 0.7654" in line
    assert "R^2 0.1234" in line and "Brier" not in line and "accuracy" not in line and "posterior" not in line
    assert "919 observations, 0 left out" in line and "ESS 1234 (observation 17)" in line and "0.125s" in line
    assert block("NCP_tied")[1] is None and "elpd_loo -1036" in block("NCP_tied")[0]
    both = block("cVIP_eig_tied")[1]
    assert "LOO-PIT Kolmogorov distance 0.0312 (posterior 0.0205)" in both and "90 % coverage 0.8912 (posterior 0.9021)" in both
    bern = block("dVIP_eig_tied")[1]
    assert "Brier score 0.1777, accuracy 0.7431, balanced accuracy 0.6543" in bern and "LOO-PIT" not in bern and "RMSE" not in bern
    assert block("i_tied") == ("i_tied: PSIS-LOO / WAIC not computed", None)
    assert sum(1 for l in out if "LOO predictive:" in l) == 3
