"""CPU: the host half of the predictive report -- the float64 definition tests/psis_ref.py against a closed-form
leave-one-out density, the tail-length rule, ModelSpec.observation_table against the per-model restatements of
tests/loglik_ref.py, diagnostics.loo_summary / loo_compare, the flags, the funnel refusal and the null keys."""
import math

import numpy as np
import pytest
import torch

import loglik_ref as lr
import psis_ref as pr

TABLE_SPECS = {
    "8schools": lambda m: m._spec_eight_schools(), "radon": lambda m: m._spec_radon("MN"),
    "radon_stddvs": lambda m: m._spec_radon_stddvs("MN"), "german_credit_lognormalcentered": lambda m: m._spec_german(),
    "german_credit_gammascale": lambda m: m._spec_german_gammascale(), "election": lambda m: m._spec_election(),
    "electric": lambda m: m._spec_electric(), "time_series": lambda m: m._spec_time_series()}
TERMS = {"8schools": 1, "radon": 2, "radon_stddvs": 2, "german_credit_lognormalcentered": None,
         "german_credit_gammascale": None, "election": 3, "electric": 2, "time_series": 2}


def table_predictor(table, x):
    """(eta, s) [R, N] in float64 from an observation table and centred states x [R, D]."""
    x = np.asarray(x, np.float64)
    eta = np.einsum("nt,rnt->rn", table.w.astype(np.float64), x[:, table.idx])
    s = np.broadcast_to(table.log_scale.astype(np.float64), eta.shape).copy()
    on = table.scale_idx >= 0
    s[:, on] += x[:, table.scale_idx[on]]
    return eta, s


def test_reference_matches_the_closed_form_leave_one_out_density():
    """y_n ~ N(theta, 1), flat prior: theta | y ~ N(ybar, 1 / 20) and p(y_n | y_-n) = N(y_n; ybar_-n, 1 + 1 / 19).  The
    definition must be within 1e-2 of it for every observation (Monte-Carlo error of 65 536 draws included)."""
    rs = np.random.RandomState(1)
    y = 0.3 + rs.randn(20)
    theta = y.mean() + rs.randn(65536) / math.sqrt(20.0)
    ll = (-0.5 * (y[:, None] - theta[None, :]) ** 2 - lr.HALF_LOG_2PI).astype(np.float32)
    out = pr.psis_loo(ll)
    v = 1.0 + 1.0 / 19.0
    for n in range(20):
        m = (y.sum() - y[n]) / 19.0
        exact = -0.5 * (y[n] - m) ** 2 / v - 0.5 * math.log(2.0 * math.pi * v)
        assert abs(out[n, 0] - exact) <= 1e-2, (n, out[n, 0], exact)
        assert np.isfinite(out[n, 1]) and out[n, 1] < 0.5
    assert np.array_equal(out[:, 4], np.full(20, 768.0)) and np.array_equal(out[:, 7], np.full(20, 65536.0))


@pytest.mark.parametrize("R, M", [(24, 4), (25, 5), (225, 45), (226, 45), (4096, 192), (65536, 768)])
def test_tail_lengths(R, M):
    assert pr.tail_len(R) == M
    ll =np.random.RandomState(R).randn(1, R).astype(np.float32)
    out = pr.psis_loo(ll)
    assert out[0, 4] == M and (np.isinf(out[0, 1]) if M < 5 else np.isfinite(out[0, 1]))


def test_reference_ignores_which_tied_draw_is_in_the_tail():
    rs = np.random.RandomState(3)
    base = (-np.abs(rs.randn(100))).astype(np.float32)
    ll = np.repeat(base, 3)[None, :]               # R = 300, M = 52: the cut-off splits a group of three
    a = pr.psis_loo(ll)
    b = pr.psis_loo(ll[:, rs.permutation(300)])
    assert np.array_equal(a[:, 4:6], b[:, 4:6]) and np.allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", sorted(TABLE_SPECS))
def test_observation_table_matches_the_model_programs(name):
    """sum_t w x and s from the table, in float64, equal loglik_ref's predictor and log-scale on random centred states:
    products of float32 data with float64 states are exact on both sides; the sums differ by their order only."""
    from autoreparam_amd import models
    spec = TABLE_SPECS[name](models)
    t = spec.observation_table()
    N = np.asarray(spec.raw["y"]).size
    T = TERMS[name] if TERMS[name] is not None else spec.raw["X"].shape[1]
    assert t.idx.shape == (N, T) and t.w.shape == (N, T) and t.idx.dtype == np.int32 and t.w.dtype == np.float32
    assert t.y.shape == (N,) and t.scale_idx.shape == (N,) and t.log_scale.shape == (N,)
    assert t.scale_idx.dtype == np.int32 and t.log_scale.dtype == np.float32 and t.y.dtype == np.float32
    assert t.idx.min() >= 0 and t.idx.max() < spec.D and t.scale_idx.min() >= -1 and t.scale_idx.max() < spec.D
    assert np.all(t.idx[t.w == 0] == 0)
    x = 0.5 * np.random.RandomState(7).randn(16, spec.D)
    kind, eta, s, y = lr.predictor(spec, x)
    assert t.kind == kind and np.array_equal(t.y.astype(np.float64), y)
    eta_t, s_t = table_predictor(t, x)
    scale = np.einsum("nt,rnt->rn", np.abs(t.w.astype(np.float64)), np.abs(x[:, t.idx]))
    assert np.all(np.abs(eta_t - eta) <= 2.0 ** -50 * T * (scale + 1e-300)), name
    assert np.all(np.abs(s_t - s) <= 2.0 ** -24 * np.abs(s) + 2.0 ** -50), name        # (log_scale is stored as float32)


def test_one_hot_quirk_rows_are_restated():
    """The reference feeds 1-based indices to tf.one_hot: the highest state / pair / grade is an all-zero row.  Those
    observations are in the real data, and the table gives them a zero weight and, for electric's grade, no scale latent."""
    from autoreparam_amd import models
    el = models._spec_election()
    t = el.observation_table()
    out = np.asarray(el.raw["state"]).reshape(-1) >= int(el.raw["n_state"])
    assert out.any() and np.all(t.w[out, 0] == 0) and np.all(t.w[~out, 0] == 1)
    ec = models._spec_electric()
    t = ec.observation_table()
    pair_out = np.asarray(ec.raw["pair"]).reshape(-1) >= int(ec.raw["n_pair"])
    grade_out = np.asarray(ec.raw["grade"]).reshape(-1) >= int(ec.raw["n_grade"])
    assert pair_out.any() and grade_out.any()
    assert np.all(t.w[pair_out, 0] == 0) and np.all(t.w[grade_out, 1] == 0)
    assert np.all(t.scale_idx[grade_out] == -1) and np.all(t.log_scale[grade_out] == 0) and np.all(t.scale_idx[~grade_out] >= 0)


def test_funnel_has_no_table_and_radon_stddvs_refuses_like_its_builder():
    from autoreparam_amd import models
    assert models._spec_funnel().observation_table() is None
    sp = models._spec_radon_stddvs("MN")
    sp.raw = dict(sp.raw)
    county = np.array(sp.raw["county"]).copy()
    county[3] = len(sp.raw["u"])
    sp.raw["county"] = county
    with pytest.raises(ValueError, match="radon_stddvs: county index out of range"):
        sp.observation_table()
    # plain radon takes the same data: an all-zero one-hot row, the observation only informs b2
    rd = models._spec_radon("MN")
    rd.raw = dict(rd.raw, county=county)
    t = rd.observation_table()
    assert t.w[3, 0] == 0 and t.idx[3, 0] == 0 and np.all(np.delete(t.w[:, 0], 3) == 1)


def test_loo_summary_and_compare_on_hand_made_columns():
    from autoreparam_amd import diagnostics
    e = np.array([-1.0, -2.0, -4.0])
    l = np.array([-0.5, -1.5, -3.0])
    p = np.array([0.25, 0.5, 0.75])
    s = diagnostics.loo_summary(e, l, p)
    assert s.elpd_loo == -7.0 and s.p_loo == 2.0 and s.p_waic == 1.5 and s.elpd_waic == -6.5
    assert s.elpd_loo_se == pytest.approx(math.sqrt(3 * np.var(e, ddof=1)), rel=1e-15)
    assert s.elpd_waic_se == pytest.approx(math.sqrt(3 * np.var(l - p, ddof=1)), rel=1e-15)
    ref = pr.summary(e, l, p)
    assert all(getattr(s, key) == pytest.approx(ref[key], rel=1e-15) for key in ref)
    assert diagnostics.loo_summary([-1.0, -np.inf], [0.0, 0.0], [0.0, 0.0]).elpd_loo == -np.inf     # carried, not skipped
    y = np.array([1.0, 0.0, 1.0], np.float32)
    a, b = {"elpd_loo_i": e, "y": y}, {"elpd_loo_i": e + np.array([0.5, -0.25, 1.0]), "y": y.copy()}
    diff, se = diagnostics.loo_compare(a, b)
    d = -np.array([0.5, -0.25, 1.0])
    assert diff == pytest.approx(d.sum()) and se == pytest.approx(math.sqrt(3 * np.var(d, ddof=1)))
    assert (diff, se) == pytest.approx(pr.compare(a["elpd_loo_i"], b["elpd_loo_i"]))
    with pytest.raises(ValueError, match="same observations"):
        diagnostics.loo_compare(a, {"elpd_loo_i": e, "y": np.array([1.0, 1.0, 1.0])})
    with pytest.raises(ValueError, match="different numbers"):
        diagnostics.loo_compare(a, {"elpd_loo_i": e[:2], "y": y[:2]})
    assert diagnostics.pareto_k_threshold(65536) == 0.7 and diagnostics.pareto_k_threshold(100) == 0.5
    assert diagnostics.pareto_k_threshold(1000) == pytest.approx(pr.k_threshold(1000)) and math.isnan(diagnostics.pareto_k_threshold(1))


def test_keys_fold_the_columns():
    from autoreparam_amd import main
    rs = np.random.RandomState(5)
    c = np.zeros((6, 8))
    c[:, 0], c[:, 2], c[:, 3] = -rs.rand(6) - 1.0, -rs.rand(6), rs.rand(6)
    c[:, 1] = [0.1, 0.9, np.inf, 0.3, 0.71, -0.2]
    keys = main.loo_keys(c, R=1000, left_out=10, n_chains=99, n_steps=10)
    ref = pr.summary(c[:, 0], c[:, 2], c[:, 3])
    assert all(keys[key] == pytest.approx(ref[key], rel=1e-14) for key in ref)
    assert keys["loo_draws"] == 990 and keys["loo_draws_left_out"] == 10 and keys["loo_chains"] == 99 and keys["loo_steps"] == 10
    assert keys["loo_observations"] == 6 and keys["pareto_k_max"] == 0.9 and keys["pareto_k_max_observation"] == 1
    assert keys["pareto_k_threshold"] == pytest.approx(1.0 - 1.0 / math.log10(990)) and keys["pareto_k_above_threshold"] == 3
    assert keys["loo_nonfinite_observations"] == 0
    c[4, 0] = -np.inf
    keys = main.loo_keys(c, R=1000, left_out=0, n_chains=100, n_steps=10)
    assert keys["elpd_loo"] is None and keys["loo_nonfinite_observations"] == 1 and keys["elpd_waic"] is not None
    assert set(keys) | {"loo_time_sec"} == set(main.LOO_KEYS)


def test_steps_and_tiles():
    from autoreparam_amd import main
    assert main.loo_steps(1000, 65536, 65536) == [999]                     # one step: the last
    assert main.loo_steps(1000, 100000, 65536) == [999]                    # never fewer than one
    s = main.loo_steps(1000, 256, 65536)
    assert len(s) == 256 and s[0] == 0 and s[-1] == 999
    assert main.loo_steps(10, 256, 65536) == list(range(10))               # never more than were recorded
    assert len(main.loo_steps(100, 1 << 20, 1 << 30)) == 16                # never more draws than the fit takes
    assert main.loo_tile_rows(11566, 65536) == 1024 and main.loo_tile_rows(8, 65536) == 8 and main.loo_tile_rows(5, 1 << 30) == 1


def test_flags_and_the_funnel_refusal():
    from autoreparam_amd import main
    from autoreparam_amd.flags import FlagValues
    f = FlagValues()
    assert f.predictive_diagnostics is False and f.loo_draws == 65536
    f.parse(["--predictive_diagnostics", "--loo_draws=4096", "--model=radon"])
    assert f.predictive_diagnostics is True and f.loo_draws == 4096
    main.check_predictive(f)
    f.parse(["--model=neals_funnel"])
    with pytest.raises(ValueError, match="neals_funnel has no observations"):
        main.check_predictive(f)
    with pytest.raises(ValueError, match="neals_funnel has no observations"):
        main.main([], flags=f)                                             # before the model is loaded or anything runs
    f.parse(["--nopredictive_diagnostics"])
    main.check_predictive(f)


def test_sharded_job_and_missing_trace_write_null_keys(monkeypatch, capsys):
    from autoreparam_amd import diagnostics, main, models, parallel
    from autoreparam_amd.flags import FlagValues

    def never(*a, **k):
        raise AssertionError("the device functions must not be called")
    monkeypatch.setattr(diagnostics, "pointwise_loglik", never)
    monkeypatch.setattr(diagnostics, "psis_loo", never)
    f = FlagValues()
    f.parse(["--predictive_diagnostics"])
    spec = models._spec_eight_schools()
    trace = torch.zeros(4, 3, spec.D)
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    keys, arrays = main._loo_report(None, trace, 3, spec, f)
    assert arrays is None and tuple(keys) == main.LOO_KEYS and all(v is None for v in keys.values())
    assert capsys.readouterr().out.count("PSIS-LOO / WAIC: not computed") == 1
    monkeypatch.setattr(parallel, "world", lambda: (0, 1))
    keys, arrays = main._loo_report(None, torch.zeros(4, 0, spec.D), 0, spec, f)
    assert arrays is None and tuple(keys) == main.LOO_KEYS and all(v is None for v in keys.values())
    assert capsys.readouterr().out.count("no chain has its trace on the device") == 1

    class Results(object):
        trace = None
    cfg = type("Cfg", (), {"model": spec})()
    keys, arrays = main._convergence_report(Results(), cfg, f, None)
    assert arrays is None and tuple(keys) == main.LOO_KEYS and all(v is None for v in keys.values())
    f.parse(["--nopredictive_diagnostics"])
    assert main._convergence_report(Results(), cfg, f, None) == ({}, None)          # as before without the flag
