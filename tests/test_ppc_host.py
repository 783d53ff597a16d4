"""CPU: the host half of the posterior predictive checks -- the flag, the two ABI entries, diagnostics.ppc_summary and
combine_draw_stats on hand-made columns, the additivity over draws that the sharded report rests on, analyze --ppc, the
refusal for a model without data, the null keys, and the Philox restatement of tests/ppc_ref.py against its known answers."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import ppc_ref as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("arp_predictive_check", "arp_predictive_workspace_bytes")


def columns(y_rep, dev_rep, dev_obs, mu):
    """[R, 8] draw statistics of replicated data sets y_rep [N, R], as the kernel folds them."""
    N, R = y_rep.shape
    return np.stack([y_rep.sum(0), (y_rep ** 2).sum(0), y_rep.min(0), y_rep.max(0), dev_rep, dev_obs, mu.sum(0),
                     np.full(R, float(N))], axis=1)


def test_reference_philox_passes_the_known_answers():
    for counter, key, out in pp.KNOWN_ANSWERS:
        assert tuple(int(v) for v in pp.philox4x32_10(counter, key)) == out
    # vectorised over a counter word, as the reference uses it
    got = pp.philox4x32_10((np.array([0, 0x243f6a88], np.uint64), np.array([0, 0x85a308d3], np.uint64),
                            np.array([0, 0x13198a2e], np.uint64), np.array([0, 0x03707344], np.uint64)), (0, 0))
    assert tuple(int(v[0]) for v in got) == pp.KNOWN_ANSWERS[0][2]
    w0, w1 = pp.words(np.arange(3, dtype=np.uint64)[:, None], np.arange(5, dtype=np.uint64)[None, :] + np.uint64(1 << 33), 7)
    assert w0.shape == (3, 5) and len(np.unique(w0)) == 15
    one = pp.philox4x32_10((2, 4, 2, 0), (7, 0))                       # g = 2^33 + 4: lo 4, hi 2
    assert int(w0[2, 4]) == int(one[0]) and int(w1[2, 4]) == int(one[1])


def test_reference_uniform_and_normal_inputs():
    assert pp.uniform(0) == 0.0 and pp.uniform(0xFFFFFFFF) == 1.0 - 2.0 ** -24 and pp.uniform(0x100) == 2.0 ** -24
    up, a = pp.normal_inputs(np.array([0, 0xFFFFFFFF, 1 << 31], np.uint64), np.array([0, 0x7FFFFF, 0xFF800000], np.uint64))
    assert up[0] == 2.0 ** -33 and up[1] == 1.0 and up[2] == np.float32(0.5 + 2.0 ** -33)
    assert a[0] == 1.0 and a[1] == 2.0 - 2.0 ** -23 and a[2] == 1.0
    z = pp.normal(np.arange(1, 200001, dtype=np.uint64) * np.uint64(21473), np.arange(200000, dtype=np.uint64) * np.uint64(7919))
    assert np.isfinite(z).all() and abs(z.std() - 1.0) < 0.02 and abs(z.mean()) < 0.02


def test_flag_header_and_symbols():
    from autoreparam_amd import _lib, main
    from autoreparam_amd.flags import FlagValues
    f = FlagValues()
    assert f.predictive_checks is False
    f.parse(["--predictive_checks", "--model=radon"])
    assert f.predictive_checks is True
    main.check_predictive_checks(f)
    src = open(os.path.join(ROOT, "include", "autoreparam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)                      # as tests/test_abi.py reads the header
    declared = sorted(set(re.findall(r"\b(arp_[a-z_0-9]+)\s*\(", src)))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS, name
    assert sorted(declared) == sorted(_lib.SYMBOLS)


def test_funnel_is_refused_before_anything_runs():
    from autoreparam_amd import main
    from autoreparam_amd.flags import FlagValues
    f = FlagValues()
    f.parse(["--predictive_checks", "--model=neals_funnel"])
    with pytest.raises(ValueError, match="--predictive_checks: neals_funnel has no observations"):
        main.check_predictive_checks(f)
    with pytest.raises(ValueError, match="--predictive_checks: neals_funnel has no observations"):
        main.main([], flags=f)
    main.check_predictive(f)                                            # the other report's rule is its own
    f.parse(["--nopredictive_checks"])
    main.check_predictive_checks(f)


def test_p_values_always_above_always_below_and_ties():
    from autoreparam_amd import diagnostics
    y = np.array([1.0, 2.0, 3.0, 6.0])                                   # mean 3, min 1, max 6
    R = 5
    above = np.tile(y[:, None] + 10.0, (1, R))
    s = diagnostics.ppc_summary(columns(above, np.full(R, 9.0), np.full(R, 1.0), above), np.zeros((4, 4)), y, 0)
    assert s.p["mean"] == 1.0 and s.p["min"] == 1.0 and s.p["max"] == 1.0 and s.p["deviance"] == 1.0
    assert s.p["sd"] == 1.0                                              # the same spread exactly: a tie counts as >=
    below = np.tile(0.5 * y[:, None] - 10.0, (1, R))
    s = diagnostics.ppc_summary(columns(below, np.full(R, 1.0), np.full(R, 9.0), below), np.zeros((4, 4)), y, 0)
    assert all(s.p[k] == 0.0 for k in diagnostics.PPC_STATISTICS)
    # ties: the replicated data ARE the data in draws 0 and 2, below in the others; equal deviances in draw 1
    mixed = below.copy()
    mixed[:, 0] = mixed[:, 2] = y
    s = diagnostics.ppc_summary(columns(mixed, np.array([1.0, 4.0, 1.0, 1.0, 1.0]), np.full(R, 4.0), mixed), np.zeros((4, 4)), y, 0)
    assert s.p["mean"] == 0.4 and s.p["sd"] == 0.4 and s.p["min"] == 0.4 and s.p["max"] == 0.4 and s.p["deviance"] == 0.2
    assert s.draws_used == 5 and s.draws_left_out == 0 and s.observations == 4
    assert s.obs["mean"] == 3.0 and s.obs["min"] == 1.0 and s.obs["max"] == 6.0 and s.obs["deviance"] == 4.0
    assert s.rep["mean"] == pytest.approx(mixed.mean(0).mean(), rel=1e-15)


def test_sd_uses_divisor_n_minus_one():
    from autoreparam_amd import diagnostics
    y = np.array([0.0, 2.0, 4.0, 10.0])
    assert diagnostics.ppc_summary(columns(y[:, None], np.zeros(1), np.zeros(1), y[:, None]), np.zeros((4, 4)), y, 0).obs["sd"] \
        == pytest.approx(math.sqrt(((y - 4.0) ** 2).sum() / 3.0), rel=1e-15)
    rep = np.array([[0.0], [0.0], [3.0], [3.0]])                          # sd with N - 1: sqrt(3); with N: 1.5
    s = diagnostics.ppc_summary(columns(rep, np.zeros(1), np.zeros(1), rep), np.zeros((4, 4)), y, 0)
    assert s.rep["sd"] == pytest.approx(math.sqrt(3.0), rel=1e-15)
    y2 = np.array([0.0, 0.0, 3.4, 3.4])                                   # sd(y2) = 1.963 with N - 1: above sqrt(3); 1.7 with N
    s = diagnostics.ppc_summary(columns(rep, np.zeros(1), np.zeros(1), rep), np.zeros((4, 4)), y2, 0)
    assert s.p["sd"] == 0.0 and s.obs["sd"] == pytest.approx(np.std(y2, ddof=1), rel=1e-15)


def test_masked_draws_are_not_counted():
    from autoreparam_amd import diagnostics
    y = np.array([1.0, 2.0, 3.0])
    rep = np.stack([y + 1.0, y - 1.0, np.zeros(3), y + 2.0], axis=1)
    c = columns(rep, np.array([5.0, 1.0, 0.0, 5.0]), np.array([2.0, 2.0, 0.0, 2.0]), rep)
    c[2] = 0.0                                                          # the kernel's row of a draw left out
    mask = np.array([0, 0, 1, 0], np.uint8)
    obs = np.array([[6.0, 30.0, 1.5, 2.0], [9.0, 60.0, 1.2, 1.0], [12.0, 90.0, 2.7, 3.0]])
    s = diagnostics.ppc_summary(c, obs, y, 0, mask)
    assert s.draws_used == 3 and s.draws_left_out == 1
    assert s.p["mean"] == pytest.approx(2.0 / 3.0) and s.p["deviance"] == pytest.approx(2.0 / 3.0)
    assert np.allclose(s.predictive_mean, [2.0, 3.0, 4.0], rtol=1e-15)
    assert np.allclose(s.predictive_sd, np.sqrt([10.0 - 4.0, 20.0 - 9.0, 30.0 - 16.0]), rtol=1e-14)
    assert np.allclose(s.pit, [0.5, 0.4, 0.9], rtol=1e-15) and np.allclose(s.rep_le_obs, [2.0 / 3.0, 1.0 / 3.0, 1.0], rtol=1e-15)
    # torch tensors are taken as well
    t = diagnostics.ppc_summary(torch.as_tensor(c), torch.as_tensor(obs), y, 0, torch.as_tensor(mask))
    assert t.p == s.p and t.draws_used == 3
    with pytest.raises(ValueError, match="cover all 3 observations"):
        diagnostics.ppc_summary(c, obs, y, 0)                           # the zero row without its mask
    # no draw left at all: nothing is defined, nothing raises
    none = diagnostics.ppc_summary(c, np.zeros((3, 4)), y, 0, np.ones(4, np.uint8))
    assert none.draws_used == 0 and all(v is None for v in none.p.values()) and np.isnan(none.pit).all() and none.pit_ks is None


def test_bernoulli_reports_what_is_defined():
    from autoreparam_amd import diagnostics, main
    y = np.array([1.0, 0.0, 1.0, 1.0])
    rep = np.array([[1.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 0.0]])
    c = columns(rep, np.array([3.0, 5.0]), np.array([4.0, 4.0]), np.full((4, 2), 0.6))
    obs = np.array([[1.2, 1.2, 1.4, 2.0], [1.2, 1.2, 0.4, 1.0], [1.2, 1.2, 1.4, 2.0], [1.2, 1.2, 1.4, 2.0]])
    s = diagnostics.ppc_summary(c, obs, y, 1)
    assert s.p["mean"] == 0.5 and s.p["deviance"] == 0.5
    assert s.p["sd"] is None and s.p["min"] is None and s.p["max"] is None and s.rep["sd"] is None and s.obs["sd"] is None
    assert s.pit_ks is None and s.coverage_90 is None
    assert np.allclose(s.predictive_mean, 0.6) and np.allclose(s.predictive_sd, math.sqrt(0.6 - 0.36))
    keys = main.ppc_keys(s, 2, 1)
    assert set(keys) | {"ppc_time_sec"} == set(main.PPC_KEYS)
    assert [k for k, v in keys.items() if v is None] == ["ppc_p_sd", "ppc_p_min", "ppc_p_max", "ppc_rep_sd", "ppc_obs_sd",
                                                         "ppc_pit_ks", "ppc_coverage_90"]
    json.dumps(keys)


def test_pit_ks_of_a_uniform_grid_and_coverage():
    from autoreparam_amd import diagnostics
    for N in (1, 7, 100):
        pit = np.arange(1, N + 1) / (N + 1.0)
        obs = np.zeros((N, 4))
        obs[:, 2] = 3.0 * pit[::-1]                                     # 3 draws; the order of the observations is free
        y = np.zeros(N)
        s = diagnostics.ppc_summary(columns(np.zeros((N, 3)), np.zeros(3), np.zeros(3), np.zeros((N, 3))), obs, y, 0)
        assert s.pit_ks == pytest.approx(1.0 / (N + 1.0), rel=1e-12)    # max_i i / N - i / (N + 1) = 1 / (N + 1), at i = N
        assert s.coverage_90 == pytest.approx(np.mean((pit >= 0.05) & (pit <= 0.95)))
    obs = np.zeros((4, 4))
    obs[:, 2] = [0.05, 0.95, 0.04, 0.5]
    s = diagnostics.ppc_summary(columns(np.zeros((4, 1)), np.zeros(1), np.zeros(1), np.zeros((4, 1))), obs, np.zeros(4), 0)
    assert s.coverage_90 == 0.75                                        # the ends of [0.05, 0.95] are inside


def random_case(seed, N=9, R=24):
    rs = np.random.RandomState(seed)
    y = rs.randn(N)
    rep = rs.randn(N, R) * 1.3 + 0.1
    mu = rs.randn(N, R)
    dev_rep, dev_obs = rs.rand(R) * 10.0, rs.rand(R) * 10.0
    obs = lambda cols: np.stack([mu[:, cols].sum(1), (mu[:, cols] ** 2 + 1.0).sum(1), rs.rand(N) * len(cols),
                                 (rep[:, cols] <= y[:, None]).sum(1).astype(np.float64)], axis=1)
    return y, rep, mu, dev_rep, dev_obs, obs


def test_combining_two_observation_ranges_gives_the_whole():
    from autoreparam_amd import diagnostics
    y, rep, mu, dev_rep, dev_obs, _ = random_case(1)
    # integers, so that the sums do not depend on their association
    rep, mu = np.round(rep * 8.0), np.round(mu * 8.0)
    dev_a, dev_b = np.round(dev_rep * 3.0), np.round(dev_rep * 5.0)
    whole = columns(rep, dev_a + dev_b, 2.0 * dev_a + dev_b, mu)
    a, b = columns(rep[:4], dev_a, 2.0 * dev_a, mu[:4]), columns(rep[4:], dev_b, dev_b, mu[4:])
    assert np.array_equal(diagnostics.combine_draw_stats(a, b), whole)
    assert np.array_equal(diagnostics.combine_draw_stats(b, a), whole)
    t = diagnostics.combine_draw_stats(torch.as_tensor(a), torch.as_tensor(b))
    assert torch.is_tensor(t) and np.array_equal(t.numpy(), whole)
    with pytest.raises(ValueError, match="one shape"):
        diagnostics.combine_draw_stats(a, b[:3])


def test_counts_add_over_draws_so_a_sharded_job_reports_the_same():
    """The sharding argument: the summary of the summed counts and obs_sums of two halves of the draws (two ranks) equals
    the summary of all draws, masked draws and both kinds of data included."""
    from autoreparam_amd import diagnostics
    for kind in (0, 1):
        y, rep, mu, dev_rep, dev_obs, obs = random_case(2 + kind)
        if kind == 1:
            y, rep = (y > 0).astype(np.float64), (rep > 0).astype(np.float64)
        c = columns(rep, dev_rep, dev_obs, mu)
        mask = np.zeros(24, np.uint8)
        mask[[3, 17, 23]] = 1
        c[mask != 0] = 0.0
        keep = np.flatnonzero(mask == 0)
        left, right = np.arange(10), np.arange(10, 24)
        o_all = obs(keep)
        o_l, o_r = obs(np.intersect1d(keep, left)), obs(np.intersect1d(keep, right))
        o_all[:, 2] = (o_l + o_r)[:, 2]                                  # (the pit sums are random stand-ins: make them add)
        whole = diagnostics.ppc_summary(c, o_all, y, kind, mask)
        counts = diagnostics.ppc_counts(c[left], y, mask[left]) + diagnostics.ppc_counts(c[right], y, mask[right])
        assert np.array_equal(counts[:7], diagnostics.ppc_counts(c, y, mask)[:7])        # the integer counts: exactly
        both = diagnostics.ppc_from_counts(counts, o_l + o_r, y, kind)
        assert both.draws_used == whole.draws_used == 21 and both.draws_left_out == 3
        assert both.p == whole.p and both.obs["mean"] == whole.obs["mean"]
        for name in diagnostics.PPC_STATISTICS:
            assert (both.rep[name] is None) == (whole.rep[name] is None)
            if both.rep[name] is not None:
                assert both.rep[name] == pytest.approx(whole.rep[name], rel=1e-13)
        for a, b in ((both.predictive_mean, whole.predictive_mean), (both.predictive_sd, whole.predictive_sd), (both.pit, whole.pit)):
            assert np.allclose(a, b, rtol=1e-12, atol=0)
        assert np.array_equal(both.rep_le_obs, whole.rep_le_obs)
        # a rank without a device trace adds zeros
        idle = diagnostics.ppc_counts(np.zeros((0, 8)), y, np.zeros(0, np.uint8))
        assert np.array_equal(idle, np.zeros(diagnostics.PPC_COUNTS))


def test_tiles_count_the_workspace_in():
    from autoreparam_amd import main
    ws = lambda rows, R: 40 * rows * R                                   # ten times the log-likelihood matrix
    assert main.loo_tile_rows(11566, 65536) == 1024
    rows = main.ppc_tile_rows(11566, 65536, ws)
    assert rows == 64 and ws(rows, 65536) <= main.LOO_CHUNK_BYTES < ws(2 * rows, 65536)
    assert main.ppc_tile_rows(8, 64, ws) == 8 and main.ppc_tile_rows(5, 1 << 30, ws) == 1


def test_missing_trace_and_wide_models_write_null_keys(monkeypatch, capsys):
    from autoreparam_amd import diagnostics, main, models
    from autoreparam_amd.flags import FlagValues

    def never(*a, **k):
        raise AssertionError("the device function must not be called")
    monkeypatch.setattr(diagnostics, "predictive_check", never)
    f = FlagValues()
    f.parse(["--predictive_checks"])
    spec = models._spec_eight_schools()
    keys, arrays = main._ppc_report(None, torch.zeros(4, 0, spec.D), 0, 0, spec, f, None)
    assert arrays is None and tuple(keys) == main.PPC_KEYS and all(v is None for v in keys.values())
    assert capsys.readouterr().out.count("posterior predictive checks: not computed, no chain has its trace on the device") == 1
    keys, arrays = main._ppc_report(None, torch.zeros(4, 2, 300), 2, 2, spec, f, None)
    assert arrays is None and tuple(keys) == main.PPC_KEYS and all(v is None for v in keys.values())
    assert capsys.readouterr().out.count("more than 255 elements") == 1

    class Results(object):
        trace = None
    cfg = type("Cfg", (), {"model": spec})()
    keys, arrays = main._convergence_report(Results(), cfg, f, None)
    assert arrays is None and tuple(keys) == main.PPC_KEYS and all(v is None for v in keys.values())
    f.parse(["--predictive_diagnostics"])
    keys, arrays = main._convergence_report(Results(), cfg, f, None)
    assert tuple(keys) == main.LOO_KEYS + main.PPC_KEYS and all(v is None for v in keys.values())
    f.parse(["--nopredictive_checks", "--nopredictive_diagnostics"])
    assert main._convergence_report(Results(), cfg, f, None) == ({}, None)          # as before without the flags


def test_analyze_prints_the_report(tmp_path, capsys):
    from autoreparam_amd import analyze, main
    d = tmp_path / "radon_MN"
    d.mkdir()
    run = {"ppc_draws": 8192, "ppc_draws_left_out": 0, "ppc_chains": 256, "ppc_steps": 32, "ppc_observations": 919,
           "ppc_p_mean": 0.48, "ppc_p_sd": 0.52, "ppc_p_min": 0.003, "ppc_p_max": 0.31, "ppc_p_deviance": 0.5,
           "ppc_rep_mean": 1.224, "ppc_rep_sd": 0.81, "ppc_obs_mean": 1.225, "ppc_obs_sd": 0.82, "ppc_pit_ks": 0.021,
           "ppc_coverage_90": 0.9, "ppc_time_sec": 0.25}
    assert set(run) == set(main.PPC_KEYS)
    (d / "CP_tied.json").write_text(json.dumps({k: [None, v] for k, v in run.items()}))
    (d / "NCP_tied.json").write_text(json.dumps({k: [v, None] for k, v in run.items()}))
    (d / "cVIP_eig_tied.json").write_text(json.dumps({"ess_min": [1.0]}))
    analyze.main(["--results_dir", str(tmp_path), "--model", "radon_MN", "--ppc"])
    out = capsys.readouterr().out
    line = [l for l in out.splitlines() if l.startswith("CP_tied:")]
    assert len(line) == 1 and "mean 0.48" in line[0] and "deviance 0.5" in line[0] and "919 observations" in line[0]
    assert "8192 draws of 256 chains" in line[0] and "EXTREME: min" in line[0] and "0.021" in line[0]
    assert "NCP_tied: posterior predictive checks not computed" in out and "cVIP" not in out
    analyze.main(["--results_dir", str(tmp_path), "--model", "radon_MN", "--loo"])
    assert "ppc" not in capsys.readouterr().out and "predictive p-values" not in out.split("NCP_tied")[1]
