"""CPU: the host half of the prior predictive checks -- the float64 restatement of arp_site_prior_draws
(tests/prior_draw_ref.py) against Philox's known answer and the closed-form distributions of its draws, the share of
undecided log-Gamma attempts on the inputs the GPU test uses (the condition that test relies on), the two pure-numpy
summaries on hand-built inputs, the flag with its refusal and its null keys, analyze --prior, and the ABI entry.

The inputs of tests/test_gpu_prior_draws.py are defined here (MODELS, DRAWS, SEED, synthetic_chain, one_element,
rounded) so that both files speak of the same ones."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import prior_draw_ref as pr
from test_site_table_host import SPECS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = sorted(name for name in SPECS if name != "radon_PA")          # the nine models (radon at MN)
DRAWS = 4096
SEED = 0x5EED0123456789AB
UNDECIDED_CAP = 1.0e-3               # of the log-Gamma elements
KS_CRITICAL = 1.95                   # the 0.001 critical value of sqrt(N) times the Kolmogorov distance
SHAPES = (0.5, 1.0, 2.5)


def rounded(table, D):
    """The table as the kernel reads it: diagnostics.upload_site_table's float32-rounded host copy (no GPU needed)"""
    from autoreparam_amd import diagnostics
    return diagnostics.upload_site_table(table, D, "cpu").host


def synthetic_chain(D=255):
    """Element d depends on d - 1 and d - 2 through both its loc and its log-scale; the forms cycle 0, 1, 2 and the
    log-Gamma shapes 0.5, 1, 2.5; weights small enough that s stays within +-20 (an autoregression of weight 0.3 on the
    locs, 0.05 on the log-scales, whose largest parents are log-Gamma draws near -20)."""
    from autoreparam_amd import models
    rs = np.random.RandomState(255)
    d = np.arange(D)
    form = (d % 3).astype(np.int32)
    idx = np.stack([np.maximum(d - 1, 0), np.maximum(d - 2, 0)], axis=1).astype(np.int32)
    loc_w, scale_w = 0.3 * rs.randn(D, 2), 0.05 * rs.randn(D, 2)
    loc_w[0], scale_w[0] = 0.0, 0.0
    loc_w[1, 1], scale_w[1, 1] = 0.0, 0.0
    loc0 = 0.5 * rs.randn(D)
    gamma = np.flatnonzero(form == 2)
    loc0[gamma] = np.asarray(SHAPES)[np.arange(gamma.size) % 3]
    return models.SiteTable(form, idx, loc_w, loc0, idx.copy(), scale_w, 0.3 * rs.randn(D), np.zeros(D), np.zeros(D, np.int32))


def one_element(form, loc0, log_scale0):
    from autoreparam_amd import models
    z2i, z2f = np.zeros((1, 2), np.int32), np.zeros((1, 2))
    return models.SiteTable(np.array([form], np.int32), z2i, z2f, np.array([loc0]), z2i.copy(), z2f.copy(),
                            np.array([log_scale0]), np.zeros(1), np.zeros(1, np.int32))


def gpu_inputs():
    """(name, rounded table) of every table the GPU parity test draws from, at DRAWS draws each"""
    from autoreparam_amd import models
    for name in MODELS:
        spec = SPECS[name](models)
        yield name, rounded(spec.site_table(), spec.D)
    yield "synthetic D=255", rounded(synthetic_chain(255), 255)
    for form, loc0 in ((0, 0.3), (1, -0.2), (2, 0.5)):
        yield "D=1 form %d" % form, rounded(one_element(form, loc0, 0.4), 1)


def kolmogorov(sample, cdf):
    s = np.sort(np.asarray(sample, np.float64))
    F = cdf(s)
    i = np.arange(1, s.size + 1, dtype=np.float64)
    return float(max(np.max(i / s.size - F), np.max(F - (i - 1.0) / s.size)))


erf = np.vectorize(math.erf)
GAMMA_CDF = {0.5: lambda g: erf(np.sqrt(g / 2.0)),
             1.0: lambda g: 1.0 - np.exp(-g / 2.0),
             2.5: lambda g: erf(np.sqrt(g / 2.0)) - np.sqrt(2.0 / np.pi) * np.exp(-g / 2.0) * (np.sqrt(g) + g ** 1.5 / 3.0)}


def test_reference_philox_passes_the_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds"""
    zero = tuple(int(v) for v in pr.philox(0, 0, 0, 0, 0, 0))
    assert zero == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    ones = tuple(int(v) for v in pr.philox(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff))
    assert ones == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    pi = tuple(int(v) for v in pr.philox(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0))
    assert pi == (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    many = pr.philox(3, np.arange(5, dtype=np.uint64), 1, 0, 7, 9)          # vectorised over a counter word
    assert all(int(many[k][4]) == int(pr.philox(3, 4, 1, 0, 7, 9)[k]) for k in range(4))


def test_reference_inputs_are_the_float32_ones():
    up = pr.open_uniform(np.array([0, 0xFFFFFFFF, 1 << 31], np.uint64))
    assert up[0] == 2.0 ** -33 and up[1] == 1.0 and up[2] == np.float32(0.5 + 2.0 ** -33)
    z = pr.standard_normal(np.array([1 << 31], np.uint64), np.array([0xFF800000], np.uint64))      # a = 1: cospi(2) = 1
    assert z[0] == math.sqrt(-2.0 * math.log(float(np.float32(0.5 + 2.0 ** -33))))
    # a quarter and three quarters of a revolution are exact zeros, as cospi's are; the half is exactly -1
    frac = np.array([0.25, 0.75, 0.5, 0.25 + 2.0 ** -23])
    c = pr.cos_revolutions(frac)
    assert c[0] == 0.0 and c[1] == 0.0 and c[2] == -1.0 and abs(c[3] + 2.0 * math.pi * 2.0 ** -23) < 1e-18
    grid = np.arange(1 << 12) / float(1 << 12)
    # (the plain form's own argument 2 pi g is rounded: half an ulp of 6.28 is 4.4e-16, its product and cos round again)
    assert np.max(np.abs(pr.cos_revolutions(grid) - np.cos(2.0 * np.pi * grid))) < 1.5e-15


@pytest.mark.parametrize("shape", SHAPES)
def test_log_gamma_draws_follow_the_gamma_distribution(shape):
    """65 536 draws at rate 0.5: g = exp(x) against the closed-form CDF"""
    N = 65536
    d = pr.draw(rounded(one_element(2, shape, math.log(0.5)), 1), N, SEED, 0)
    assert not d.undrawn.any() and np.isfinite(d.x).all()
    ks = kolmogorov(np.exp(d.x[:, 0]), GAMMA_CDF[shape])
    print("shape %g: Kolmogorov distance %.5f, allowed %.5f" % (shape, ks, KS_CRITICAL / math.sqrt(N)))
    assert ks < KS_CRITICAL / math.sqrt(N)


@pytest.mark.parametrize("form", (0, 1))
def test_normal_draws_standardise_to_the_normal(form):
    N = 65536
    table = rounded(one_element(form, 1.5, -0.7), 1)
    d = pr.draw(table, N, SEED, 0)
    s = float(table.log_scale0[0])
    sigma = math.exp(s) if form == 0 else max(s, 0.0) + math.log1p(math.exp(-abs(s)))
    z = (d.x[:, 0] - float(table.loc0[0])) / sigma
    ks = kolmogorov(z, lambda v: 0.5 * (1.0 + erf(v / math.sqrt(2.0))))
    print("form %d: Kolmogorov distance %.5f, allowed %.5f" % (form, ks, KS_CRITICAL / math.sqrt(N)))
    assert ks < KS_CRITICAL / math.sqrt(N)


def test_offsets_and_teacher_forcing_in_the_reference():
    table = rounded(synthetic_chain(12), 12)
    whole = pr.draw(table, 70, SEED, 0)
    part = pr.draw(table, 5, SEED, 65)
    assert np.array_equal(part.x, whole.x[65:70])
    forced = pr.draw(table, 70, SEED, 0, parents=whole.x)
    assert np.array_equal(forced.x, whole.x)
    far = pr.draw(table, 3, SEED, (1 << 32) + 5)
    assert not np.array_equal(far.x, pr.draw(table, 3, SEED, 5).x)          # hi32 g enters the counter


def test_undecided_share_on_the_gpu_tests_inputs():
    """The condition the GPU parity test relies on: an attempt whose accept margin lies within its float32 error bound
    E_m is rare -- at most 1 in 1 000 log-Gamma elements of every input, by the reference alone."""
    seen = 0
    for name, table in gpu_inputs():
        d = pr.draw(table, DRAWS, SEED, 0)
        gamma = np.asarray(table.form) == pr.LOG_GAMMA
        assert not d.undrawn.any(), name
        if not gamma.any():
            continue
        marks = pr.undecided(table, d)
        assert not marks[:, ~gamma].any()
        share = marks[:, gamma].mean()
        seen += int(gamma.sum()) * DRAWS
        print("%s: %d of %d log-Gamma elements undecided (share %.2g)" % (name, int(marks.sum()), int(gamma.sum()) * DRAWS, share))
        assert share <= UNDECIDED_CAP, (name, share)
        s = d.terms["s"]
        assert np.abs(s[np.isfinite(s)]).max() <= 20.0 or "synthetic" not in name
    assert seen > 0


def test_tainted_follows_the_table():
    table = rounded(synthetic_chain(6), 6)
    marks = np.zeros((2, 6), bool)
    marks[0, 2] = True
    out = pr.tainted(table, marks)
    assert out[0].tolist() == [False, False, True, True, True, True] and not out[1].any()


def columns(y_rep):
    N, R = y_rep.shape
    zero = np.zeros(R)
    return np.stack([y_rep.sum(0), (y_rep ** 2).sum(0), y_rep.min(0), y_rep.max(0), zero, zero, zero, np.full(R, float(N))], axis=1)


def test_prior_predictive_summary_takes_known_order_statistics():
    from autoreparam_amd import diagnostics
    assert [diagnostics.order_statistic_index(p, 20) for p in (0.05, 0.5, 0.95)] == [0, 9, 18]
    assert [diagnostics.order_statistic_index(p, 1) for p in (0.05, 0.5, 0.95)] == [0, 0, 0]
    assert diagnostics.order_statistic_index(0.05, 21) == 1                  # ceil(1.05) = 2: the second smallest
    R, N = 20, 4
    rs = np.random.RandomState(4)
    means = rs.permutation(np.arange(1.0, R + 1))                            # the replicated means 1 ... 20 in some order
    y_rep = means[None, :] + np.array([-1.5, -0.5, 0.5, 1.5])[:, None]       # sd sqrt(5 / 3), min mean - 1.5, max mean + 1.5
    y = np.array([0.0, 1.0, 2.0, 3.0])
    s = diagnostics.prior_predictive_summary(columns(y_rep), y, 0)
    assert s.draws_used == R and s.draws_left_out == 0
    assert s.quantiles["mean"] == (1.0, 10.0, 19.0)
    assert s.quantiles["min"] == (-0.5, 8.5, 17.5) and s.quantiles["max"] == (2.5, 11.5, 20.5)
    assert np.allclose(s.quantiles["sd"], math.sqrt(5.0 / 3.0), rtol=1e-12)
    mask = np.zeros(R, np.uint8)
    mask[np.argmax(means)] = 1                                               # the draw with mean 20 is left out: 19 kept
    s = diagnostics.prior_predictive_summary(columns(y_rep), y, 0, mask)
    assert s.draws_used == 19 and s.draws_left_out == 1 and s.quantiles["mean"] == (1.0, 10.0, 19.0)
    none = diagnostics.prior_predictive_summary(columns(y_rep), y, 0, np.ones(R))
    assert none.draws_used == 0 and all(v is None for v in none.quantiles.values())


def test_prior_predictive_summary_bernoulli_nulls_and_the_shared_helper():
    from autoreparam_amd import diagnostics
    rs = np.random.RandomState(5)
    y_rep = (rs.rand(6, 40) < 0.3).astype(np.float64)
    y = np.array([1.0, 0, 0, 1, 0, 0])
    s = diagnostics.prior_predictive_summary(columns(y_rep), y, 1)
    assert s.quantiles["sd"] is None and s.quantiles["min"] is None and s.quantiles["max"] is None
    want = np.sort(y_rep.mean(0))[[1, 19, 37]]
    assert s.quantiles["mean"] == tuple(want)
    # one definition of the replicated statistics: ppc_counts' sums are those of the helper's columns
    c = columns(y_rep)
    rep = diagnostics._ppc_replicated(c, 6)
    counts = diagnostics.ppc_counts(c, y)
    assert counts[2 + 5] == np.sum(rep[0]) and counts[2 + 5 + 1] == np.sum(rep[1]) and counts[2] == np.sum(rep[0] >= y.mean())


def test_prior_contraction_summary():
    from autoreparam_amd import diagnostics
    z90 = 1.6448536269514722
    q05 = np.array([-5 * z90, 1.0, 2.0, -np.inf])
    q50 = np.array([0.0, 1.0, 3.0, 0.0])
    q95 = np.array([5 * z90, 1.0, 4.0, 1.0])
    s = diagnostics.prior_contraction_summary(q05, q50, q95, np.array([2.5, 0.0, 3.0, 0.0]), np.array([1.0, 1.0, 2.0, 1.0]))
    assert s.left_out == 2                                                   # a constant element and one without a finite interval
    assert abs(s.prior_sd_robust[0] - 5.0) < 1e-12 and abs(s.contraction[0] - (1 - 1 / 25.0)) < 1e-12 and abs(s.z_score[0] - 0.5) < 1e-12
    assert np.isnan(s.prior_sd_robust[1]) and np.isnan(s.contraction[1]) and np.isnan(s.z_score[1]) and np.isnan(s.contraction[3])
    sd2 = 2.0 / (2 * z90)
    assert abs(s.contraction[2] - (1 - (2.0 / sd2) ** 2)) < 1e-9 and s.contraction[2] < 0 and s.z_score[2] == 0.0
    with pytest.raises(ValueError, match="one length"):
        diagnostics.prior_contraction_summary(q05, q50, q95[:2], q50, q50)


def test_flag_refusal_and_unchanged_keys(capsys):
    from autoreparam_amd import main, models
    from autoreparam_amd.flags import FlagValues
    f = FlagValues()
    assert f.prior_predictive_checks is False
    f.parse(["--prior_predictive_checks", "--model=neals_funnel"])
    with pytest.raises(ValueError, match="--prior_predictive_checks: neals_funnel has no observations"):
        main.check_prior_predictive(f)
    with pytest.raises(ValueError, match="--prior_predictive_checks: neals_funnel has no observations"):
        main.main([], flags=f)
    main.check_predictive_checks(f)                                          # the other reports' rules are their own
    f.parse(["--model=radon"])
    main.check_prior_predictive(f)

    class Results(object):
        trace = None
    cfg = type("Cfg", (), {"model": models._spec_eight_schools()})()
    keys, arrays = main._convergence_report(Results(), cfg, f, None)
    assert arrays is None and tuple(keys) == main.PRIOR_KEYS and all(v is None for v in keys.values())
    assert capsys.readouterr().out.count("prior predictive checks: not computed") == 1
    f.parse(["--predictive_checks"])
    keys, _ = main._convergence_report(Results(), cfg, f, None)
    assert tuple(keys) == main.PPC_KEYS + main.PRIOR_KEYS
    f.parse(["--noprior_predictive_checks"])
    keys, _ = main._convergence_report(Results(), cfg, f, None)
    assert tuple(keys) == main.PPC_KEYS                                      # without the flag: the key set as it was
    f.parse(["--nopredictive_checks"])
    assert main._convergence_report(Results(), cfg, f, None) == ({}, None)
    assert not any(k.startswith("prior_") for k in main.PPC_KEYS + main.LOO_KEYS + main.PSENS_KEYS)


def test_wide_model_writes_null_keys(monkeypatch, capsys):
    from autoreparam_amd import diagnostics, main
    from autoreparam_amd.flags import FlagValues

    def never(*a, **k):
        raise AssertionError("the device function must not be called")
    monkeypatch.setattr(diagnostics, "site_prior_draws", never)
    f = FlagValues()
    f.parse(["--prior_predictive_checks"])
    spec = type("Spec", (), {"D": 300})()
    keys, arrays = main._prior_report(spec, f, None, None, None)
    assert arrays is None and tuple(keys) == main.PRIOR_KEYS and all(v is None for v in keys.values())
    assert capsys.readouterr().out.count("more than 255 elements") == 1


def test_prior_keys_from_summaries():
    from autoreparam_amd import diagnostics, main
    y = np.array([0.0, 1.0, 2.0, 3.0])
    y_rep = np.arange(1.0, 21.0)[None, :] + np.array([-1.5, -0.5, 0.5, 1.5])[:, None]
    c = columns(y_rep)
    summary = diagnostics.ppc_summary(c, np.zeros((4, 4)), y, 0)
    predictive = diagnostics.prior_predictive_summary(c, y, 0)
    contraction = diagnostics.prior_contraction_summary([-1.0, 0.0, -2.0], [0.0, 0.0, 0.0], [1.0, 0.0, 2.0], [0.1, 0.0, -3.0],
                                                        [0.1, 1.0, 1.0])
    keys = main.prior_keys(summary, predictive, contraction, ["mu", "tau", "theta[0]"])
    assert tuple(keys) == main.PRIOR_KEYS[:-1]
    assert keys["prior_draws"] == 20 and keys["prior_rep_mean_q50"] == 10.0 and keys["prior_rep_max_q95"] == 20.5
    assert keys["prior_p_mean"] == 19 / 20.0                                 # replicated means 2 ... 20 are >= the observed 1.5
    assert keys["prior_contraction_min_element"] == "theta[0]" and keys["prior_z_score_max_element"] == "theta[0]"
    assert keys["prior_elements_left_out"] == 1
    json.dumps(keys)


def test_analyze_prints_both_lines(tmp_path, capsys):
    from autoreparam_amd import analyze, main
    d = tmp_path / "8schools"
    d.mkdir()
    run = {key: 0.5 for key in main.PRIOR_KEYS}
    run.update(prior_draws=65536, prior_draws_left_out=3, prior_observations=8, prior_contraction_min_element="log_tau",
               prior_z_score_max_element="theta[0]", prior_elements_left_out=0, prior_p_mean=0.41, prior_contraction_min=0.123)
    (d / "CP_tied.json").write_text(json.dumps({k: [None, v] for k, v in run.items()}))
    (d / "NCP_tied.json").write_text(json.dumps({k: [v, None] for k, v in run.items()}))
    (d / "cVIP_eig_tied.json").write_text(json.dumps({"ess_min": [1.0]}))
    analyze.main(["--results_dir", str(tmp_path), "--model", "8schools", "--prior"])
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("CP_tied:")]
    assert len(lines) == 2 and "mean 0.41" in lines[0] and "65536 prior draws, 3 left out" in lines[0]
    assert "least contraction 0.123 (log_tau)" in lines[1] and "(theta[0])" in lines[1]
    assert "NCP_tied: prior predictive checks not computed" in out and "cVIP" not in out
    analyze.main(["--results_dir", str(tmp_path), "--model", "8schools", "--ppc"])
    assert "prior" not in capsys.readouterr().out


def test_symbol_is_declared_and_listed():
    from autoreparam_amd import _lib
    src = open(os.path.join(ROOT, "include", "autoreparam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)                          # as tests/test_abi.py reads the header
    declared = sorted(set(re.findall(r"\b(arp_[a-z_0-9]+)\s*\(", src)))
    assert "arp_site_prior_draws" in declared and "arp_site_prior_draws" in _lib.SYMBOLS
    assert sorted(declared) == sorted(_lib.SYMBOLS)
    assert os.path.exists(os.path.join(ROOT, "autoreparam_amd", "csrc", "prior_draw.hip"))


def test_wrapper_refuses_what_the_kernel_refuses():
    from autoreparam_amd import diagnostics
    up = diagnostics.upload_site_table(synthetic_chain(6), 6, "cpu")
    for kwargs, word in ((dict(draws=0), "1 <= draws"), (dict(draws=(1 << 24) + 1), "1 <= draws"),
                         (dict(draws=4, draw_offset=-1), "draw_offset"), (dict(draws=4), "on the GPU")):
        with pytest.raises(ValueError, match=word):
            diagnostics.site_prior_draws(up, **kwargs)
    with pytest.raises(ValueError, match="DeviceSiteTable"):
        diagnostics.site_prior_draws(synthetic_chain(6), 4)
