"""Moment matching for a high Pareto k-hat, the part that needs no device: the float64 restatement (tests/mmatch_ref.py)
on the closed-form case, the flags' refusals, the key lists and their null path, the batch rule, the host formulas and
the files."""
import json
import os

import numpy as np
import pytest

import mmatch_cases as mc
import mmatch_ref as mr
import psis_ref as pr

TAU = pr.k_threshold(mc.DRAWS)


def plain_and_matched(case, seed):
    x = mc.draws(seed)
    plain = pr.psis_row(mc.loglik(case, x).astype(np.float32))
    res = mr.moment_match(x, np.zeros(mc.DRAWS, bool), mc.logp, lambda t, rows: mc.loglik(case, rows), [0], [plain[1]], [plain[0]],
                          TAU)
    return plain, res


@pytest.mark.parametrize("seed", mc.SEEDS)
def test_the_restatement_repairs_the_closed_form_case(seed):
    """Posterior N(0, I_4), left-out term Normal(2.0 | theta_0, variance 1.3); the exact elpd is -8.44996.  Measured
    (plain error, matched error) and (plain k-hat, final k-hat), maps:
      seed 0: (1.594, 0.016), (1.360, 0.648), "12";    seed 1: (2.523, 0.027), (1.146, 0.319), "112";
      seed 2: (2.721, 0.145), (1.055, 0.680), "111";   seed 3: (2.954, 0.438), (0.967, 0.616), "11"."""
    exact = mc.exact_elpd(mc.HIGH)
    assert abs(exact - -8.44996) < 1e-5
    plain, res = plain_and_matched(mc.HIGH, seed)
    print("seed", seed, "plain", plain[0] - exact, plain[1], "matched", res.elpd[0] - exact, res.pareto_k[0], res.maps[0])
    assert plain[1] > TAU and res.attempted[0]
    assert len(res.maps[0]) >= 1 and set(res.maps[0]) <= {"1", "2"}
    assert res.pareto_k[0] < plain[1]
    assert abs(res.elpd[0] - exact) <= 0.25 * abs(plain[0] - exact)
    assert np.all(np.isfinite(res.scale[0])) and np.all(np.isfinite(res.shift[0])) and res.is_ess[0] > 1


@pytest.mark.parametrize("seed", mc.SEEDS)
def test_a_target_below_the_threshold_is_not_touched(seed):
    plain, res = plain_and_matched(mc.LOW, seed)
    assert plain[1] <= TAU and not res.attempted[0] and res.maps[0] == ""
    assert res.elpd[0].tobytes() == np.float64(plain[0]).tobytes() and res.pareto_k[0].tobytes() == np.float64(plain[1]).tobytes()
    assert np.isnan(res.scale[0]).all() and np.isnan(res.shift[0]).all() and np.isnan(res.pareto_k_full[0])


def test_the_float32_affine_restatement_and_its_parity():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((7, 3)).astype(np.float32)
    x[2, 1], x[3, 0] = np.nan, np.inf
    m, s, u = (rng.standard_normal((2, 3)).astype(np.float32) for _ in range(3))
    every = mr.affine_rows(x, m, s, u)
    want = ((x[None] - m[:, None]).astype(np.float32) * s[:, None]).astype(np.float32) + u[:, None]
    assert every.dtype == np.float32 and every.tobytes() == want.astype(np.float32).tobytes()
    for parity in (0, 1):
        out = mr.affine_rows(x, m, s, u, parity)
        moved = (np.arange(7) & 1) == parity
        assert out[:, moved].tobytes() == every[:, moved].tobytes()
        assert out[:, ~moved].tobytes() == np.repeat(x[None, ~moved], 2, axis=0).tobytes()
    # three roundings, not a fused or a float64 evaluation
    a = np.float32(1.0) + np.float32(2.0 ** -23)
    one = mr.affine_rows(np.array([[a]], np.float32), [[0.0]], [[a]], [[2.0 ** -24]])[0, 0, 0]
    assert one == np.float32(np.float32(a * a) + np.float32(2.0 ** -24))


def test_the_moment_restatement_on_a_case_worked_by_hand():
    x = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0], [np.nan, np.inf]], np.float32)
    lw = np.array([[0.0, np.log(2.0), -np.inf, -np.inf], [-np.inf] * 4, [0.0, 0.0, 0.0, -np.inf], [0.0, np.nan, 0.0, -np.inf]])
    out, mag = mr.weighted_moments(x, lw, np.array([1.0, 0.0], np.float32))
    # w = (1/2, 1): sum w = 1.5, sum w^2 = 1.25; column 0 about 1: e = (0, 1); column 1 about 0: e = (10, 20)
    assert np.allclose(out[0], [np.log(2.0), 1.5, 1.25, 2, 1.0, 1.0, 25.0, 450.0], rtol=1e-15)
    assert out[1].tolist() == [-np.inf, 0, 0, 0, 0, 0, 0, 0]
    assert out[2].tolist() == [0.0, 3.0, 3.0, 3.0, 4.0, 10.0, 70.0, 2100.0]
    assert out[3, 0] == 0.0 and out[3, 3] == 3 and np.isnan(out[3, [1, 2, 4, 5, 6, 7]]).all()
    sums = [1, 2, 4, 5, 6, 7]
    assert np.all(mag[:3][:, sums] >= np.abs(out[:3][:, sums]) * (1 - 1e-15)) and mr.bound(3, 1.0) == 35 * 2.0 ** -52


def test_flag_refusals_before_any_device_and_the_keys(capsys, monkeypatch):
    import torch
    from autoreparam_amd import main, models
    from autoreparam_amd.flags import FlagValues

    def touched(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    monkeypatch.setattr(torch.cuda, "device_count", touched)
    f = FlagValues()
    assert f.loo_moment_match is False and f.loo_moment_match_max == 64 and not main.loo_moment_match(f)
    main.check_loo_moment_match(f)
    f.parse(["--model=radon", "--loo_moment_match"])
    with pytest.raises(ValueError, match="--loo_moment_match is read with --predictive_diagnostics only"):
        main.main([], flags=f)
    f.parse(["--predictive_diagnostics"])
    main.check_loo_moment_match(f)
    for cap in (0, -1, 4097):
        f.parse(["--loo_moment_match_max=%d" % cap])
        with pytest.raises(ValueError, match="^--loo_moment_match_max: .*outside 1 ... 4096"):
            main.main([], flags=f)
    for cap in (1, 4096):
        f.parse(["--loo_moment_match_max=%d" % cap])
        main.check_loo_moment_match(f)
    f.parse(["--model=neals_funnel"])                                         # (main.main stops at --predictive_diagnostics itself)
    with pytest.raises(ValueError, match="--loo_moment_match: neals_funnel has no observations"):
        main.check_loo_moment_match(f)
    with pytest.raises(ValueError, match="neals_funnel has no observations"):
        main.main([], flags=f)

    assert main.LOO_MM_KEYS == (
        "loo_mm_observations", "loo_mm_not_attempted", "loo_mm_improved", "loo_mm_resolved", "loo_mm_iterations_max", "elpd_loo_mm",
        "elpd_loo_mm_se", "p_loo_mm", "loo_mm_pareto_k_max", "loo_mm_pareto_k_max_observation", "loo_mm_pareto_k_above_threshold",
        "loo_mm_full_pareto_k_max", "loo_mm_time_sec")
    assert main.LOGO_MM_KEYS == (
        "logo_mm_observations", "logo_mm_not_attempted", "logo_mm_improved", "logo_mm_resolved", "logo_mm_iterations_max",
        "elpd_logo_mm", "elpd_logo_mm_se", "p_logo_mm", "logo_mm_pareto_k_max", "logo_mm_pareto_k_max_group",
        "logo_mm_pareto_k_above_threshold", "logo_mm_full_pareto_k_max", "logo_mm_time_sec")
    assert not set(main.LOO_MM_KEYS + main.LOGO_MM_KEYS) & set(main.LOO_KEYS + main.LOO_PRED_KEYS + main.LOGO_KEYS)

    # null whenever the LOO report's keys are: no device trace, and a sharded job -- no message of its own
    class Results(object):
        trace = None
    cfg = type("Cfg", (), {"model": models._spec_eight_schools()})()
    for extra, want in ((["--loo_moment_match"], main.LOO_KEYS + main.LOO_MM_KEYS),
                        (["--loo_moment_match", "--loo_groups=theta"],
                         main.LOO_KEYS + main.LOGO_KEYS + main.LOO_MM_KEYS + main.LOGO_MM_KEYS),
                        (["--loo_groups=theta"], main.LOO_KEYS + main.LOGO_KEYS)):
        f = FlagValues()
        f.parse(["--predictive_diagnostics"] + extra)
        capsys.readouterr()
        keys, arrays = main._convergence_report(Results(), cfg, f, None)
        assert arrays is None and tuple(keys) == want and all(v is None for v in keys.values())
        assert capsys.readouterr().out.count("not computed") == 1
        monkeypatch.setattr(main.parallel, "world", lambda: (0, 2))
        keys, arrays = main._loo_report(None, None, 4, cfg.model, f)
        assert arrays is None and tuple(keys) == want and all(v is None for v in keys.values())
        assert capsys.readouterr().out.count("not computed") == 1
        monkeypatch.setattr(main.parallel, "world", lambda: (0, 1))


def test_the_batch_rule_at_its_edges():
    from autoreparam_amd import report_common as rc
    R, D = 8192, 10
    one = 4 * R * D
    assert rc.mm_batch_size(64, R, D, budget=one * 7) == 7
    assert rc.mm_batch_size(64, R, D, budget=one * 7 - 1) == 6
    assert rc.mm_batch_size(64, R, D, budget=one - 1) == 1                    # at least one, whatever the budget
    assert rc.mm_batch_size(3, R, D, budget=one * 7) == 3                     # no more than there are
    assert rc.mm_batch_size(0, R, D) == 1
    assert rc.mm_batch_size(10 ** 6, 1, 1) == rc.MM_MAX_BATCH == 4095         # one row is left for the unweighted moments
    assert rc.mm_batch_size(64, 65536, 255) == rc.LOO_CHUNK_BYTES // (4 * 65536 * 255) == 4


def fake_result(chosen, D, rng):
    from autoreparam_amd import diagnostics
    n = len(chosen)
    maps = ["12", "", "111"][:n] + ["1"] * max(0, n - 3)
    return diagnostics.MomentMatch(np.ones(n, bool), rng.standard_normal(n), rng.uniform(0.2, 0.9, n), rng.uniform(0, 2, n),
                                   rng.uniform(0, 1, n), rng.uniform(10, 100, n), np.array([len(m) for m in maps]), maps,
                                   rng.uniform(0.5, 2, (n, D)), rng.standard_normal((n, D)), np.zeros(D))


def test_selection_merge_and_keys_on_the_host():
    from autoreparam_amd import diagnostics, main
    rng = np.random.default_rng(11)
    T, D = 9, 3
    c = rng.standard_normal((T, 8))
    c[:, 1] = [0.1, 0.9, np.inf, 0.71, 0.7, 1.5, 0.9, np.nan, 0.2]
    chosen, past = main.mm_select(c[:, 1], 0.7, 64)
    assert chosen.tolist() == [2, 5, 1, 6, 3] and past == 0                    # the worst first, ties ascending, +inf included, NaN not
    chosen, past = main.mm_select(c[:, 1], 0.7, 3)
    assert chosen.tolist() == [2, 5, 1] and past == 2
    assert main.mm_select(c[:, 1], 2.0, 3)[0].tolist() == [2] and main.mm_select([0.1, 0.2], 0.7, 3)[0].size == 0

    res = fake_result(chosen, D, rng)
    res.pareto_k[:] = [0.5, 1.2, 0.9]                                          # 2: resolved; 5: improved; 1: as it was
    res.elpd[1] = c[5, 0]                                                      # (no map accepted: the plain figure)
    merged = main.mm_merge(c, chosen, res)
    assert merged["attempted"].tolist() == [i in (1, 2, 5) for i in range(T)]
    rest = ~merged["attempted"]
    assert merged["elpd_loo_i"][rest].tobytes() == c[rest, 0].tobytes() and merged["pareto_k"][rest].tobytes() == c[rest, 1].tobytes()
    assert merged["elpd_loo_i"][[2, 5, 1]].tolist() == res.elpd.tolist() and merged["maps"].tolist()[:3] == ["", "111", "12"]
    assert merged["maps"].dtype.kind == "U" and merged["iterations"].tolist() == [0, 3, 2, 0, 0, 0, 0, 0, 0]
    assert merged["shift"].shape == (T, D) and np.isnan(merged["shift"][rest]).all() and np.array_equal(merged["scale"][5], res.scale[1])
    assert np.isnan(merged["pareto_k_full"][rest]).all() and np.isnan(merged["is_ess"][rest]).all()

    keys = main.mm_keys("loo", c, merged, past, 0.7)
    assert tuple(keys) == main.LOO_MM_KEYS[:-1]
    want = diagnostics.loo_summary(merged["elpd_loo_i"], c[:, 2], c[:, 3])      # loo_summary applied to the merged column
    assert (keys["elpd_loo_mm"], keys["elpd_loo_mm_se"], keys["p_loo_mm"]) == (want.elpd_loo, want.elpd_loo_se, want.p_loo)
    assert want.elpd_loo == merged["elpd_loo_i"].sum() and want.p_loo == (c[:, 2] - merged["elpd_loo_i"]).sum()
    assert keys["loo_mm_observations"] == 3 and keys["loo_mm_not_attempted"] == 2
    assert keys["loo_mm_improved"] == 2 and keys["loo_mm_resolved"] == 1 and keys["loo_mm_iterations_max"] == 3
    assert keys["loo_mm_pareto_k_max"] == 1.2 and keys["loo_mm_pareto_k_max_observation"] == 5
    assert keys["loo_mm_pareto_k_above_threshold"] == 4                        # 1, 3, 5, 6
    assert keys["loo_mm_full_pareto_k_max"] == res.pareto_k_full.max()

    # groups: an empty group's row is NaN throughout and enters nothing; the worst is named
    g = c.copy()
    g[7] = np.nan
    names = ["m[%d]" % i for i in range(T)]
    merged = main.mm_merge(g, chosen, res)
    keys = main.mm_keys("logo", g, merged, 0, 0.7, names)
    assert tuple(keys) == main.LOGO_MM_KEYS[:-1] and keys["logo_mm_pareto_k_max_group"] == "m[5]"
    filled = np.arange(T) != 7
    want = diagnostics.loo_summary(merged["elpd_loo_i"][filled], g[filled, 2], g[filled, 3])
    assert (keys["elpd_logo_mm"], keys["elpd_logo_mm_se"], keys["p_logo_mm"]) == (want.elpd_loo, want.elpd_loo_se, want.p_loo)

    # nothing above the threshold: zeros, and the totals are the plain ones
    c[2, 1] = 0.3
    none, past = main.mm_select(c[:, 1], 5.0, 64)
    merged = main.mm_merge(c, none, fake_result(none, D, rng))
    keys = main.mm_keys("loo", c, merged, past, 5.0)
    plain = diagnostics.loo_summary(c[:, 0], c[:, 2], c[:, 3])
    assert keys["loo_mm_observations"] == 0 and keys["loo_mm_iterations_max"] == 0 and keys["elpd_loo_mm"] == plain.elpd_loo
    assert keys["loo_mm_full_pareto_k_max"] is None and merged["shift"].shape == (T, D)


def test_the_files_are_written_from_save_loo_and_analyze_prints_the_line(tmp_path, capsys):
    from autoreparam_amd import analyze, main
    rng = np.random.default_rng(3)
    N, G, D = 6, 4, 3
    plain = {"elpd_loo_i": rng.standard_normal(N), "pareto_k": rng.uniform(0, 1, N), "lppd_i": rng.standard_normal(N),
             "p_waic_i": rng.uniform(0, 1, N), "y": rng.standard_normal(N).astype(np.float32), "model": np.asarray("radon")}
    logo = {"part": np.asarray("m"), "groups": np.asarray(["m[%d]" % g for g in range(G)]), "elpd_logo_g": rng.standard_normal(G)}
    mm = lambda T: main.mm_merge(rng.standard_normal((T, 8)), [1], fake_result([1], D, rng))
    base = str(tmp_path / "CP")
    arrays = dict(plain)
    arrays[main.LOGO_ARRAYS] = dict(logo, **{main.LOGO_MM_ARRAYS: mm(G)})
    arrays[main.LOO_MM_ARRAYS] = mm(N)
    main.save_loo(base, arrays)
    assert sorted(os.listdir(str(tmp_path))) == ["CP_logo.npz", "CP_logo_mm.npz", "CP_loo.npz", "CP_loo_mm.npz"]
    assert main.LOO_MM_ARRAYS in arrays and main.LOGO_MM_ARRAYS in arrays[main.LOGO_ARRAYS]       # the caller's dicts are left alone
    with np.load(base + "_loo.npz") as z:
        assert sorted(z.files) == sorted(plain) and all(np.array_equal(z[name], plain[name]) for name in plain)
    with np.load(base + "_logo.npz") as z:
        assert sorted(z.files) == sorted(logo)
    for name, T in (("_loo_mm.npz", N), ("_logo_mm.npz", G)):
        with np.load(base + name) as z:
            assert {"attempted", "elpd_loo_i", "pareto_k", "pareto_k_full", "pareto_k_split", "is_ess", "iterations", "maps",
                    "shift", "scale"} <= set(z.files)
            assert z["attempted"].tolist() == [t == 1 for t in range(T)] and z["shift"].shape == (T, D) and z["maps"][1] == "12"
    # without the flag's arrays: the two files of before, nothing else
    other = tmp_path / "plain"
    other.mkdir()
    main.save_loo(str(other / "CP"), dict(plain, **{main.LOGO_ARRAYS: dict(logo)}))
    assert sorted(os.listdir(str(other))) == ["CP_logo.npz", "CP_loo.npz"]

    # analyze --loo: the line, for a run that recorded the keys, and none for one that did not
    run = {key: [None, 1.5] for key in main.LOO_KEYS + main.LOGO_KEYS + main.LOO_MM_KEYS + main.LOGO_MM_KEYS}
    run.update(loo_observations=[6, 6], logo_groups=[4, 4], logo_part=["m", "m"], logo_marginal=[True, True],
               loo_mm_observations=[2, 2], logo_mm_observations=[None, 3], elpd_loo_mm=[0.0, -12.25], elpd_logo_mm=[0.0, -7.5],
               logo_mm_pareto_k_max_group=["m[0]", "m[2]"])
    lines = analyze.report_loo({"CP": run})
    matched = [line for line in lines if "moment matching" in line]
    assert len(matched) == 2 and "elpd_loo_mm -12.25" in matched[0] and "elpd_logo_mm -7.5" in matched[1]
    assert "2 observation(s)" in matched[0] and "3 group(s), conditional form" in matched[1] and "(plain 1.5" in matched[0]
    for key in main.LOO_MM_KEYS + main.LOGO_MM_KEYS:
        del run[key]
    assert not [line for line in analyze.report_loo({"CP": run}) if "moment matching" in line]
    json.dumps(dict(main.mm_keys("loo", rng.standard_normal((3, 8)), mm(3), 0, 0.7)))            # plain Python values
