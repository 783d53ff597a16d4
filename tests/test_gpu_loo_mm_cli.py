"""GPU: --loo_moment_match end to end through main.main, at the sizes of test_gpu_logo_cli (NCP or CP, 256 chains, 200
samples, --loo_draws=8192, one copied VI / tuning directory).

Radon MA grouped by m, two sampling runs, --predictive_diagnostics --loo_groups=m with and without the flag: the flag adds
exactly LOO_MM_KEYS, LOGO_MM_KEYS and the two _mm.npz files and changes nothing else, bit for bit; no attempted group's
k-hat rises, at least one falls; and over the attempted groups the matched conditional elpd lies closer to the MARGINAL one
-- the exact ratio with a low k-hat, on a posterior that is Gaussian -- than the plain conditional elpd does, in the sum of
absolute differences.  Election by a (Bernoulli: no marginal form, conditional k-hat up to 1.5): the report runs and the
worst k-hat does not rise.  Eight schools CP, observations only.  analyze --loo prints the line."""
import json
import os
import shutil

import numpy as np
import pytest

from test_gpu_loo_cli import HM, _cli, pipeline

pytestmark = pytest.mark.gpu

RUN = ["--predictive_diagnostics", "--loo_draws=8192"]
MM_FILES = sorted(["attempted", "elpd_loo_i", "pareto_k", "pareto_k_full", "pareto_k_split", "is_ess", "iterations", "maps", "shift",
                   "scale", "y", "model"])


def path(root, suffix, method="NCP"):
    return os.path.join(root, method + "_tied" + suffix)


@pytest.fixture(scope="module")
def radon_pair(gpu, tmp_path_factory):
    """(on, off, top): radon MA by county with and without --loo_moment_match, from one VI / tuning directory."""
    top = tmp_path_factory.mktemp("radon_mm")
    on, off = str(top / "on"), str(top / "off")
    common = ["--model=radon", "--dataset=MA", "--num_chains=256", "--seed=3", "--num_optimization_steps=400", "--method=NCP"]
    _cli(common + ["--results_dir=" + on, "--inference=VI"])
    _cli(common + ["--results_dir=" + on, "--inference=HMCtuning", "--num_leapfrog_steps=4"] + HM)
    shutil.copytree(on, off)
    _cli(common + ["--results_dir=" + off, "--inference=HMC", "--loo_groups=m"] + RUN + HM)
    _cli(common + ["--results_dir=" + on, "--inference=HMC", "--loo_groups=m", "--loo_moment_match"] + RUN + HM)
    return on, off, str(top)


def check_mm_file(z, T, D, grouped):
    want = MM_FILES + (["part", "groups", "group_of"] if grouped else [])
    assert sorted(z.files) == sorted(want)
    tried = z["attempted"]
    assert tried.dtype == bool and tried.shape == (T,) and z["shift"].shape == z["scale"].shape == (T, D)
    assert np.isnan(z["shift"][~tried]).all() and np.isnan(z["scale"][~tried]).all() and np.isfinite(z["scale"][tried]).all()
    assert np.isnan(z["pareto_k_full"][~tried]).all() and not z["iterations"][~tried].any() and all(m == "" for m in z["maps"][~tried])
    assert all(len(m) == n and set(m) <= {"1", "2"} for m, n in zip(z["maps"], z["iterations"])) and z["iterations"].max() <= 30
    return tried


def test_radon_by_county_is_repaired_towards_the_marginal_form(radon_pair, capsys):
    """Measured: 12 of 13 counties attempted, k-hat fell for 12 (1.06 -> 0.83 at worst), 11 at or below 0.7; the sum over the
    attempted counties of |elpd - marginal elpd| is 6.96 matched against 14.41 plain conditional."""
    from autoreparam_amd import main as cli, models
    on, off, _ = radon_pair
    r, plain = json.load(open(path(on, ".json"))), json.load(open(path(off, ".json")))
    D = models._spec_radon("MA").D
    z, logo = np.load(path(on, "_logo_mm.npz")), np.load(path(on, "_logo.npz"))
    tried = check_mm_file(z, 13, D, True)
    k_plain, k = logo["conditional_pareto_k"], z["pareto_k"]
    tau = r["logo_pareto_k_threshold"][0]
    assert np.array_equal(tried, k_plain > tau) and tried.sum() == r["logo_mm_observations"][0] >= 1
    assert r["logo_mm_not_attempted"] == [0]
    assert np.all(k[tried] <= k_plain[tried])                                  # by construction: the bookkeeping
    assert np.array_equal(k[~tried], k_plain[~tried]) and np.array_equal(z["elpd_loo_i"][~tried], logo["conditional_elpd_logo_g"][~tried])
    assert r["logo_mm_improved"][0] == int(np.sum(k[tried] < k_plain[tried])) >= 1
    assert r["logo_mm_resolved"][0] == int(np.sum(k[tried] <= tau))
    assert r["logo_mm_pareto_k_max"][0] == k.max() <= r["logo_conditional_pareto_k_max"][0]
    assert r["logo_mm_pareto_k_max_group"][0] == list(z["groups"])[int(k.argmax())]
    assert r["elpd_logo_mm"][0] == pytest.approx(z["elpd_loo_i"].sum(), rel=1e-12)
    assert 0 < r["logo_mm_time_sec"][0] <= r["logo_time_sec"][0] <= r["loo_time_sec"][0]
    # the yardstick: the marginal form
    marginal = logo["elpd_logo_g"]
    matched_gap = float(np.abs(z["elpd_loo_i"][tried] - marginal[tried]).sum())
    plain_gap = float(np.abs(logo["conditional_elpd_logo_g"][tried] - marginal[tried]).sum())
    with capsys.disabled():
        print("\nradon MA by m: %d of 13 groups attempted, k-hat fell for %d, at or below %.3f for %d, at most %d maps; worst k-hat "
              "%.3f (plain conditional %.3f, marginal %.3f)" % (tried.sum(), r["logo_mm_improved"][0], tau, r["logo_mm_resolved"][0],
                                                                r["logo_mm_iterations_max"][0], k.max(), k_plain.max(),
                                                                r["logo_pareto_k_max"][0]))
        print("sum over the attempted groups of |elpd - marginal elpd|: matched %.4f, plain conditional %.4f" % (matched_gap, plain_gap))
        print("elpd_logo_mm %.4f, conditional %.4f, marginal %.4f; logo_mm_time_sec %.3f, loo_mm_time_sec %.3f of loo_time_sec %.3f"
              % (r["elpd_logo_mm"][0], r["logo_conditional_elpd"][0], r["elpd_logo"][0], r["logo_mm_time_sec"][0],
                 r["loo_mm_time_sec"][0], r["loo_time_sec"][0]))
        for g in np.flatnonzero(tried):
            print("  %s: k %.3f -> %.3f (full %.3f, split %.3f), maps %s, elpd %.4f -> %.4f (marginal %.4f), ESS %.0f"
                  % (z["groups"][g], k_plain[g], k[g], z["pareto_k_full"][g], z["pareto_k_split"][g], z["maps"][g],
                     logo["conditional_elpd_logo_g"][g], z["elpd_loo_i"][g], marginal[g], z["is_ess"][g]))
    assert matched_gap < plain_gap
    # the observations' report ran too
    zo = np.load(path(on, "_loo_mm.npz"))
    check_mm_file(zo, r["loo_observations"][0], D, False)
    for key in cli.LOO_MM_KEYS + cli.LOGO_MM_KEYS:
        assert len(r[key]) == 1, key
    assert set(r) - set(plain) == set(cli.LOO_MM_KEYS + cli.LOGO_MM_KEYS)


def test_the_flag_changes_nothing_that_was_there(radon_pair):
    from autoreparam_amd import main as cli
    on, off, _ = radon_pair
    r, plain = json.load(open(path(on, ".json"))), json.load(open(path(off, ".json")))
    assert set(plain) <= set(r)
    for key in plain:
        if "time" not in key:
            assert plain[key] == r[key], key
    for key in cli.LOO_KEYS + cli.LOGO_KEYS:
        assert key in plain and ("time" in key or plain[key] == r[key]), key
    for suffix in ("_loo.npz", "_logo.npz", "_rhat.npz", "_ess.npz"):
        a, b = np.load(path(on, suffix)), np.load(path(off, suffix))
        assert sorted(a.files) == sorted(b.files), suffix
        assert all(a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes() for name in a.files), suffix
    assert not os.path.exists(path(off, "_loo_mm.npz")) and not os.path.exists(path(off, "_logo_mm.npz"))


def test_analyze_prints_the_line(radon_pair, capsys):
    from autoreparam_amd import analyze
    on, off, top = radon_pair
    r = json.load(open(path(on, ".json")))
    capsys.readouterr()
    analyze.main(["--results_dir=" + top, "--model=on", "--loo"])
    shown = capsys.readouterr().out
    assert "      moment matching over {} group(s), conditional form".format(r["logo_mm_observations"][0]) in shown
    assert "elpd_logo_mm {:.4g} +/- {:.4g} (plain {:.4g})".format(r["elpd_logo_mm"][0], r["elpd_logo_mm_se"][0],
                                                                 r["logo_conditional_elpd"][0]) in shown
    assert "      moment matching over {} observation(s)".format(r["loo_mm_observations"][0]) in shown
    analyze.main(["--results_dir=" + top, "--model=off", "--loo"])
    assert "moment matching" not in capsys.readouterr().out


def test_election_by_state(gpu, tmp_path, capsys):
    from autoreparam_amd import main as cli
    root = str(tmp_path / "election")
    pipeline(root, "election", [], RUN + ["--loo_groups=a", "--loo_moment_match"])
    text = capsys.readouterr().out
    r = json.load(open(path(root, ".json")))
    assert r["logo_mm_observations"][0] >= 1
    null_ok = {"logo_mm_full_pareto_k_max", "loo_mm_full_pareto_k_max", "loo_mm_pareto_k_max_observation"}
    for key in cli.LOO_MM_KEYS + cli.LOGO_MM_KEYS:
        v = r[key]
        assert len(v) == 1 and (v[0] is not None or key in null_ok), key
        assert v[0] is None or isinstance(v[0], str) or np.isfinite(v[0]), key
    assert r["logo_mm_pareto_k_max"][0] <= r["logo_conditional_pareto_k_max"][0]
    z, logo = np.load(path(root, "_logo_mm.npz")), np.load(path(root, "_logo.npz"))
    tried = check_mm_file(z, 51, int(z["shift"].shape[1]), True)
    assert np.all(z["pareto_k"][tried] <= logo["conditional_pareto_k"][tried]) and not tried[logo["n_obs"] == 0].any()
    line = [l for l in text.splitlines() if l.startswith("    moment matching over") and "group(s) of a" in l]
    assert len(line) == 1
    with capsys.disabled():
        print("\n" + line[0].strip())
        print("election by a: k-hat max %.3f -> %.3f; logo_mm_time_sec %.3f, loo_mm_time_sec %.3f of loo_time_sec %.3f"
              % (r["logo_conditional_pareto_k_max"][0], r["logo_mm_pareto_k_max"][0], r["logo_mm_time_sec"][0], r["loo_mm_time_sec"][0],
                 r["loo_time_sec"][0]))


def test_eight_schools_observations_only(gpu, tmp_path, capsys):
    from autoreparam_amd import main as cli
    root = str(tmp_path / "schools")
    common = ["--model=8schools", "--num_chains=256", "--seed=3", "--num_optimization_steps=400", "--method=CP", "--results_dir=" + root]
    _cli(common + ["--inference=VI"])
    _cli(common + ["--inference=HMCtuning", "--num_leapfrog_steps=4"] + HM)
    _cli(common + ["--inference=HMC", "--loo_moment_match"] + RUN + HM)
    text = capsys.readouterr().out
    r = json.load(open(path(root, ".json", "CP")))
    assert set(cli.LOO_MM_KEYS) <= set(r) and not set(cli.LOGO_MM_KEYS) & set(r)
    z, loo = np.load(path(root, "_loo_mm.npz", "CP")), np.load(path(root, "_loo.npz", "CP"))
    tried = check_mm_file(z, 8, 10, False)
    assert np.array_equal(tried, loo["pareto_k"] > r["pareto_k_threshold"][0]) and r["loo_mm_observations"] == [int(tried.sum())]
    assert z["elpd_loo_i"][~tried].tobytes() == loo["elpd_loo_i"][~tried].tobytes()
    assert z["pareto_k"][~tried].tobytes() == loo["pareto_k"][~tried].tobytes() and np.all(z["pareto_k"][tried] <= loo["pareto_k"][tried])
    assert np.array_equal(z["y"], loo["y"]) and not os.path.exists(path(root, "_logo_mm.npz", "CP"))
    if not tried.any():
        assert r["elpd_loo_mm"] == r["elpd_loo"] and r["loo_mm_pareto_k_max"] == r["pareto_k_max"]
    with capsys.disabled():
        print("\n" + [l for l in text.splitlines() if l.startswith("    moment matching over")][0].strip())
