"""GPU: --vi_diagnostics end to end -- radon MN through main.main at the reference's defaults for CP, NCP and cVIP: the JSON
keys, <method>_vicheck.npz, the evidence of CP against the closed form, the route from a result file written without the
flag, analyze --vi, and the test that the density checked is the one the fit optimised:

    |vi_elbo_final - elbo| <= 4 estimated_elbo_std + 6 vi_elbo_final_se

(not derived: it covers the jitter of the optimiser's last 32 iterates by their own spread).  Measured on an MI355X, seed 3
(gap against bound; k-hat):  CP 0.0116 against 0.190 (0.508);  NCP 0.0111 against 0.350 (0.933);  cVIP 0.0044 against 0.165
(0.527).  CP's log evidence: -1163.4071 against the closed form's -1163.3952, se 0.0064."""
import json
import math
import os

import numpy as np
import pytest

from vicheck_ref import Case

pytestmark = pytest.mark.gpu

COMMON = ["--model=radon", "--dataset=MN", "--inference=VI", "--seed=3"]
FILES = {"CP": "CP_tied", "NCP": "NCP_tied", "cVIP": "cVIP_eig_tied"}


def _cli(args):
    from autoreparam_amd import flags as flags_mod
    from autoreparam_amd import main as cli
    return cli.main(args, flags=flags_mod.FlagValues())


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("vicheck"))
    for method in FILES:
        _cli(COMMON + ["--method=" + method, "--results_dir=" + root, "--vi_diagnostics"])
    return root, {m: json.load(open(os.path.join(root, f + ".json"))) for m, f in FILES.items()}


@pytest.mark.parametrize("method", sorted(FILES))
def test_keys_and_arrays(runs, method):
    from autoreparam_amd import main as cli, models
    root, results = runs
    r = results[method]
    spec = models.get_model_by_name("radon", dataset="MN").model
    names = cli.element_names(spec)
    for key in cli.VI_CHECK_KEYS:
        assert key in r, key
        if key.endswith("_element"):
            assert r[key] in names, (key, r[key])
        else:
            assert r[key] is not None and math.isfinite(r[key]), (key, r[key])
    assert r["vi_check_draws"] == 65536 and r["vi_check_draws_left_out"] == 0 and r["vi_tail_length"] == 768
    assert 0 < r["vi_is_ess"] <= 65536 and r["vi_pareto_k_threshold"] == 0.7 and r["vi_check_time_sec"] > 0
    assert r["vi_sd_ratio_min"] <= r["vi_sd_ratio_max"] and r["vi_score_gap_max"] >= 0
    assert r["vi_kl_estimate"] == pytest.approx(r["vi_log_evidence"] - r["vi_elbo_final"], abs=1e-9)
    with np.load(os.path.join(root, FILES[method] + "_vicheck.npz")) as z:
        assert len(z.files) == len(cli.VI_CHECK_FAMILIES) * len(spec.part_names) + 3
        for family in cli.VI_CHECK_FAMILIES:
            for name, shape in zip(spec.part_names, spec.part_shapes):
                a = z["%s/%s" % (family, name)]
                assert a.shape == tuple(shape) and np.all(np.isfinite(a)), (family, name)
        assert z["log_ratio"].shape == (65536,) and z["log_ratio"].dtype == np.float32 and np.all(np.isfinite(z["log_ratio"]))
        assert z["log_weight"].shape == (65536,) and z["log_weight"].dtype == np.float64 and z["log_weight"].max() <= 0.0
        assert int(z["left_out"]) == 0
        # the JSON figures are the arrays': ELBO of the final parameters, and the largest score gap
        const = r["vi_elbo_final"] - float(np.mean(z["log_ratio"].astype(np.float64)))
        assert r["vi_log_evidence"] == pytest.approx(
            float(np.log(np.mean(np.exp(z["log_weight"])))) + float(z["log_ratio"].astype(np.float64).max()) + const, abs=1e-6)
        gaps = np.concatenate([z["score_gap/" + n].reshape(-1) for n in spec.part_names])
        assert r["vi_score_gap_max"] == gaps.max() and r["vi_score_gap_max_element"] == names[int(gaps.argmax())]


def test_cp_evidence_against_the_closed_form(runs, oracle_lib):
    _, results = runs
    c = Case(oracle_lib, "CP")
    evidence = c.logp_mean + 0.5 * c.sp.D * math.log(2.0 * math.pi) - 0.5 * np.linalg.slogdet(c.P)[1] + c.const
    r = results["CP"]
    print("CP: log evidence %.4f against %.4f, se %.4g; k-hat %.4f" % (r["vi_log_evidence"], evidence, r["vi_log_evidence_se"],
                                                                      r["vi_pareto_k"]))
    assert abs(r["vi_log_evidence"] - evidence) <= 5.0 * r["vi_log_evidence_se"]


def test_ncp_is_further_from_the_posterior_than_cp(runs):
    """k-hat separates the parameterisations at the FITTED q as well: the float64 reference pipeline on the oracle's own
    fits shows NCP - CP = 0.33 (tests/test_vicheck_host.py: test_fitted_q_separates_cp_from_ncp holds it above 0.2), so
    the order is asserted here."""
    _, results = runs
    print("k-hat: CP %.4f, NCP %.4f, cVIP %.4f" % tuple(results[m]["vi_pareto_k"] for m in ("CP", "NCP", "cVIP")))
    assert results["NCP"]["vi_pareto_k"] > results["CP"]["vi_pareto_k"]


@pytest.mark.parametrize("method", sorted(FILES))
def test_elbo_of_the_final_parameters_is_the_fits(runs, method):
    """The density the check evaluates is the one the fit optimised (cVIP above all: the learned a with the b the kernel
    read): the ELBO of the final parameters agrees with the optimiser's own figure within the bound of the module
    docstring.  The same cVIP run evaluated under NCP's (a, b) misses it by a wide margin (the commit message has the figure)."""
    _, results = runs
    r = results[method]
    gap = abs(r["vi_elbo_final"] - r["elbo"])
    bound = 4.0 * r["estimated_elbo_std"] + 6.0 * r["vi_elbo_final_se"]
    print("%s: |vi_elbo_final - elbo| = %.4g, bound %.4g (elbo %.4f +- %.4g, vi_elbo_final %.4f +- %.4g), k-hat %.4f" % (
        method, gap, bound, r["elbo"], r["estimated_elbo_std"], r["vi_elbo_final"], r["vi_elbo_final_se"], r["vi_pareto_k"]))
    assert gap <= bound


def test_existing_json_route_gives_the_same_bits(runs, tmp_path, monkeypatch, capsys):
    """A directory whose JSON was written without the flag: the second run adds the keys without refitting, and they are
    the bits of a run with the flag from the start (the fit is bitwise reproducible; JSON round-trips float32)."""
    from autoreparam_amd import analyze, inference, main as cli
    root, results = runs
    late = str(tmp_path / "late")
    plain = _cli(COMMON + ["--method=CP", "--results_dir=" + late])
    path = os.path.join(late, "CP_tied.json")
    assert not [k for k in plain if k.startswith("vi_")] and not os.path.exists(path[:-5] + "_vicheck.npz")
    for key in plain:
        if key != "variational_fit_time_secs":
            assert json.loads(json.dumps(plain[key])) == results["CP"][key], key            # nothing changes without the flag

    def never(*a, **k):
        raise AssertionError("the stored fit must not be refitted")
    monkeypatch.setattr(inference, "find_best_learning_rate", never)
    _cli(COMMON + ["--method=CP", "--results_dir=" + late, "--vi_diagnostics"])
    r = json.load(open(path))
    assert set(r) - set(plain) == set(cli.VI_CHECK_KEYS)
    for key in cli.VI_CHECK_KEYS:
        if key != "vi_check_time_sec":
            assert r[key] == results["CP"][key], key
    with np.load(path[:-5] + "_vicheck.npz") as a, np.load(os.path.join(root, "CP_tied_vicheck.npz")) as b:
        assert sorted(a.files) == sorted(b.files)
        assert all(a[n].dtype == b[n].dtype and a[n].tobytes() == b[n].tobytes() for n in a.files)
    capsys.readouterr()
    assert _cli(COMMON + ["--method=CP", "--results_dir=" + late, "--vi_diagnostics"]) is None     # the keys are there: skipped
    assert "Skipping" in capsys.readouterr().out
    analyze.main(["--results_dir=" + os.path.dirname(late), "--model=late", "--vi"])
    assert "CP_tied: Pareto k-hat" in capsys.readouterr().out
