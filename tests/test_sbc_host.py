"""CPU: the host side of simulation-based calibration (--inference=SBC).  diagnostics.sbc_summary under the null (its
p-value and its two z figures are calibrated), on three known faults and on the permuted control, on ties and on a
replicate left out; tests/sbc_ref.py's fold on a hand-made case; ModelSpec.with_observations for every model with data;
every refusal of sbc.check_sbc through main.main, before any device call; the ABI lists."""
import math
import os
import re

import numpy as np
import pytest

import sbc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS_WITH_DATA = (("8schools", None), ("radon", "MN"), ("radon", "MA"), ("radon_stddvs", "MN"), ("electric", None),
                    ("time_series", None), ("german_credit_lognormalcentered", None), ("german_credit_gammascale", None),
                    ("election", None))


def summary_of(draws, truth, names=None):
    from autoreparam_amd import diagnostics
    ref = sbc_ref.fold(draws, truth)
    return diagnostics.sbc_summary(ref["counts"], ref["sums"], np.shape(draws)[1], ref["left_out"], names)


def test_calibrated_under_the_null():
    """2 000 experiments of N = 256 replicates with ranks uniform on 0 ... 256 -- one quantity each, handed to one call as
    2 000 columns, which sbc_summary treats independently.  Four standard errors at 2 000 experiments around the nominal
    values: 0.05 +- 4 * 0.005 for the share of p < 0.05, 1 +- 4 * 0.016 for the sd of a z figure."""
    from autoreparam_amd import diagnostics
    E, N, L = 2000, 256, 256
    rng = np.random.default_rng(20181)
    counts = np.zeros((N, E, 2), np.int64)
    counts[:, :, 0] = rng.integers(0, L + 1, size=(N, E))
    s = diagnostics.sbc_summary(counts, np.zeros((N, E, 2)), L)
    share = float(np.mean(s.ks_p < 0.05))
    sd_mean, sd_var = float(np.std(s.rank_mean_z, ddof=1)), float(np.std(s.rank_var_z, ddof=1))
    print("null: share of ks_p < 0.05 %.4f, sd of rank_mean_z %.4f, of rank_var_z %.4f" % (share, sd_mean, sd_var))
    assert 0.03 <= share <= 0.07
    assert 0.93 <= sd_mean <= 1.07 and 0.93 <= sd_var <= 1.07
    assert abs(float(np.mean(s.rank_mean_z))) < 4.0 / math.sqrt(E) and abs(float(np.mean(s.rank_var_ratio)) - 1.0) < 0.01


@pytest.fixture(scope="module")
def faults():
    """N = 1 024 truths N(0, 1) and L = 256 draws per replicate from three wrong posteriors"""
    N, L = 1024, 256
    rng = np.random.default_rng(7)
    truth = rng.standard_normal((N, 1)).astype(np.float32)
    z = rng.standard_normal((N, L, 1)).astype(np.float32)
    return {"shifted": summary_of(z + np.float32(0.5), truth), "narrow": summary_of(z * np.float32(0.7), truth),
            "wide": summary_of(z * np.float32(1.5), truth)}


def test_known_faults(faults):
    """Against truths N(0, 1): draws N(0.5, 1) sit above the truth -- E u = Phi(-0.5 / sqrt 2) = 0.362, so
    rank_mean_z = (0.362 - 0.5) sqrt(12 * 1024) = -15; draws N(0, 0.7^2) are too narrow (a U-shaped histogram), draws
    N(0, 1.5^2) too wide"""
    s = faults["shifted"]
    expected = (0.5 * math.erfc(0.5 / 2.0) - 0.5) * math.sqrt(12 * 1024)
    print("shifted: rank_mean_z %.2f (expected %.2f)" % (s.rank_mean_z[0], expected))
    assert s.rank_mean_z[0] < -10 and abs(s.rank_mean_z[0] - expected) < 4.0 and s.ks_p[0] < 1e-6
    assert abs(s.post_z_mean[0] - 0.5) < 0.2
    s = faults["narrow"]
    assert s.rank_var_ratio[0] > 1 and s.rank_var_z[0] > 4 and s.post_z_sd[0] > 1.2
    s = faults["wide"]
    assert s.rank_var_ratio[0] < 1 and s.rank_var_z[0] < -4 and s.post_z_sd[0] < 0.8


def test_permuted_control():
    """Draws N(c_r, 0.2^2) around centres that know nothing of the truths: the ranks pile up at both ends"""
    N, L = 64, 256
    rng = np.random.default_rng(11)
    truth = rng.standard_normal((N, 1)).astype(np.float32)
    centre = rng.standard_normal((N, 1, 1)).astype(np.float32)
    s = summary_of(centre + np.float32(0.2) * rng.standard_normal((N, L, 1)).astype(np.float32), truth)
    print("permuted control: ks_p %.3g" % s.ks_p[0])
    assert s.ks_p[0] < 1e-4 and s.rank_var_ratio[0] > 1


def test_ties_and_the_mid_rank():
    from autoreparam_amd import diagnostics
    draws = np.array([[[1.0, 5.0, 0.0], [2.0, 5.0, -0.0], [2.0, 5.0, 0.0], [3.0, 5.0, 1.0]]] * 2, np.float32)   # [2, 4, 3]
    truth = np.array([[2.0, 5.0, 0.0], [3.0, 5.0, -0.0]], np.float32)
    ref = sbc_ref.fold(draws, truth)
    assert ref["counts"].tolist() == [[[1, 2], [0, 4], [0, 3]], [[3, 1], [0, 4], [0, 3]]]
    assert ref["sums"][0, 0].tolist() == [0.0, 2.0] and ref["sums"][1, 0].tolist() == [-4.0, 6.0]
    s = diagnostics.sbc_summary(ref["counts"], ref["sums"], 4, ref["left_out"], ["a", "b", "c"])
    assert s.u[:, 0].tolist() == [(1 + 1 + 0.5) / 5.0, (3 + 0.5 + 0.5) / 5.0]
    assert s.u[:, 1].tolist() == [0.5, 0.5] and s.constant.tolist() == [False, True, False]      # a constant column: u = 1/2
    assert s.replications == 2 and s.left_out == 0 and s.draws == 4 and s.names == ["a", "b", "c"]
    assert s.post_bias[1, 0] == -1.0 and s.post_sd[1, 0] == pytest.approx(math.sqrt((6.0 - 16.0 / 4) / 3))
    assert s.post_z[1, 0] == pytest.approx(-1.0 / math.sqrt(2.0 / 3.0))
    one = diagnostics.sbc_summary(ref["counts"], ref["sums"], 1)
    assert np.isnan(one.post_sd).all()                                                          # L = 1: no sd


def test_a_replicate_left_out_enters_nothing():
    from autoreparam_amd import diagnostics
    rng = np.random.default_rng(3)
    draws = rng.standard_normal((9, 16, 2)).astype(np.float32)
    truth = rng.standard_normal((9, 2)).astype(np.float32)
    draws[4, 15, 1] = np.inf
    truth[7, 0] = np.nan
    ref = sbc_ref.fold(draws, truth)
    assert ref["left_out"].tolist() == [0, 0, 0, 0, 1, 0, 0, 1, 0] and ref["n_left_out"] == 2
    assert not ref["counts"][[4, 7]].any() and not ref["sums"][[4, 7]].any()
    s = diagnostics.sbc_summary(ref["counts"], ref["sums"], 16, ref["left_out"])
    keep = [0, 1, 2, 3, 5, 6, 8]
    t = summary_of(draws[keep], truth[keep])
    assert s.replications == 7 and s.left_out == 2 and np.isnan(s.u[[4, 7]]).all() and np.isnan(s.post_z[[4, 7]]).all()
    for name in ("ks", "ks_p", "rank_mean_z", "rank_var_ratio", "rank_var_z", "post_z_mean", "post_z_sd"):
        assert np.array_equal(getattr(s, name), getattr(t, name)), name
    assert np.array_equal(s.u[keep], t.u)
    none = diagnostics.sbc_summary(ref["counts"], ref["sums"], 16, np.ones(9))
    assert none.replications == 0 and np.isnan(none.ks).all() and np.isnan(none.ks_p).all()


def test_kolmogorov_helpers():
    """Kolmogorov's distribution at two tabulated points; the distance is the one behind the PIT calibration"""
    from autoreparam_amd import diagnostics
    n = 10 ** 8                                                  # (Stephens' correction is then below 2e-5)
    assert diagnostics.kolmogorov_p_value(1.3581 / math.sqrt(n), n) == pytest.approx(0.05, abs=2e-4)
    assert diagnostics.kolmogorov_p_value(1.0 / math.sqrt(n), n) == pytest.approx(0.2700, abs=2e-4)
    assert diagnostics.kolmogorov_p_value(0.2 / math.sqrt(n), n) == 1.0 and diagnostics.kolmogorov_p_value(1.0, 100) < 1e-80
    u = np.array([0.1, 0.4, 0.45, 0.9])
    assert diagnostics.kolmogorov_distance(u) == pytest.approx(0.3)          # at 0.45: F_n = 0.75
    assert diagnostics._pit_calibration(u)[0] == diagnostics.kolmogorov_distance(u)


@pytest.mark.parametrize("name,dataset", MODELS_WITH_DATA)
def test_with_observations(name, dataset):
    from autoreparam_amd import models
    spec = models.spec_by_name(name, dataset)
    before = {k: np.array(v, copy=True) for k, v in spec.raw.items()}
    same = spec.with_observations(np.asarray(spec.raw["y"], np.float64).reshape(-1))
    assert same is not spec and same.raw is not spec.raw

    def dataset_arrays(s):
        d, keep = s.dataset()
        return [int(getattr(d, f)) for f in ("model", "n_obs", "n_groups", "n_features")], keep
    head, keep = dataset_arrays(spec)
    head2, keep2 = dataset_arrays(same)
    assert head == head2 and len(keep) == len(keep2)
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(keep, keep2))
    for table in ("observation_table", "site_table"):
        a, b = getattr(spec, table)(), getattr(same, table)()
        for field, u, v in zip(a._fields, a, b):
            assert np.asarray(u).dtype == np.asarray(v).dtype and np.array_equal(u, v), (table, field)
    assert list(same.observed) == list(spec.observed)
    for key in spec.observed:
        assert same.observed[key].shape == spec.observed[key].shape and same.observed[key].dtype == spec.observed[key].dtype
        assert np.array_equal(same.observed[key], spec.observed[key])
    # another y: only y differs, and the original is unchanged
    y = np.asarray(spec.raw["y"], np.float64).reshape(-1)
    other = spec.with_observations(1.0 - y)
    assert other.raw["y"].shape == spec.raw["y"].shape and other.raw["y"].dtype == spec.raw["y"].dtype
    assert all(other.raw[k] is spec.raw[k] for k in spec.raw if k != "y")
    a, b = spec.observation_table(), other.observation_table()
    for field, u, v in zip(a._fields, a, b):
        if field == "y":
            assert np.array_equal(v, (1.0 - y).astype(spec.raw["y"].dtype).astype(np.float32).reshape(-1)) and not np.array_equal(u, v)
        else:
            assert np.array_equal(u, v), field
    assert all(np.array_equal(u, v) for u, v in zip(spec.site_table(), other.site_table()))
    assert other.part_names == spec.part_names and other.D == spec.D and other.options == spec.options
    assert all(np.array_equal(before[k], spec.raw[k]) for k in before) and set(before) == set(spec.raw)
    with pytest.raises(ValueError, match="observations are required"):
        spec.with_observations(y[:-1])


def test_with_observations_refuses_the_funnel_and_get_model_by_name_is_unchanged():
    from autoreparam_amd import models
    with pytest.raises(ValueError, match="no observations"):
        models.spec_by_name("neals_funnel").with_observations([])
    cfg = models.get_model_by_name("8schools")
    again = models.model_config_for(cfg.model)
    assert again.model is cfg.model and again.model_args == [] and again.observed_data is cfg.model.observed
    assert again.bijectors_fn is None and all(callable(f) for f in again[3:7])


REFUSALS = (
    (["--method=cVIP"], "--method must be CP or NCP, not cVIP .*cVIP, dVIP and i need a stored fit per data set"),
    (["--method=dVIP"], "--method must be CP or NCP"),
    (["--method=i"], "--method must be CP or NCP"),
    (["--model=neals_funnel"], "--model=neals_funnel has no observations"),
    (["--num_leapfrog_steps=0"], "--num_leapfrog_steps is required"),
    (["--sbc_replications=7"], "--sbc_replications must lie in 8 ... 16384, not 7"),
    (["--sbc_replications=16385"], "--sbc_replications must lie in 8 ... 16384"),
    (["--sbc_steps=0"], "--sbc_steps must lie in 1 ... 20"),
    (["--sbc_steps=21"], "--sbc_steps must lie in 1 ... 20 .*not 21"),
)
BASE = ["--inference=SBC", "--model=radon", "--dataset=MA", "--method=NCP", "--num_leapfrog_steps=4", "--num_samples=20",
        "--sbc_replications=64"]


def no_device(monkeypatch):
    """Every way to the device raises: a refusal that comes first is a refusal before any device call"""
    from autoreparam_amd import _lib, diagnostics, engine, models

    def never(*a, **k):
        raise AssertionError("nothing may be drawn, launched or loaded before the refusal")
    monkeypatch.setattr(_lib, "lib", never)
    monkeypatch.setattr(engine, "Engine", never)
    monkeypatch.setattr(diagnostics, "site_prior_draws", never)
    monkeypatch.setattr(models, "get_model_by_name", never)
    return never


@pytest.mark.parametrize("extra,message", REFUSALS)
def test_refusals_come_before_any_device_call(monkeypatch, tmp_path, extra, message):
    from autoreparam_amd import main, sbc
    from autoreparam_amd.flags import FlagValues
    no_device(monkeypatch)
    args = BASE + ["--results_dir=" + str(tmp_path / "out")] + extra
    with pytest.raises(ValueError, match=message):
        main.main(args, flags=FlagValues())
    assert not os.path.exists(str(tmp_path / "out"))
    f = FlagValues()
    f.parse(args)
    with pytest.raises(ValueError, match=message):
        sbc.check_sbc(f)


def test_the_missing_leapfrog_count_a_sharded_job_and_the_passing_case(monkeypatch, tmp_path):
    from autoreparam_amd import main, sbc
    from autoreparam_amd.flags import FlagValues
    never = no_device(monkeypatch)
    f = FlagValues()
    assert f.sbc_replications == 256 and f.sbc_steps == 1
    f.parse([a for a in BASE if not a.startswith("--num_leapfrog_steps")])
    with pytest.raises(ValueError, match="--num_leapfrog_steps is required .*no tuning runs per replicate"):
        main.main([], flags=f)
    f.parse(BASE)
    sbc.check_sbc(f)                                             # the job of tests/test_gpu_sbc_cli.py passes
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="--inference=SBC runs in one process: WORLD_SIZE=2"):
        main.main([], flags=f)
    monkeypatch.delenv("WORLD_SIZE")
    f.parse(["--inference=HMC", "--sbc_replications=1", "--method=i"])
    sbc.check_sbc(f)                                             # another --inference: the SBC flags are not looked at
    f.parse(["--count_in_leapfrog_steps", "--inference=SBC", "--method=CP", "--sbc_replications=8", "--sbc_steps=6"])
    with pytest.raises(ValueError, match="--sbc_steps must lie in 1 ... 5"):     # 20 samples / 4 leapfrog steps
        sbc.check_sbc(f)
    assert never is not None


def test_a_wide_model_is_refused_before_anything_is_drawn(monkeypatch, tmp_path):
    from autoreparam_amd import sbc
    from autoreparam_amd.flags import FlagValues
    no_device(monkeypatch)
    f = FlagValues()
    f.parse(BASE)
    cfg = type("Cfg", (), {"model": type("Spec", (), {"D": 256})()})()
    with pytest.raises(ValueError, match="256 elements, more than the 255"):
        sbc.run_sbc(cfg, str(tmp_path), str(tmp_path / "NCP_tied.json"), f)
    assert os.listdir(str(tmp_path)) == []


def test_an_existing_report_is_not_run_again(monkeypatch, tmp_path, capsys):
    from autoreparam_amd import sbc
    from autoreparam_amd.flags import FlagValues
    no_device(monkeypatch)
    f = FlagValues()
    f.parse(BASE)
    (tmp_path / "NCP_tied_sbc.json").write_text("{}")
    assert sbc.run_sbc(None, str(tmp_path), str(tmp_path / "NCP_tied.json"), f) is None
    assert "Already ran experiment SBC-NCP" in capsys.readouterr().out


def test_keys_line_and_warning_from_a_summary():
    """sbc_keys, the printed line and the warning on the three faults as three quantities of one report"""
    from autoreparam_amd import diagnostics, sbc
    N, L = 256, 64
    rng = np.random.default_rng(5)
    truth = rng.standard_normal((N, 4)).astype(np.float32)
    z = rng.standard_normal((N, L, 4)).astype(np.float32)
    draws = z * np.array([1.0, 1.0, 0.5, 2.0], np.float32) + np.array([0.0, 1.0, 0.0, 0.0], np.float32)
    s = summary_of(draws, truth, ["fine", "high", "narrow", "wide"])
    keys = sbc.sbc_keys(s)
    assert set(keys) < set(sbc.SBC_KEYS) and keys["sbc_replications"] == N and keys["sbc_replications_left_out"] == 0
    assert keys["sbc_draws"] == L and keys["sbc_quantities"] == 4 and keys["sbc_p_threshold"] == 0.01 / 4
    assert sorted(keys["sbc_miscalibrated_elements"]) == ["high", "narrow", "wide"]
    assert keys["sbc_p_min"] == float(np.min(s.ks_p)) and keys["sbc_ks_max"] == float(np.max(s.ks))
    assert keys["sbc_rank_mean_z_max_abs_element"] == "high" and keys["sbc_rank_mean_z_max_abs"] == abs(float(s.rank_mean_z[1]))
    assert keys["sbc_rank_var_ratio_max_element"] == "narrow" and keys["sbc_rank_var_ratio_min_element"] == "wide"
    assert keys["sbc_post_z_sd_max"] == float(np.max(s.post_z_sd)) and keys["sbc_post_z_sd_min"] == float(np.min(s.post_z_sd))
    line, warning = sbc.sbc_line(keys, s), sbc.sbc_warning(keys, s)
    assert "worst %s with p = " % keys["sbc_p_min_element"] in line and "256 replicates (0 left out), 64 draws each" in line
    assert "high (p = " in warning and "shifted above the truth" in warning and "too narrow" in warning and "too wide" in warning
    assert "fine" not in warning and "a convention" in warning
    fine = summary_of(z[:, :, :1], truth[:, :1], ["fine"])
    assert sbc.sbc_warning(sbc.sbc_keys(fine), fine) is None
    none = diagnostics.sbc_summary(np.zeros((8, 2, 2)), np.zeros((8, 2, 2)), 4, np.ones(8), ["a", "b"])
    keys = sbc.sbc_keys(none)
    assert keys["sbc_p_min"] is None and keys["sbc_p_min_element"] is None and keys["sbc_miscalibrated_elements"] == []
    assert "worst None" in sbc.sbc_line(keys, none)


def test_symbol_is_declared_and_listed():
    from autoreparam_amd import _lib
    src = open(os.path.join(ROOT, "include", "autoreparam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)                          # as tests/test_abi.py reads the header
    declared = sorted(set(re.findall(r"\b(arp_[a-z_0-9]+)\s*\(", src)))
    assert "arp_sbc_fold" in declared and "arp_sbc_fold" in _lib.SYMBOLS and sorted(declared) == sorted(_lib.SYMBOLS)
    assert os.path.exists(os.path.join(ROOT, "autoreparam_amd", "csrc", "sbc.hip"))


def test_wrapper_refuses_what_the_kernel_refuses(monkeypatch):
    import torch
    from autoreparam_amd import _lib, diagnostics

    def never(*a, **k):
        raise AssertionError("no call may be made")
    monkeypatch.setattr(_lib, "call", never)
    with pytest.raises(ValueError, match="on the GPU"):
        diagnostics.sbc_fold(torch.zeros(2, 3, 4), torch.zeros(2, 4))
    with pytest.raises(ValueError, match="on the GPU"):
        diagnostics.sbc_fold(np.zeros((2, 3, 4), np.float32), np.zeros((2, 4), np.float32))
