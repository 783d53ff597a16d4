"""CPU: the host layer of the variational-fit check (--vi_diagnostics).  (a) the flag, its refusals, what run_vi adds to
the result file with the device half replaced by the float64 reference, and the route from an existing file; (b) the known
answer: the reference pipeline (tests/vicheck_ref.py) on the float64 oracle's log joint of radon MN, whose posterior is
exactly normal, at the KL-optimal mean-field normal (loc = the posterior mean, scale_d = P_dd^-1/2), through
diagnostics.vi_check_summary.

Figures of (b) at R = 65 536, seed 2018 (the bounds are the issue's):
  CP   k-hat 0.553 against 0.7; log evidence off by 1.3 se of 5; KL 0.3355 against the exact 0.3428, 0.9 se of 5; largest
       |gradient| / se 2.89 of 6 (loc), 2.21 (scale); score gap off by at most 0.6 % of 5 %; corrected sd off by at most
       2.3 % of 5 % (q's own sd is 15.5 % short); with loc moved, largest |gradient - closed form| / se 2.89 of 6
  NCP  k-hat 0.904 against its threshold 0.7"""
import json
import math
import os

import numpy as np
import pytest

import vicheck_ref as vr

from vicheck_ref import Case, check_known_answer, R


@pytest.fixture(scope="module")
def cp(oracle_lib):
    c = Case(oracle_lib, "CP")
    c.pipe, c.summary = c.run()
    return c


# ---- (b) the known answer ----
def test_cp_known_answer(cp):
    check_known_answer(cp, cp.summary)
    assert cp.pipe.mask.sum() == 0 and cp.summary.tail_length == 768
    # is_mean / is_sd are the same two figures in centred coordinates: CP's coordinates are the centred ones
    np.testing.assert_allclose(cp.summary.is_sd, cp.summary.sd_ratio * cp.scale, rtol=1e-6)
    np.testing.assert_allclose(cp.summary.is_mean, cp.loc + cp.summary.loc_shift * cp.scale, rtol=0, atol=1e-6)


def test_cp_moved_loc_shows_in_the_gradient(cp):
    """loc moved by +0.5 sd in one element: elbo_grad_loc = -scale * P (loc - mean), within 6 se in every element."""
    loc = cp.loc.copy()
    loc[7] += np.float32(0.5) * cp.scale[7]
    _, s = cp.run(loc)
    sq = cp.scale.astype(np.float64)
    want = -sq * (cp.P @ (loc.astype(np.float64) - cp.mean))
    t = np.abs(s.elbo_grad_loc - want) / s.elbo_grad_loc_se
    print("largest |gradient - closed form| / se %.2f; the moved element reads %.4f (closed form %.4f)" % (t.max(), s.elbo_grad_loc[7], want[7]))
    assert t.max() <= 6.0
    assert abs(want[7] + 0.5) < 1e-3 and abs(s.elbo_grad_loc[7] + 0.5) <= 6.0 * s.elbo_grad_loc_se[7]


def test_ncp_is_far_and_says_so(oracle_lib):
    from autoreparam_amd import main
    c = Case(oracle_lib, "NCP")
    _, s = c.run()
    print("NCP k-hat %.4f (threshold %.4f)" % (s.pareto_k, s.pareto_k_threshold))
    assert s.pareto_k > s.pareto_k_threshold
    keys = main.vi_check_keys(s, R, 0, main.element_names(c.sp))
    text = main.vi_check_warning(keys)
    assert text and "far from the posterior" in text and "unreliable" in text and "--method" in text


def test_fitted_q_separates_cp_from_ncp(oracle_lib):
    """Not only at the optimal q: at the q the float64 oracle's own optimiser ends in (one learning rate, the reference's
    3 000 steps of 256 draws) k-hat reads 0.569 for CP and 0.900 for NCP.  The gap above 0.2 is what lets
    tests/test_gpu_vicheck_cli.py assert the order on the device's fits."""
    from autoreparam_amd import diagnostics
    k = {}
    for kind in ("CP", "NCP"):
        c = Case(oracle_lib, kind)
        rs = np.random.RandomState(3)
        loc, rho = 1e-2 * rs.randn(1, c.sp.D), np.full((1, c.sp.D), -2.0)
        c.orc.vi_run(c.a, c.b, [0.05], loc, rho, None, 3000, 256, seed=3)
        c.loc, c.scale = loc[0].astype(np.float32), np.log1p(np.exp(rho[0])).astype(np.float32)
        k[kind] = c.run()[1].pareto_k
    print("fitted q: k-hat CP %.4f, NCP %.4f" % (k["CP"], k["NCP"]))
    assert k["NCP"] - k["CP"] > 0.2


def test_no_warning_below_the_threshold_and_one_without_a_fit(cp):
    from autoreparam_amd import main
    keys = main.vi_check_keys(cp.summary, R, 0, main.element_names(cp.sp))
    assert main.vi_check_warning(keys) is None
    keys["vi_pareto_k"] = None
    assert "not fitted" in main.vi_check_warning(keys)


def test_summary_of_an_empty_check_is_null():
    from autoreparam_amd import diagnostics
    D = 3
    s = diagnostics.vi_check_summary(np.zeros((D, 9)), np.array([0.0, 0.0, 0.0, 0.0, np.inf]),
                                     np.array([np.nan, np.inf, np.nan, np.nan, 0.0, np.nan, np.nan, 0.0]), np.zeros(D), np.ones(D),
                                     np.zeros(D), 0.0)
    assert s.draws == 0 and s.pareto_k is None and s.elbo_final is None and np.isnan(s.sd_ratio).all()


def test_summary_definitions_on_a_hand_made_case():
    """Two kept draws, one element: every statistic from its definition."""
    from autoreparam_amd import diagnostics
    w = np.array([1.0, 0.25])
    z, u, c, ll = np.array([0.5, -1.0]), np.array([-0.4, 1.1]), np.array([0.2, -0.3]), np.array([3.0, 3.0 + math.log(4.0)])
    elem = np.array([[u.sum(), (u * u).sum(), (u * z).sum(), ((u * z) ** 2).sum(), ((u + z) ** 2).sum(), (w * z).sum(),
                      (w * z * z).sum(), (w * c).sum(), (w * c * c).sum()]])
    tot = np.array([2.0, w.sum(), (w * w).sum(), ll.sum(), ll.min()])
    out8 = np.array([np.nan, np.inf, np.nan, np.var(ll, ddof=1), 0.0, np.nan, np.nan, 2.0])
    s = diagnostics.vi_check_summary(elem, tot, out8, [1.0], [2.0], [10.0], 7.0)
    assert s.pareto_k is None and s.tail_length == 0 and s.draws == 2
    assert s.elbo_final == pytest.approx(-ll.mean() + 7.0) and s.elbo_final_se == pytest.approx(math.sqrt(np.var(ll, ddof=1) / 2))
    assert s.is_ess == pytest.approx(1.25 ** 2 / (1 + 0.0625))
    assert s.log_evidence == pytest.approx(math.log(np.mean(np.exp(-ll))) + 7.0)
    assert s.log_evidence_se == pytest.approx(math.sqrt(1 / s.is_ess - 0.5))
    assert s.kl_estimate == pytest.approx(s.log_evidence - s.elbo_final)
    assert s.kl_estimate_se == pytest.approx(math.hypot(s.log_evidence_se, s.elbo_final_se))
    assert s.elbo_grad_loc[0] == pytest.approx(u.mean()) and s.elbo_grad_loc_se[0] == pytest.approx(np.std(u, ddof=1) / math.sqrt(2))
    assert s.elbo_grad_scale[0] == pytest.approx((u * z).mean() + 1.0)
    assert s.elbo_grad_scale_se[0] == pytest.approx(np.std(u * z, ddof=1) / math.sqrt(2))
    assert s.score_gap[0] == pytest.approx(math.sqrt(((u + z) ** 2).mean()))
    m = (w * z).sum() / w.sum()
    assert s.loc_shift[0] == pytest.approx(m) and s.sd_ratio[0] == pytest.approx(math.sqrt((w * z * z).sum() / w.sum() - m * m))
    mc = (w * c).sum() / w.sum()
    assert s.is_mean[0] == pytest.approx(10.0 + mc) and s.is_sd[0] == pytest.approx(math.sqrt((w * c * c).sum() / w.sum() - mc * mc))


# ---- the reference itself ----
def test_reference_normals_are_standard_and_offsets_are_rows():
    z = vr.normals(5, np.arange(40000, dtype=np.uint64), 11)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01 and np.abs(np.corrcoef(z.T) - np.eye(5)).max() < 0.03
    part = vr.normals(5, np.uint64(123) + np.arange(10, dtype=np.uint64), 11)
    assert np.array_equal(part, z[123:133])
    assert np.array_equal(vr.normals(3, np.arange(8, dtype=np.uint64), 11), z[:8, :3])       # (an element's draw does not depend on D)


def test_reference_weights_scatter_back_through_the_stable_order():
    ll = np.repeat(-np.arange(1.0, 61.0), 5).astype(np.float32)[::-1].copy()      # 300 draws in groups of five equal values
    out8, lw, tail = vr.weights_row(ll)
    assert out8[4] == 52 and tail.size == 52
    order = np.argsort(ll.astype(np.float64), kind="stable")
    assert np.array_equal(np.sort(tail), np.sort(order[:52]))
    raw = ll.astype(np.float64).min() - ll.astype(np.float64)
    rest = np.setdiff1d(np.arange(300), tail)
    assert np.array_equal(lw[rest], raw[rest])
    assert np.all(np.diff(lw[order[:52]]) <= 0) and lw[order[0]] <= 0.0           # the smoothed tail descends along the order
    mask = np.zeros(300, np.uint8)
    mask[::7] = 1
    _, lwm, tailm = vr.weights_row(ll, mask)
    assert np.all(np.isneginf(lwm[mask != 0])) and np.all(np.isfinite(lwm[mask == 0])) and not np.intersect1d(tailm, np.flatnonzero(mask)).size
    bad = ll.copy()
    bad[5] = np.inf
    _, lwb, tailb = vr.weights_row(bad, mask)
    assert np.all(np.isnan(lwb[mask == 0])) and np.all(np.isneginf(lwb[mask != 0])) and tailb.size == 0


# ---- (a) the flag, the refusals, run_vi ----
def test_flag_parses_and_draws_are_bounded():
    from autoreparam_amd import main
    from autoreparam_amd.flags import FlagValues
    f = FlagValues()
    assert f.vi_diagnostics is False and f.vi_check_draws == 65536
    f.parse(["--vi_diagnostics", "--vi_check_draws=2048"])
    assert f.vi_diagnostics is True and f.vi_check_draws == 2048
    main.check_vi_diagnostics(f)
    for bad in (1023, (1 << 20) + 1, 0, -5):
        g = FlagValues()
        g.parse(["--model=radon", "--dataset=MN", "--inference=VI", "--vi_diagnostics", "--vi_check_draws=%d" % bad])
        with pytest.raises(ValueError, match="vi_check_draws"):
            main.main([], flags=g)                                            # (before a model is loaded or a file is touched)
    for ok in (1024, 1 << 20):
        g = FlagValues()
        g.parse(["--vi_diagnostics", "--vi_check_draws=%d" % ok])
        main.check_vi_diagnostics(g)
    g = FlagValues()
    g.parse(["--vi_check_draws=5"])
    main.check_vi_diagnostics(g)                                              # without the flag the value is not read


class FakeEngine(object):
    def __init__(self):
        self.ab = None

    def set_param(self, which, ab):
        self.ab = (which, ab)


@pytest.fixture
def fake_vi(monkeypatch, cp):
    """run_vi with the fit and the device half replaced: the fit is the known-answer q, the check the reference's."""
    from autoreparam_amd import diagnostics, inference, main, models, util
    sp = cp.sp
    calls = {"fit": 0, "check": 0, "engine": FakeEngine()}
    vp = {}
    for k, name in enumerate(sp.part_names):
        lo, hi = sp.offsets[k], sp.offsets[k + 1]
        vp[name + "_loc"] = cp.loc[lo:hi].reshape(sp.part_shapes[k])
        vp[name + "_scale"] = cp.scale[lo:hi].reshape(sp.part_shapes[k])

    def fit(elbo, variational_parameters, **kw):
        calls["fit"] += 1
        timeline = list(-1000.0 + 0.01 * np.arange(40))
        return np.float64(-999.7), timeline, 0.1, util.get_approximate_step_size(vp, num_leapfrog_steps=1), vp, None

    def check(eng, loc, scale, which=0, draws=65536, seed=0):
        calls["check"] += 1
        calls["args"] = (np.array(loc), np.array(scale), which, draws, seed)
        assert eng is calls["engine"] and eng.ab is not None
        p = cp.pipe
        return diagnostics.ViCheck(p.elem, p.tot, p.out8, p.e0.astype(np.float64), cp.const, int(p.mask.sum()), -p.ll, p.lw)
    monkeypatch.setattr(inference, "find_best_learning_rate", fit)
    monkeypatch.setattr(diagnostics, "vi_check", check)
    monkeypatch.setattr(main._engine, "engine_for", lambda spec, device=None: calls["engine"])
    calls["config"] = models.get_model_by_name("radon", dataset="MN")
    return calls


def _flags(*extra):
    from autoreparam_amd.flags import FlagValues
    f = FlagValues()
    f.parse(["--model=radon", "--dataset=MN", "--inference=VI", "--method=CP", "--seed=3", "--device=cpu"] + list(extra))
    return f


def test_run_vi_adds_exactly_the_keys(fake_vi, cp, tmp_path):
    from autoreparam_amd import main
    plain, checked = str(tmp_path / "plain.json"), str(tmp_path / "checked.json")
    a = main.run_vi(fake_vi["config"], str(tmp_path), plain, _flags())
    assert fake_vi["check"] == 0 and not [k for k in a if k.startswith("vi_")] and not os.path.exists(plain[:-5] + "_vicheck.npz")
    b = main.run_vi(fake_vi["config"], str(tmp_path), checked, _flags("--vi_diagnostics"))
    assert fake_vi["fit"] == 2 and fake_vi["check"] == 1
    assert set(b) - set(a) == set(main.VI_CHECK_KEYS) and set(a) <= set(b)
    for k in a:
        if k != "variational_fit_time_secs":
            assert a[k] == b[k], k
    with open(checked) as f:
        on_disk = json.load(f)
    assert on_disk == json.loads(json.dumps(b))
    loc, scale, which, draws, seed = fake_vi["args"]
    assert np.array_equal(loc, cp.loc) and np.array_equal(scale, cp.scale) and loc.dtype == np.float32 and which == 0
    assert draws == 65536 and seed == (3 * 0x9E3779B97F4A7C15 + main.VI_CHECK_SEED) & 0xFFFFFFFFFFFFFFFF
    assert np.array_equal(fake_vi["engine"].ab[1][0], cp.a) and np.array_equal(fake_vi["engine"].ab[1][1], cp.b)
    s = cp.summary
    assert b["vi_check_draws"] == 65536 and b["vi_check_draws_left_out"] == 0 and b["vi_tail_length"] == 768
    assert b["vi_pareto_k"] == s.pareto_k and b["vi_elbo_final"] == s.elbo_final and b["vi_kl_estimate"] == s.kl_estimate
    names = main.element_names(cp.sp)
    at = int(np.abs(s.elbo_grad_loc).argmax())
    assert b["vi_elbo_grad_loc_max"] == s.elbo_grad_loc[at] and b["vi_elbo_grad_loc_max_element"] == names[at]
    assert b["vi_elbo_grad_loc_max_se"] == s.elbo_grad_loc_se[at]
    assert b["vi_sd_ratio_min"] == s.sd_ratio.min() and b["vi_sd_ratio_min_element"] == names[int(s.sd_ratio.argmin())]
    assert b["vi_sd_ratio_max"] == s.sd_ratio.max() and b["vi_score_gap_max"] == s.score_gap.max()
    assert all(b[k] is None or isinstance(b[k], (int, float, str)) for k in main.VI_CHECK_KEYS)
    with np.load(checked[:-5] + "_vicheck.npz") as z:
        for family in main.VI_CHECK_FAMILIES:
            for name, shape in zip(cp.sp.part_names, cp.sp.part_shapes):
                assert z["%s/%s" % (family, name)].shape == tuple(shape)
        assert z["log_ratio"].shape == (R,) and z["log_ratio"].dtype == np.float32 and z["log_weight"].shape == (R,)
        assert int(z["left_out"]) == 0
        assert np.array_equal(np.concatenate([z["sd_ratio/" + n].reshape(-1) for n in cp.sp.part_names]), s.sd_ratio)


def test_existing_json_is_checked_without_a_refit(fake_vi, tmp_path, capsys):
    from autoreparam_amd import main
    path = str(tmp_path / "CP.json")
    first = main.run_vi(fake_vi["config"], str(tmp_path), path, _flags())
    assert fake_vi["fit"] == 1 and fake_vi["check"] == 0
    assert main.run_vi(fake_vi["config"], str(tmp_path), path, _flags()) is None          # as before: skipped
    second = main.run_vi(fake_vi["config"], str(tmp_path), path, _flags("--vi_diagnostics"))
    assert fake_vi["fit"] == 1 and fake_vi["check"] == 1
    assert set(second) - set(first) == set(main.VI_CHECK_KEYS)
    assert all(second[k] == json.loads(json.dumps(first))[k] for k in first)
    with open(path) as f:
        assert json.load(f) == json.loads(json.dumps(second))
    loc, scale = fake_vi["args"][:2]
    assert loc.dtype == np.float32 and np.array_equal(loc, fake_vi["args"][0])
    capsys.readouterr()
    assert main.run_vi(fake_vi["config"], str(tmp_path), path, _flags("--vi_diagnostics")) is None   # the keys are there: skipped
    assert fake_vi["fit"] == 1 and fake_vi["check"] == 1 and "Skipping" in capsys.readouterr().out


def test_stored_fit_round_trips_to_the_same_float32(fake_vi, cp, tmp_path):
    """JSON round-trips float32 exactly: the q the existing-file route checks is bit for bit the fresh route's."""
    from autoreparam_amd import main
    path = str(tmp_path / "CP.json")
    main.run_vi(fake_vi["config"], str(tmp_path), path, _flags())
    with open(path) as f:
        loc, scale = main._fitted_q(cp.sp, json.load(f))
    assert np.array_equal(loc.view(np.uint32), cp.loc.view(np.uint32)) and np.array_equal(scale.view(np.uint32), cp.scale.view(np.uint32))


def test_analyze_prints_the_table(fake_vi, tmp_path, capsys):
    from autoreparam_amd import analyze, main
    os.makedirs(str(tmp_path / "radon_MN"))
    main.run_vi(fake_vi["config"], str(tmp_path / "radon_MN"), str(tmp_path / "radon_MN" / "CP.json"), _flags("--vi_diagnostics"))
    main.run_vi(fake_vi["config"], str(tmp_path / "radon_MN"), str(tmp_path / "radon_MN" / "NCP.json"), _flags())
    capsys.readouterr()
    analyze.main(["--results_dir=%s" % tmp_path, "--model=radon_MN", "--vi"])
    out = capsys.readouterr().out
    assert "CP: Pareto k-hat" in out and "NCP" not in out and "FAR" not in out and "65536 draws" in out
