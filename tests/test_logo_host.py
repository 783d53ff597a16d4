"""CPU: the host side of --loo_groups.  diagnostics.marginal_selection on the frozen data (the groups are group_selection's;
which models have a closed marginal form, and why the others do not) and on synthetic tables that break each of its
conditions; the refusals of the flag before anything touches a device, each naming it; the order of LOGO_KEYS and the null
paths; diagnostics.logo_summary against psis_ref.summary; the keys; the side file; analyze --loo and --logo_compare with
its refusals; and the self-check of the float64 reference of tests/logo_ref.py: the kernel's closed form, restated in
float64, agrees with scipy's multivariate_normal on the cases the GPU test runs."""
import collections
import json
import os

import numpy as np
import pytest

import logo_cases as cases
import logo_ref as lg
import psis_ref as pr

# (model, dataset, part): groups, marginal form
FROZEN = ((("radon", "MN", "m"), (85, True)), (("radon", "MA", "m"), (13, True)), (("radon_stddvs", "MN", "m"), (85, True)),
          (("8schools", None, "theta"), (8, True)), (("electric", None, "a"), (96, True)), (("electric", None, "b"), (4, True)),
          (("election", None, "a"), (51, False)))


@pytest.mark.parametrize("which, want", FROZEN, ids=["-".join(str(v) for v in w) for w, _ in FROZEN])
def test_marginal_selection_on_the_frozen_data(which, want):
    from autoreparam_amd import diagnostics, main, models
    model, dataset, part = which
    spec = models.spec_by_name(model, dataset)
    table, site = spec.observation_table(), spec.site_table()
    group_of, names, slope, elem, ok, why = diagnostics.marginal_selection(site, table, spec, part)
    ref_of, ref_names = diagnostics.group_selection(table, spec, part)
    assert np.array_equal(group_of, ref_of) and names == ref_names                 # the grouping rule has one definition
    assert (len(names), ok) == want and (why is None) == ok
    k = spec.part_names.index(part)
    lo, hi = int(spec.offsets[k]), int(spec.offsets[k + 1])
    assert elem.dtype == np.int32 and np.array_equal(elem, np.arange(lo, hi))
    assert slope.dtype == np.float32 and slope.shape == group_of.shape
    for n in range(group_of.size):                                                # the slope: the weights on the group's own element
        own = sum(float(w) for i, w in zip(table.idx[n], table.w[n]) if group_of[n] >= 0 and int(i) == lo + group_of[n])
        assert slope[n] == np.float32(own) and (slope[n] != 0) == (group_of[n] >= 0), n
    if ok:
        # the closed form's conditions, from the tables themselves: a Normal site nobody else reads, Normal data, no scale
        assert table.kind == 0 and np.all(np.asarray(site.form)[lo:hi] == models.SITE_NORMAL)
        assert not np.any((np.asarray(table.scale_idx) >= lo) & (np.asarray(table.scale_idx) < hi))
    else:
        assert "Bernoulli" in why and table.kind == 1
    # through to the keys: without a marginal form its six keys are null, the conditional ones are filled
    G, rs = len(names), np.random.RandomState(1)
    sizes = np.bincount(group_of[group_of >= 0], minlength=G)
    c = rs.randn(G, 8)
    c[sizes == 0] = np.nan
    keys = main.logo_keys(c, c + 1.0 if ok else None, part, names, int(np.sum(group_of < 0)), 8192, 0)
    assert tuple(keys) == main.LOGO_KEYS[:-1] and keys["logo_marginal"] is ok and keys["logo_groups"] == G
    assert keys["logo_groups_empty"] == int(np.sum(sizes == 0)) and keys["logo_observations_left_out"] == int(np.sum(group_of < 0))
    assert all((keys[name] is not None) == ok for name in main.LOGO_MARGINAL_KEYS)
    assert all(keys["logo_conditional_" + name] is not None for name in ("elpd", "elpd_se", "p", "pareto_k_max", "pareto_k_max_group"))
    json.dumps(keys)


def test_the_election_groups_are_counted_as_the_grouped_check_counts_them():
    from autoreparam_amd import diagnostics, models
    spec = models.spec_by_name("election")
    group_of, names, _, _, ok, why = diagnostics.marginal_selection(spec.site_table(), spec.observation_table(), spec, "a")
    sizes = np.bincount(group_of[group_of >= 0], minlength=len(names))
    assert int(np.sum(sizes == 0)) == 3 and int(np.sum(group_of < 0)) == 15 and not ok and why.startswith("the data are Bernoulli")


Spec = collections.namedtuple("Spec", ["name", "part_names", "part_shapes", "offsets"])
Table = collections.namedtuple("Table", ["kind", "idx", "w", "y", "scale_idx", "log_scale"])


def synthetic():
    """A state (mu, tau, t[0..2], child): t reads mu and tau; six Normal observations read t (one of them twice) and mu."""
    from autoreparam_amd import models
    spec = Spec("toy", ["mu", "tau", "t", "child"], [(), (), (3,), ()], [0, 1, 2, 5, 6])
    D = 6
    site = models.SiteTable(np.zeros(D, np.int32), np.zeros((D, 2), np.int32), np.zeros((D, 2)), np.zeros(D), np.zeros((D, 2), np.int32),
                            np.zeros((D, 2)), np.zeros(D), np.zeros(D), np.array([0, 1, 2, 2, 2, 3], np.int32))
    site.loc_w[2:5, 0], site.scale_idx[2:5, 0], site.scale_w[2:5, 0] = 1.0, 1, 1.0
    idx = np.array([[2, 0], [3, 0], [4, 4], [2, 0], [0, 0], [3, 0]], np.int32)
    w = np.array([[1.0, 0.5], [2.0, 0.5], [0.25, 0.5], [1.0, 0.0], [1.0, 0.0], [-1.5, 0.5]], np.float32)
    table = Table(0, idx, w, np.arange(6, dtype=np.float32), np.full(6, -1, np.int32), np.zeros(6, np.float32))
    return spec, site, table


def test_marginal_selection_refuses_what_has_no_closed_form():
    from autoreparam_amd import diagnostics, models
    spec, site, table = synthetic()
    group_of, names, slope, elem, ok, why = diagnostics.marginal_selection(site, table, spec, "t")
    assert ok and why is None and names == ["t[0]", "t[1]", "t[2]"] and list(elem) == [2, 3, 4]
    assert list(group_of) == [0, 1, 2, 0, -1, 1] and list(slope) == [1.0, 2.0, 0.75, 1.0, 0.0, -1.5]     # (0.25 + 0.5: read twice)
    # not a leaf: a later site reads the part, in its loc or in its log-scale
    for column, weights in (("loc_idx", "loc_w"), ("scale_idx", "scale_w")):
        child = site._replace(**{column: getattr(site, column).copy(), weights: getattr(site, weights).copy()})
        getattr(child, column)[5, 1], getattr(child, weights)[5, 1] = 3, 0.5
        *_, ok, why = diagnostics.marginal_selection(child, table, spec, "t")
        assert not ok and "not a leaf" in why and "element 5" in why
        getattr(child, weights)[5, 1] = 0.0                                      # (a term of weight 0 reads nothing)
        assert diagnostics.marginal_selection(child, table, spec, "t")[4]
    gamma = site._replace(form=np.array([0, 0, 0, 0, 0, models.SITE_LOG_GAMMA], np.int32), loc_idx=site.loc_idx.copy(), loc_w=site.loc_w.copy())
    gamma.loc_idx[5, 0], gamma.loc_w[5, 0] = 3, 1.0                              # (the log-Gamma form does not read its loc terms)
    assert diagnostics.marginal_selection(gamma, table, spec, "t")[4]
    # a softplus site
    soft = site._replace(form=np.array([0, 0, 0, models.SITE_NORMAL_SOFTPLUS, 0, 0], np.int32))
    *_, ok, why = diagnostics.marginal_selection(soft, table, spec, "t")
    assert not ok and "not a Normal with scale exp" in why and "form 1" in why
    # a scale that reads the part
    scaled = table._replace(scale_idx=np.array([-1, -1, 3, -1, -1, -1], np.int32))
    *_, ok, why = diagnostics.marginal_selection(site, scaled, spec, "t")
    assert not ok and "the scale of observation 2 reads t" in why
    # Bernoulli data
    *_, ok, why = diagnostics.marginal_selection(site, table._replace(kind=1), spec, "t")
    assert not ok and "Bernoulli" in why
    # the conditional report needs none of these: the groups are there in every case
    assert list(diagnostics.marginal_selection(soft, scaled._replace(kind=1), spec, "t")[0]) == [0, 1, 2, 0, -1, 1]
    # group_selection's refusals come through, under this flag's name
    with pytest.raises(ValueError, match="^--loo_groups: mu has one element"):
        diagnostics.marginal_selection(site, table, spec, "mu")
    with pytest.raises(ValueError, match="^--loo_groups: zz is no latent part of toy"):
        diagnostics.marginal_selection(site, table, spec, "zz")


def test_flag_refusals_before_any_device_and_the_key_order(capsys, monkeypatch):
    import torch
    from autoreparam_amd import main, models
    from autoreparam_amd.flags import FlagValues

    def touched(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    monkeypatch.setattr(torch.cuda, "device_count", touched)
    f = FlagValues()
    assert f.loo_groups == "" and main.loo_groups_part(f) == ""
    main.check_loo_groups(f)
    f.parse(["--model=radon", "--loo_groups=m"])
    with pytest.raises(ValueError, match="--loo_groups is read with --predictive_diagnostics only"):
        main.main([], flags=f)
    f.parse(["--predictive_diagnostics"])
    main.check_loo_groups(f)
    for model, part, word in (("radon", "b1", "one element"), ("radon", "county", "no latent part of radon"),
                              ("german_credit_lognormalcentered", "beta", "more than one element"),
                              ("electric", "sigma_y", "no observation"), ("time_series", "alpha3", "one element")):
        f.parse(["--model=" + model, "--loo_groups=" + part])
        with pytest.raises(ValueError, match="^--loo_groups: .*" + word):
            main.main([], flags=f)
    f.parse(["--model=neals_funnel", "--loo_groups=x2"])                      # (main.main stops at --predictive_diagnostics itself)
    with pytest.raises(ValueError, match="--loo_groups: neals_funnel has no observations"):
        main.check_loo_groups(f)
    with pytest.raises(ValueError, match="neals_funnel has no observations"):
        main.main([], flags=f)

    # the order of the keys
    assert main.LOGO_KEYS == (
        "logo_part", "logo_groups", "logo_groups_empty", "logo_observations_left_out", "logo_draws", "elpd_logo", "elpd_logo_se",
        "p_logo", "logo_pareto_k_max", "logo_pareto_k_max_group", "logo_pareto_k_above_threshold", "logo_conditional_elpd",
        "logo_conditional_elpd_se", "logo_conditional_p", "logo_conditional_pareto_k_max", "logo_conditional_pareto_k_max_group",
        "logo_conditional_pareto_k_above_threshold", "logo_pareto_k_threshold", "logo_nonfinite_groups", "logo_marginal", "logo_time_sec")
    assert not set(main.LOGO_KEYS) & set(main.LOO_KEYS + main.LOO_PRED_KEYS)

    # the null path: no device trace -- every key null, no message of its own
    class Results(object):
        trace = None
    cfg = type("Cfg", (), {"model": models._spec_eight_schools()})()
    for extra, want in (([], main.LOO_KEYS), (["--loo_groups=theta"], main.LOO_KEYS + main.LOGO_KEYS),
                        (["--loo_predictive", "--loo_groups=theta"], main.LOO_KEYS + main.LOO_PRED_KEYS + main.LOGO_KEYS)):
        f = FlagValues()
        f.parse(["--predictive_diagnostics"] + extra)
        capsys.readouterr()
        keys, arrays = main._convergence_report(Results(), cfg, f, None)
        assert arrays is None and tuple(keys) == want and all(v is None for v in keys.values())
        text = capsys.readouterr().out
        assert text.count("not computed") == 1 and "PSIS-LOO / WAIC: not computed" in text
    # a sharded job: the same, before the trace is looked at
    monkeypatch.setattr(main.parallel, "world", lambda: (0, 2))
    f = FlagValues()
    f.parse(["--predictive_diagnostics", "--loo_groups=theta"])
    keys, arrays = main._loo_report(None, None, 4, cfg.model, f)
    assert arrays is None and tuple(keys) == main.LOO_KEYS + main.LOGO_KEYS and all(v is None for v in keys.values())
    assert capsys.readouterr().out.count("not computed") == 1


def random_columns(rs, sizes):
    c = np.stack([-3.0 + rs.randn(sizes.size), 0.4 * rs.rand(sizes.size), -2.5 + rs.randn(sizes.size), rs.rand(sizes.size),
                  np.full(sizes.size, 50.0), rs.randn(sizes.size), rs.rand(sizes.size), np.full(sizes.size, 1000.0)], axis=1)
    c[sizes == 0] = np.nan
    return c


def test_logo_summary_against_the_reference_and_the_keys():
    from autoreparam_amd import diagnostics, main
    rs = np.random.RandomState(3)
    sizes = np.array([4, 0, 1, 7, 2, 0, 3])
    c, m = random_columns(rs, sizes), random_columns(rs, sizes)
    filled = sizes > 0
    for columns in (c, m):
        s = diagnostics.logo_summary(columns)
        ref = pr.summary(columns[filled, 0], columns[filled, 2], columns[filled, 3])
        assert (s.groups, s.empty) == (7, 2)
        for key, value in ref.items():
            assert getattr(s.total, key) == pytest.approx(value, rel=1e-12), key
        assert s.total.elpd_loo_se == pytest.approx(np.sqrt(5 * np.var(columns[filled, 0], ddof=1)), rel=1e-12)    # over GROUPS
    names = ["m[%d]" % g for g in range(7)]
    m[3, 1], c[4, 1] = 0.93, np.inf
    keys = main.logo_keys(c, m, "m", names, 2, 8200, 8)
    assert tuple(keys) == main.LOGO_KEYS[:-1]
    threshold = pr.k_threshold(8192)
    assert keys["logo_draws"] == 8192 and keys["logo_pareto_k_threshold"] == pytest.approx(threshold) and keys["logo_marginal"] is True
    assert keys["elpd_logo"] == pytest.approx(m[filled, 0].sum()) and keys["p_logo"] == pytest.approx((m[filled, 2] - m[filled, 0]).sum())
    assert keys["logo_conditional_elpd"] == pytest.approx(c[filled, 0].sum())
    assert keys["logo_pareto_k_max"] == 0.93 and keys["logo_pareto_k_max_group"] == "m[3]" and keys["logo_pareto_k_above_threshold"] == 1
    assert keys["logo_conditional_pareto_k_max"] == float(np.max(c[filled & np.isfinite(c[:, 1]), 1]))
    assert keys["logo_conditional_pareto_k_above_threshold"] == 1            # (a k-hat that was not fitted is above any threshold)
    assert keys["logo_groups_empty"] == 2 and keys["logo_nonfinite_groups"] == 0 and keys["logo_observations_left_out"] == 2
    m[0, 0] = -np.inf
    bad = main.logo_keys(c, m, "m", names, 2, 8200, 8)
    assert bad["logo_nonfinite_groups"] == 1 and bad["elpd_logo"] is None and bad["logo_conditional_elpd"] is not None
    none = main.logo_keys(c, None, "a", names, 2, 8200, 8)
    assert all(none[key] is None for key in main.LOGO_MARGINAL_KEYS) and none["logo_marginal"] is False
    assert none["logo_conditional_elpd"] == keys["logo_conditional_elpd"] and none["logo_nonfinite_groups"] == 0
    json.dumps(none)


def logo_file(path, model, elpd, cond, sizes, group_of, y, part="m"):
    from autoreparam_amd import main
    G = sizes.size
    arrays = collections.OrderedDict([("part", np.asarray(part)), ("groups", np.asarray(["%s[%d]" % (part, g) for g in range(G)])),
                                      ("group_of", group_of), ("n_obs", sizes)])
    for pre, e in (("", elpd), ("conditional_", cond)):
        arrays.update([(pre + "elpd_logo_g", e), (pre + "pareto_k", 0.1 * np.ones(G)), (pre + "lppd_g", e + 0.5), (pre + "p_waic_g", np.ones(G))])
    arrays.update([("y", y), ("model", np.asarray(model))])
    main.save_logo(path, arrays)


def test_the_side_file_is_written_from_save_loo(tmp_path):
    from autoreparam_amd import main
    plain = collections.OrderedDict([("elpd_loo_i", np.arange(3.0)), ("model", np.asarray("radon"))])
    flagged = collections.OrderedDict(plain)
    flagged[main.LOGO_ARRAYS] = collections.OrderedDict([("part", np.asarray("m")), ("groups", np.asarray(["m[0]", "m[1]"])),
                                                         ("elpd_logo_g", np.ones(2))])
    main.save_loo(str(tmp_path / "a"), plain)
    main.save_loo(str(tmp_path / "b"), flagged)
    assert sorted(os.listdir(str(tmp_path))) == ["a_loo.npz", "b_logo.npz", "b_loo.npz"]
    a, b = np.load(str(tmp_path / "a_loo.npz")), np.load(str(tmp_path / "b_loo.npz"))
    assert sorted(a.files) == sorted(b.files) == ["elpd_loo_i", "model"] and all(a[k].tobytes() == b[k].tobytes() for k in a.files)
    z = np.load(str(tmp_path / "b_logo.npz"))
    assert sorted(z.files) == ["elpd_logo_g", "groups", "part"] and str(z["part"]) == "m" and list(z["groups"]) == ["m[0]", "m[1]"]
    assert main.LOGO_ARRAYS in flagged                                   # (the caller's dict is left as it was)
    assert main.LOGO_ARRAYS not in [row.tag for row in main.SIDE_REPORTS]


def test_analyze_prints_the_line_and_compares_two_models(tmp_path, capsys):
    from autoreparam_amd import analyze, main
    d = tmp_path / "radon_MA"
    d.mkdir()
    run = {key: 0.5 for key in main.LOO_KEYS + main.LOGO_KEYS}
    run.update(loo_observations=1659, loo_draws=8192, loo_chains=256, logo_part="m", logo_groups=13, logo_groups_empty=0,
               logo_observations_left_out=0, logo_draws=8192, elpd_logo=-2711.5, elpd_logo_se=41.25, logo_pareto_k_max=0.31,
               logo_pareto_k_max_group="m[4]", logo_pareto_k_above_threshold=0, logo_conditional_elpd=-2650.0,
               logo_conditional_elpd_se=44.5, logo_conditional_pareto_k_max=1.75, logo_conditional_pareto_k_max_group="m[9]",
               logo_conditional_pareto_k_above_threshold=11, logo_pareto_k_threshold=0.7, logo_nonfinite_groups=0, logo_marginal=True)
    (d / "CP_tied.json").write_text(json.dumps({k: [None, v] for k, v in run.items()}))
    bern = dict(run)
    bern.update({key: None for key in main.LOGO_MARGINAL_KEYS})
    bern.update(logo_marginal=False, logo_part="a")
    (d / "NCP_tied.json").write_text(json.dumps({k: [v] for k, v in bern.items()}))
    (d / "cVIP_eig_tied.json").write_text(json.dumps({k: [v] for k, v in run.items() if k in main.LOO_KEYS}))
    analyze.main(["--results_dir", str(tmp_path), "--model", "radon_MA", "--loo"])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("      leave-one-group-out by ")]
    assert len(lines) == 2
    lines.sort(key=lambda l: "n/a" in l)
    assert lines[0].startswith("      leave-one-group-out by m: 13 groups (0 empty, 0 observations in none); marginal elpd_logo -2712 +/- 41.25, "
                               "worst Pareto k-hat 0.31 (m[4]; 0 above 0.7); conditional elpd -2650 +/- 44.5, worst Pareto k-hat 1.75 (m[9]; 11 above 0.7);")
    assert "by a:" in lines[1] and "marginal elpd_logo n/a (no closed marginal form); conditional elpd -2650 +/- 44.5" in lines[1]
    # --logo_compare: the paired difference over the non-empty groups
    rs = np.random.RandomState(8)
    sizes = np.array([3, 0, 2, 4, 1])
    group_of = np.array([0, 0, 0, 2, 2, 3, 3, 3, 3, 4, -1], np.int32)
    y = rs.randn(11).astype(np.float32)
    ea, eb = -3.0 + rs.randn(5), -3.5 + rs.randn(5)
    ea[1] = eb[1] = np.nan
    a, b = str(tmp_path / "A"), str(tmp_path / "B")
    logo_file(a, "radon", ea, ea - 1.0, sizes, group_of, y)
    logo_file(b, "radon_stddvs", eb, eb - 2.0, sizes, group_of, y)
    analyze.main(["--logo_compare=%s_logo.npz,%s_logo.npz" % (a, b)])
    filled = sizes > 0
    diff, se = pr.compare(ea[filled], eb[filled])
    assert "elpd_logo(radon) - elpd_logo(radon_stddvs) = {:.4g} +/- {:.4g} over 4 groups of m (marginal)".format(diff, se) in capsys.readouterr().out
    # a file without a marginal form: the conditional columns are compared
    logo_file(b, "election", np.full(5, np.nan), eb - 2.0, sizes, group_of, y)
    analyze.main(["--logo_compare=%s_logo.npz,%s_logo.npz" % (a, b)])
    diff, se = pr.compare(ea[filled] - 1.0, eb[filled] - 2.0)
    assert "= {:.4g} +/- {:.4g} over 4 groups of m (conditional)".format(diff, se) in capsys.readouterr().out
    # refused: another y, other groups, another part
    other = group_of.copy()
    other[0] = 2
    for kwargs, word in ((dict(y=y + 1.0), "differ in y"), (dict(group_of=other), "differ in group_of"), (dict(part="t"), "differ in part")):
        args = dict(sizes=sizes, group_of=group_of, y=y)
        args.update(kwargs)
        logo_file(b, "radon_stddvs", eb, eb - 2.0, **args)
        with pytest.raises(ValueError, match="logo_compare: the two files " + word):
            analyze.main(["--logo_compare=%s_logo.npz,%s_logo.npz" % (a, b)])
    with pytest.raises(SystemExit):
        analyze.main(["--logo_compare=" + a + "_logo.npz"])


@pytest.mark.parametrize("i", cases.NORMAL_CASES, ids=[cases.IDS[i] for i in cases.NORMAL_CASES])
def test_the_reference_agrees_with_the_closed_form_in_float64(i):
    """Self-check of tests/logo_ref.py on the cases of tests/test_gpu_logo.py -- exp(sj) in {e^-6, 1, e^6} and t0 five prior
    standard deviations from loc among them: the kernel's expression, restated in float64, against multivariate_normal."""
    c = cases.case(i)
    D = c.x3.shape[2]
    x = c.x3.reshape(-1, D)
    x = x[np.isfinite(x).all(axis=1)]
    q = lg.quantities(c.table, c.site, x, c.slope, c.elem)
    ref = lg.marginal(c.table, q, c.group_of, c.G, c.slope)
    closed = lg.closed_form(q, c.group_of, c.G)
    assert np.all(np.isfinite(ref)) and np.all(np.abs(closed - ref) <= 1e-9 * np.maximum(1.0, np.abs(ref)))
    log_sj, far = cases.CASES[i][10], cases.CASES[i][11]
    assert np.all(np.abs(q.sj - log_sj) < 0.5)
    if far:
        assert np.all(np.abs((q.t0 - q.loc) * np.exp(-q.sj) - 5.0) < 1e-3)
    # lc: the groups' sums of the pointwise reference; an empty group is 0 in both
    lc = lg.conditional(q, c.group_of, c.G)
    sizes = np.bincount(c.group_of[c.group_of >= 0], minlength=c.G)
    assert np.all(lc[sizes == 0] == 0.0) and np.all(ref[sizes == 0] == 0.0)


def test_the_cases_cover_what_the_kernel_branches_on():
    shapes = [c[4] * c[5] for c in cases.CASES]
    assert {1, 64, 65, 130} <= set(shapes) and {c[1] for c in cases.CASES} == {1, 88, 255} and {c[2] for c in cases.CASES} == {1, 3}
    assert {c[6] for c in cases.CASES} == {1, 4, 5, 9} and {cases.CASES[i][10] for i in cases.NORMAL_CASES} == {-6.0, 0.0, 6.0}
    assert max(c[3] for c in cases.CASES) <= 64 and any(c[8] for c in cases.CASES) and any(c[11] for c in cases.CASES)
    one = cases.case(0)
    assert one.x3.shape == (1, 1, 1) and one.G == 1 and not one.site.loc_w.any() and not one.site.scale_w.any()
    holes = cases.case(1)
    sizes = np.bincount(holes.group_of[holes.group_of >= 0], minlength=9)
    assert list(np.flatnonzero(sizes == 0)) == [0, 4, 8] and sizes[1] == 1 and np.sum(holes.group_of < 0) == 8
    assert len(set(np.round(holes.slope[holes.group_of >= 0], 4))) > 10 and np.all(cases.case(3).slope == 1.0)
    # the part is a leaf of the table: marginal_selection's conditions hold for every Normal case
    from autoreparam_amd import diagnostics
    for i in cases.NORMAL_CASES:
        c = cases.case(i)
        D, lo, hi = c.x3.shape[2], int(c.elem[0]), int(c.elem[-1]) + 1
        spec = Spec("toy", ["head", "t", "rest"][(lo == 0):], [(lo,), (hi - lo,), (D - hi,)][(lo == 0):], [0, lo, hi, D][(lo == 0):])
        if hi - lo < 2:
            continue                                                     # (group_selection refuses a part of one element)
        group_of, _, slope, elem, ok, why = diagnostics.marginal_selection(c.site, c.table, spec, "t")
        assert ok and np.array_equal(group_of, c.group_of) and np.array_equal(slope, c.slope) and np.array_equal(elem, c.elem), why
