"""CPU: the host half of the per-site log prior -- ModelSpec.site_table against the float64 model programs (the identity
site densities + pointwise log-likelihoods = log joint, which ties tests/site_ref.py, tests/loglik_ref.py and
oracle/ed2_ref.py, written independently of each other), the table's structure for all nine models, electric's one-hot
quirk, diagnostics.upload_site_table's refusals, --sensitivity_prior_parts and its refusals before the run."""
import numpy as np
import pytest

import loglik_ref as lr
import site_ref as sr

SPECS = {
    "8schools": lambda m: m._spec_eight_schools(), "radon_MN": lambda m: m._spec_radon("MN"),
    "radon_PA": lambda m: m._spec_radon("PA"), "radon_stddvs": lambda m: m._spec_radon_stddvs("MN"),
    "neals_funnel": lambda m: m._spec_funnel(), "german_credit_lognormalcentered": lambda m: m._spec_german(),
    "german_credit_gammascale": lambda m: m._spec_german_gammascale(), "election": lambda m: m._spec_election(),
    "electric": lambda m: m._spec_electric(), "time_series": lambda m: m._spec_time_series()}
STATES = 8


def states(spec):
    return 0.7 * np.random.RandomState(20).randn(STATES, spec.D)


def absolute_terms(table, spec, x):
    """sum |terms| of the two sides of the identity: every site density and every pointwise log-likelihood"""
    size = np.abs(sr.elements(table, x)).sum(axis=1)
    if spec.name != "neals_funnel":
        size = size + np.abs(lr.loglik(spec, x)).sum(axis=1)
    return size


@pytest.mark.parametrize("name", sorted(SPECS))
def test_sites_and_likelihoods_add_up_to_the_log_joint(name):
    """sum_d site density + sum_n pointwise log-likelihood = the centred log joint of the model program, at 8 states
    0.7 N(0, 1): within (D + N + 16) 2^-53 sum |terms| -- sequential float64 addition of D + N terms and a few roundings
    per term of two formulas for the same number."""
    from autoreparam_amd import models
    from oracle import ed2_ref
    spec = SPECS[name](models)
    table = spec.site_table()
    x = states(spec)
    N = 0 if name == "neals_funnel" else np.asarray(spec.raw["y"]).size
    mine = sr.total(table, x)
    if N:
        mine = mine + lr.loglik(spec, x).sum(axis=1)
    if name == "german_credit_gammascale":
        from gammascale_ref import GermanRef
        ref = GermanRef(spec.raw["X"], spec.raw["y"], prior="gamma")
        one = np.ones(spec.D, np.float32)
        want = ref.logp_grad(x, one, one)[0] + ref.logp_const(one)
    else:
        want = np.asarray([ed2_ref.log_joint(spec, "CP", x[i])[0] for i in range(STATES)])
    allow = (spec.D + N + 16) * 2.0 ** -53 * absolute_terms(table, spec, x)
    gap = np.abs(mine - want)
    print("%s: largest gap / sum |terms| %.3g" % (name, float((gap / absolute_terms(table, spec, x)).max())))
    assert np.all(np.isfinite(want)) and np.all(gap <= allow), (name, gap, allow)


@pytest.mark.parametrize("name", sorted(SPECS))
def test_structure(name):
    from autoreparam_amd import models
    spec = SPECS[name](models)
    t = spec.site_table()
    D = spec.D
    assert type(t).__name__ == "SiteTable" and t._fields == ("form", "loc_idx", "loc_w", "loc0", "scale_idx", "scale_w",
                                                             "log_scale0", "norm", "part")
    for col in (t.form, t.part):
        assert col.shape == (D,) and col.dtype == np.int32
    for col in (t.loc_idx, t.scale_idx):
        assert col.shape == (D, 2) and col.dtype == np.int32 and col.min() >= 0 and col.max() < D
    for col in (t.loc_w, t.scale_w):
        assert col.shape == (D, 2) and col.dtype == np.float64
    for col in (t.loc0, t.log_scale0, t.norm):
        assert col.shape == (D,) and col.dtype == np.float64 and np.all(np.isfinite(col))
    assert set(np.unique(t.form)) <= {0, 1, 2}
    # part agrees with offsets
    for k in range(len(spec.part_names)):
        assert np.all(t.part[spec.offsets[k]:spec.offsets[k + 1]] == k)
    # the ancestral order, and the padding
    d = np.arange(D)[:, None]
    for idx, w in ((t.loc_idx, t.loc_w), (t.scale_idx, t.scale_w)):
        assert np.all(idx[w != 0] < np.broadcast_to(d, idx.shape)[w != 0])
        assert np.all(idx[w == 0] == 0)
    # a Normal's normaliser
    assert np.all(t.norm[t.form != 2] == -0.5 * np.log(2.0 * np.pi))


def test_the_forms_each_model_uses():
    from autoreparam_amd import models
    forms = {name: set(np.unique(SPECS[name](models).site_table().form)) for name in SPECS}
    assert forms.pop("time_series") == {0, 1} and forms.pop("german_credit_gammascale") == {0, 2}
    assert all(f == {0} for f in forms.values())
    g = models._spec_german_gammascale()
    t = g.site_table()
    bls = slice(g.offsets[1], g.offsets[2])
    assert np.all(t.loc0[bls] == 0.5) and np.all(t.log_scale0[bls] == np.log(0.5))
    assert np.allclose(t.norm[bls], -0.5 * np.log(2.0 * np.pi), rtol=1e-15)          # Gamma(1/2, 1/2): the same number
    beta = slice(g.offsets[2], g.offsets[3])
    assert np.all(t.scale_w[beta] == 1.0) and np.all(t.scale_idx[beta, 0] == 0)
    assert np.array_equal(t.scale_idx[beta, 1], np.arange(g.offsets[1], g.offsets[2]))
    f = models._spec_funnel().site_table()
    assert f.scale_w[1, 0] == 0.5 and f.log_scale0[0] == np.log(3.0)


def test_electric_one_hot_quirk_is_a_term_of_weight_zero():
    """The reference feeds the 1-based grade_pair to tf.one_hot: an index outside [0, depth) is an all-zero row, so the
    pair's loc is 0.  The real data have such pairs; a planted one (negative) behaves the same."""
    from autoreparam_amd import models
    ec = models._spec_electric()
    t = ec.site_table()
    a = np.arange(ec.offsets[2], ec.offsets[3])
    gp = np.asarray(ec.raw["grade_pair"]).reshape(-1)
    out = gp >= int(ec.raw["n_grade_pair"])
    assert out.any() and np.all(t.loc_w[a[out], 0] == 0) and np.all(t.loc_idx[a[out], 0] == 0)
    assert np.all(t.loc_w[a[~out], 0] == 100.0) and np.array_equal(t.loc_idx[a[~out], 0], ec.offsets[0] + gp[~out])
    planted = np.array(gp).copy()
    keep = int(np.flatnonzero(~out)[0])
    planted[keep] = -1
    ec.raw = dict(ec.raw, grade_pair=planted)
    t2 = ec.site_table()
    assert t2.loc_w[a[keep], 0] == 0 and t2.loc_idx[a[keep], 0] == 0
    assert np.array_equal(np.delete(t2.loc_w[a, 0], keep), np.delete(t.loc_w[a, 0], keep))


def test_upload_rounds_to_float32_and_refuses_each_broken_column():
    from autoreparam_amd import diagnostics, models
    spec = models._spec_time_series()
    t = spec.site_table()
    D = spec.D
    up = diagnostics.upload_site_table(t, D, "cpu")
    assert up.D == D and up.P == len(spec.part_names)
    for name in ("loc_w", "scale_w", "loc0", "log_scale0", "norm"):
        host, dev = getattr(up.host, name), getattr(up, name)
        assert host.dtype == np.float32 and np.array_equal(host, np.asarray(getattr(t, name), np.float32))
        assert dev.numpy().dtype == np.float32 and np.array_equal(dev.numpy(), host)
    for name in ("form", "loc_idx", "scale_idx", "part"):
        assert getattr(up.host, name).dtype == np.int32 and np.array_equal(getattr(up, name).numpy(), getattr(t, name))

    def broken(name, change):
        col = np.array(getattr(t, name)).copy()
        change(col)
        return t._replace(**{name: col})

    def at(i, v):
        def change(col):
            col[i] = v
        return change
    last = D - 1
    cases = [("loc_idx", at((3, 0), D), "outside the state"), ("loc_idx", at((3, 0), -1), "outside the state"),
             ("scale_idx", at((3, 1), D), "outside the state"), ("scale_idx", at((0, 0), -1), "outside the state"),
             ("form", at(5, 3), "form must be"), ("form", at(5, -1), "form must be"), ("part", at(0, -1), "part must not"),
             ("loc_idx", at((4, 0), last), "ancestral"),                 # alpha1's parent moved behind it
             ("scale_w", at((0, 0), 1.0), "ancestral")]                  # element 0 has nothing before it
    for name, change, message in cases:
        with pytest.raises(ValueError, match=message):
            diagnostics.upload_site_table(broken(name, change), D, "cpu")
    for name in ("form", "loc0", "log_scale0", "norm", "part"):
        with pytest.raises(ValueError, match="one entry per element"):
            diagnostics.upload_site_table(t._replace(**{name: getattr(t, name)[:-1]}), D, "cpu")
    for name in ("loc_idx", "loc_w", "scale_idx", "scale_w"):
        with pytest.raises(ValueError, match=r"of shape \[%d, 2\]" % D):
            diagnostics.upload_site_table(t._replace(**{name: getattr(t, name)[:, :1]}), D, "cpu")
    with pytest.raises(ValueError, match="one entry per element"):
        diagnostics.upload_site_table(t, D + 1, "cpu")


def test_flag_and_its_refusals_before_the_run(tmp_path):
    from autoreparam_amd import main
    from autoreparam_amd.flags import FlagValues
    f = FlagValues()
    assert f.sensitivity_prior_parts == "" and main.prior_parts(f) == []
    main.check_sensitivity_sites(f)
    f.parse(["--model=election", "--sensitivity_diagnostics", "--sensitivity_prior_parts=b1,log_sigma_a"])
    assert main.prior_parts(f) == ["b1", "log_sigma_a"]
    main.check_sensitivity_sites(f)
    results = str(tmp_path)
    for argv, message in (
            (["--nosensitivity_diagnostics"], "with --sensitivity_diagnostics only"),
            (["--sensitivity_diagnostics", "--sensitivity_prior_parts=b1,theta"],
             "theta is no latent part of election; its parts: mua, log_sigma_a, a, b1, b2"),
            (["--sensitivity_prior_parts=b1,b2,b1"], "b1 is named twice"),
            (["--sensitivity_prior_parts=b1,"], "an empty name"),
            (["--sensitivity_prior_parts=,b1"], "an empty name")):
        f.parse(argv)
        with pytest.raises(ValueError, match=message):
            main.check_sensitivity_sites(f)
        with pytest.raises(ValueError, match=message):
            main.main(["--results_dir=" + results], flags=f)                 # before the model is loaded or anything runs
    import os
    assert os.listdir(results) == []
    f.parse(["--sensitivity_prior_parts="])
    main.check_sensitivity_sites(f)


def test_null_keys_carry_the_site_keys_only_with_the_flag(capsys):
    from autoreparam_amd import main
    from autoreparam_amd.flags import FlagValues
    f = FlagValues()
    assert tuple(main._psens_null("a reason", f)) == main.PSENS_KEYS
    f.parse(["--sensitivity_diagnostics", "--sensitivity_prior_parts=mu"])
    null = main._psens_null("a reason", f)
    assert tuple(null) == main.PSENS_KEYS + main.PSENS_SITE_KEYS and all(v is None for v in null.values())
    assert capsys.readouterr().out.count("not computed") == 2
