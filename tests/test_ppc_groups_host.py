"""CPU: the host side of --predictive_checks_groups.  diagnostics.group_selection on the frozen data -- the groups, the empty
ones and the observations in none, counted from the data files when the report was written -- and its refusals, each
naming the flag; diagnostics.group_order; diagnostics.ppc_group_counts against diagnostics.ppc_counts group by group
(a group of one, an empty group, a mask) and its additivity over draws; the per-group summary and keys; the refusals of
the flag before anything touches a device; the order of the keys; the side file; analyze --ppc."""
import json
import os

import numpy as np
import pytest

# (model, dataset, part): groups, empty groups, observations in none, smallest and largest non-empty group
FROZEN = ((("radon", "MN", "m"), (85, 0, 0, 1, 116)),
          (("radon", "MA", "m"), (13, 0, 0, 6, 391)),
          (("election", None, "a"), (51, 3, 15, 12, 1280)),
          (("electric", None, "a"), (96, 1, 2, 2, 2)),
          (("electric", None, "b"), (4, 1, 117, 20, 34)),
          (("8schools", None, "theta"), (8, 0, 0, 1, 1)))


@pytest.mark.parametrize("which, want", FROZEN, ids=["-".join(str(v) for v in w) for w, _ in FROZEN])
def test_group_selection_on_the_frozen_data(which, want):
    from autoreparam_amd import diagnostics, models
    model, dataset, part = which
    spec = models.spec_by_name(model, dataset)
    table = spec.observation_table()
    group_of, names = diagnostics.group_selection(table, spec, part)
    N = table.y.size
    assert group_of.dtype == np.int32 and group_of.shape == (N,) and group_of.min() >= -1 and group_of.max() < len(names)
    sizes = np.bincount(group_of[group_of >= 0], minlength=len(names))
    assert (len(names), int(np.sum(sizes == 0)), int(np.sum(group_of < 0)), int(sizes[sizes > 0].min()), int(sizes.max())) == want
    # the rule itself: observation n reads element lo + group_of[n] of the part with a non-zero weight, and no other
    k = spec.part_names.index(part)
    lo, hi = int(spec.offsets[k]), int(spec.offsets[k + 1])
    assert len(names) == hi - lo and names[0].startswith(part + "[0") and len(set(names)) == len(names)
    for n in range(N):
        read = {int(i) - lo for i, w in zip(table.idx[n], table.w[n]) if w != 0 and lo <= i < hi}
        assert read == ({int(group_of[n])} if group_of[n] >= 0 else set()), n
    # order and group_start: sorted by group, ascending observation index within one
    order, start = diagnostics.group_order(group_of, len(names))
    assert order.dtype == start.dtype == np.int32 and start[0] == 0 and start[-1] == order.size == int(np.sum(group_of >= 0))
    assert np.array_equal(np.diff(start), sizes)
    for g in range(len(names)):
        assert np.array_equal(order[start[g]:start[g + 1]], np.flatnonzero(group_of == g))


def test_the_radon_groups_are_the_counties():
    from autoreparam_amd import diagnostics, models
    spec = models.spec_by_name("radon", "MN")
    group_of, names = diagnostics.group_selection(spec.observation_table(), spec, "m")
    assert np.array_equal(group_of, np.asarray(spec.raw["county"]).reshape(-1)) and names[17] == "m[17]"
    spec = models.spec_by_name("election")
    group_of, _ = diagnostics.group_selection(spec.observation_table(), spec, "a")
    state = np.asarray(spec.raw["state"]).reshape(-1)
    inside = (state >= 0) & (state < int(spec.raw["n_state"]))
    assert np.array_equal(group_of[inside], state[inside]) and np.all(group_of[~inside] == -1)
    assert np.any(np.diff(group_of[inside]) < 0)                         # the states are interleaved: a group is not a range


def test_group_selection_refusals_name_the_flag():
    from autoreparam_amd import diagnostics, models
    refused = [("radon", "zz", "zz is no latent part of radon; its parts: mua, b1, b2, m"),
               ("radon", "mua", "mua has one element"), ("radon", "b2", "b2 has one element"),
               ("german_credit_lognormalcentered", "beta", "1000 observation.s. read more than one element of beta"),
               ("german_credit_lognormalcentered", "beta_log_scales", "no observation's linear predictor reads beta_log_scales"),
               ("german_credit_gammascale", "beta", "more than one element of beta"),
               ("german_credit_gammascale", "overall_log_scale", "one element"),
               ("8schools", "mu", "one element"), ("election", "log_sigma_a", "one element"), ("electric", "mua", "no observation"),
               ("electric", "sigma_y", "no observation")]
    for model, part, word in refused:
        spec = models.spec_by_name(model)
        with pytest.raises(ValueError, match="^--predictive_checks_groups: .*" + word):
            diagnostics.group_selection(spec.observation_table(), spec, part)
    for model in ("time_series", "german_credit_lognormalcentered", "german_credit_gammascale"):       # every part of these
        spec = models.spec_by_name(model)
        table = spec.observation_table()
        for part in spec.part_names:
            with pytest.raises(ValueError, match="^--predictive_checks_groups: "):
                diagnostics.group_selection(table, spec, part)


def random_stats(rs, G, R, sizes):
    """[G, R, 8] statistics of replicated data sets of the groups' sizes: consistent sums, minima and maxima"""
    out = np.zeros((G, R, 8))
    for g in range(G):
        n = int(sizes[g])
        if not n:
            out[g, :, 2], out[g, :, 3] = np.inf, -np.inf
            continue
        v = rs.randn(n, R) + 0.3 * g
        out[g] = np.stack([v.sum(0), (v * v).sum(0), v.min(0), v.max(0), rs.rand(R) * n, rs.rand(R) * n, v.sum(0), np.full(R, float(n))],
                          axis=1)
    return out


def test_group_counts_are_ppc_counts_group_by_group():
    from autoreparam_amd import diagnostics
    rs = np.random.RandomState(5)
    group_of = np.array([2, 0, 2, -1, 4, 2, 0, 4, 4, -1, 2, 5], np.int32)    # group 1 and 3 empty, group 5 of one, two in none
    G, R = 6, 40
    sizes = np.bincount(group_of[group_of >= 0], minlength=G)
    y = rs.randn(group_of.size)
    stats = random_stats(rs, G, R, sizes)
    mask = np.zeros(R, np.uint8)
    mask[[3, 17, 39]] = 1
    clean = stats.copy()
    stats[:, mask != 0] = 0.0                                            # (a draw left out: zero rows, as the kernel writes them)
    for m in (None, mask):
        if m is None:
            stats, masked = clean, stats
        else:
            stats = masked
        counts = diagnostics.ppc_group_counts(stats, y, group_of, m)
        assert counts.shape == (G, diagnostics.PPC_COUNTS)
        for g in range(G):
            members = y[group_of == g]
            want = diagnostics.ppc_counts(stats[g], members, m) if members.size else np.zeros(diagnostics.PPC_COUNTS)
            assert np.array_equal(counts[g], want, equal_nan=True), g          # (a group of one: the sum of its sd is NaN)
        assert np.all(counts[[1, 3]] == 0.0) and counts[5, 0] == (R if m is None else R - 3)
        assert counts[5, 3] == 0.0                                       # a group of one: sd is NaN on both sides, never >=
    # a range of groups under its first index, and torch tensors
    import torch
    part = diagnostics.ppc_group_counts(torch.as_tensor(stats[2:5]), y, group_of, torch.as_tensor(mask), g0=2)
    assert np.array_equal(part, diagnostics.ppc_group_counts(stats, y, group_of, mask)[2:5], equal_nan=True)
    # additive over draws
    whole = diagnostics.ppc_group_counts(stats, y, group_of, mask)
    halves = diagnostics.ppc_group_counts(stats[:, :23], y, group_of, mask[:23]) + diagnostics.ppc_group_counts(stats[:, 23:], y, group_of, mask[23:])
    assert np.array_equal(halves[:, :7], whole[:, :7]) and np.allclose(halves, whole, rtol=1e-13, atol=0, equal_nan=True)
    # the statistics must cover the group, as ppc_counts demands of the whole data
    wrong = clean.copy()
    wrong[2, :, 7] += 1
    with pytest.raises(ValueError, match="must cover all 4 observations"):
        diagnostics.ppc_group_counts(wrong, y, group_of)
    with pytest.raises(ValueError, match="one entry per observation"):
        diagnostics.ppc_group_counts(stats, y[:-1], group_of)
    with pytest.raises(ValueError, match=r"\[G, R, 8\]"):
        diagnostics.ppc_group_counts(stats[0], y, group_of)


def test_group_summary_and_keys():
    from autoreparam_amd import diagnostics, main
    rs = np.random.RandomState(6)
    group_of = np.array([2, 0, 2, -1, 3, 2, 0, 3, 3, -1, 2, 1], np.int32)    # group 4 empty, group 1 of one
    G, R = 5, 4000
    names = ["m[%d]" % g for g in range(G)]
    sizes = np.bincount(group_of[group_of >= 0], minlength=G)
    y = rs.randn(group_of.size)
    y[group_of == 3] += 40.0                                             # a group the replicated data never reach
    stats = random_stats(rs, G, R, sizes)
    counts = diagnostics.ppc_group_counts(stats, y, group_of)
    s = diagnostics.ppc_group_summary(counts, y, group_of, 0)
    assert s.draws_used == R and s.draws_left_out == 0 and list(s.sizes) == list(sizes)
    for g in range(G):
        members = y[group_of == g]
        one = diagnostics.ppc_from_counts(counts[g], np.zeros((members.size, 4)), members, 0)
        for name in diagnostics.PPC_STATISTICS:
            for got, want in ((s.p, one.p), (s.rep, one.rep), (s.obs, one.obs)):
                assert (np.isnan(got[name][g]) and want[name] is None) or got[name][g] == want[name], (g, name)
    assert np.isnan(s.p["sd"][1]) and np.isfinite(s.p["mean"][1]) and all(np.isnan(s.p[n][4]) for n in diagnostics.PPC_STATISTICS)
    keys = main.ppc_group_keys(s, "m", names, 2)
    assert tuple(keys) == main.PPC_GROUP_KEYS[:-1]
    assert keys["ppc_group_part"] == "m" and keys["ppc_groups"] == 5 and keys["ppc_groups_empty"] == 1
    assert keys["ppc_group_observations_left_out"] == 2 and keys["ppc_group_draws"] == R
    assert keys["ppc_group_p_threshold"] == 0.005 / 4 and keys["ppc_group_p_mean_min"] == 0.0 and keys["ppc_group_p_mean_min_group"] == "m[3]"
    assert keys["ppc_group_p_mean_max"] == float(np.nanmax(s.p["mean"])) and keys["ppc_group_p_sd_min_group"] in ("m[0]", "m[2]", "m[3]")
    assert keys["ppc_group_extreme_groups"] == [names[g] for g in range(4) if s.p["mean"][g] <= 0.00125 or s.p["mean"][g] >= 0.99875]
    assert "m[3]" in keys["ppc_group_extreme_groups"]
    json.dumps(keys)
    mixed = main.ppc_group_keys(s, "m", names, 2, mixed=True)
    assert tuple(mixed) == main.PPC_GROUP_MIXED_KEYS[:-1] and list(mixed.values()) == list(keys.values())
    # too few draws to resolve the threshold: 1 / (0.005 / 4) = 800
    few = diagnostics.ppc_group_summary(diagnostics.ppc_group_counts(stats[:, :799], y, group_of), y, group_of, 0)
    assert main.ppc_group_keys(few, "m", names, 2)["ppc_group_extreme_groups"] is None
    enough = diagnostics.ppc_group_summary(diagnostics.ppc_group_counts(stats[:, :800], y, group_of), y, group_of, 0)
    assert main.ppc_group_keys(enough, "m", names, 2)["ppc_group_extreme_groups"] is not None
    # Bernoulli data: no sd anywhere; no draw used: no figure at all
    yb = (y > 0).astype(float)
    sb = diagnostics.ppc_group_summary(counts, yb, group_of, 1)
    kb = main.ppc_group_keys(sb, "a", names, 2)
    assert kb["ppc_group_p_sd_min"] is None and kb["ppc_group_p_sd_max_group"] is None and kb["ppc_group_p_mean_min"] is not None
    none = diagnostics.ppc_group_summary(diagnostics.ppc_group_counts(stats, y, group_of, np.ones(R)), y, group_of, 0)
    kn = main.ppc_group_keys(none, "m", names, 2)
    assert kn["ppc_group_draws"] == 0 and kn["ppc_group_p_mean_min"] is None and kn["ppc_group_extreme_groups"] is None
    assert kn["ppc_groups"] == 5 and kn["ppc_group_p_threshold"] == 0.005 / 4


def test_flag_refusals_before_any_device_and_the_key_order(capsys, monkeypatch):
    import torch
    from autoreparam_amd import main, models
    from autoreparam_amd.flags import FlagValues

    def touched(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    monkeypatch.setattr(torch.cuda, "device_count", touched)
    f = FlagValues()
    assert f.predictive_checks_groups == "" and main.groups_part(f) == ""
    main.check_predictive_groups(f)
    f.parse(["--model=radon", "--predictive_checks_groups=m"])
    with pytest.raises(ValueError, match="--predictive_checks_groups is read with --predictive_checks only"):
        main.main([], flags=f)
    f.parse(["--predictive_checks"])
    main.check_predictive_groups(f)
    for model, part, word in (("radon", "b1", "one element"), ("radon", "county", "no latent part of radon"),
                              ("german_credit_lognormalcentered", "beta", "more than one element"),
                              ("time_series", "alpha3", "one element")):
        f.parse(["--model=" + model, "--predictive_checks_groups=" + part])
        with pytest.raises(ValueError, match="--predictive_checks_groups.*" + word):
            main.main([], flags=f)
    f.parse(["--model=neals_funnel", "--predictive_checks_groups=x2"])      # (main.main stops at --predictive_checks itself)
    with pytest.raises(ValueError, match="--predictive_checks_groups: neals_funnel has no observations"):
        main.check_predictive_groups(f)
    with pytest.raises(ValueError, match="neals_funnel has no observations"):
        main.main([], flags=f)

    # the null path and the order of the keys
    class Results(object):
        trace = None
    cfg = type("Cfg", (), {"model": models._spec_eight_schools()})()
    orders = (([], main.PPC_KEYS), (["--predictive_checks_redraw=theta"], main.PPC_KEYS + main.PPC_MIXED_KEYS),
              (["--predictive_checks_groups=theta"], main.PPC_KEYS + main.PPC_GROUP_KEYS),
              (["--predictive_checks_redraw=theta", "--predictive_checks_groups=theta"],
               main.PPC_KEYS + main.PPC_MIXED_KEYS + main.PPC_GROUP_KEYS + main.PPC_GROUP_MIXED_KEYS))
    for extra, want in orders:
        f = FlagValues()
        f.parse(["--predictive_checks"] + extra)
        capsys.readouterr()
        keys, arrays = main._convergence_report(Results(), cfg, f, None)
        assert arrays is None and tuple(keys) == want and all(v is None for v in keys.values())
        assert capsys.readouterr().out.count("posterior predictive checks: not computed") == 1
    every = main.PPC_KEYS + main.PPC_MIXED_KEYS + main.PPC_GROUP_KEYS + main.PPC_GROUP_MIXED_KEYS
    assert len(set(every)) == len(every) and all(k.startswith("ppc_group") for k in main.PPC_GROUP_KEYS + main.PPC_GROUP_MIXED_KEYS)
    assert main.PPC_GROUP_KEYS[:5] == ("ppc_group_part", "ppc_groups", "ppc_groups_empty", "ppc_group_observations_left_out", "ppc_group_draws")
    for name in ("mean", "sd", "deviance"):
        for end in ("min", "max"):
            assert "ppc_group_p_%s_%s" % (name, end) in main.PPC_GROUP_KEYS and "ppc_group_p_%s_%s_group" % (name, end) in main.PPC_GROUP_KEYS
    assert main.PPC_GROUP_KEYS[-3:] == ("ppc_group_p_threshold", "ppc_group_extreme_groups", "ppc_group_time_sec")
    suffix = lambda k: k[len("ppc_group_"):] if k.startswith("ppc_group_") else k[len("ppc_"):]      # (ppc_groups, ppc_groups_empty)
    assert main.PPC_GROUP_MIXED_KEYS == tuple("ppc_group_mixed_" + suffix(k) for k in main.PPC_GROUP_KEYS)
    assert main.PPC_GROUP_ARRAYS not in [row.tag for row in main.SIDE_REPORTS] and len(main.SIDE_REPORTS) == 9


def test_the_side_file_is_written_from_save_ppc(tmp_path):
    from collections import OrderedDict
    from autoreparam_amd import main
    plain = OrderedDict([("pit", np.arange(3.0)), ("model", np.asarray("radon"))])
    flagged = OrderedDict(plain)
    flagged[main.PPC_GROUP_ARRAYS] = OrderedDict([("part", np.asarray("m")), ("groups", np.asarray(["m[0]", "m[1]"])), ("p_mean", np.ones(2))])
    both = OrderedDict(flagged)
    both[main.PPC_MIXED_ARRAYS] = OrderedDict([("parts", np.asarray(["m"]))])
    main.save_ppc(str(tmp_path / "a"), plain)
    main.save_ppc(str(tmp_path / "b"), flagged)
    main.save_ppc(str(tmp_path / "c"), both)
    assert sorted(os.listdir(str(tmp_path))) == ["a_ppc.npz", "b_ppc.npz", "b_ppc_groups.npz", "c_ppc.npz", "c_ppc_groups.npz",
                                                 "c_ppc_mixed.npz"]
    a, b = np.load(str(tmp_path / "a_ppc.npz")), np.load(str(tmp_path / "b_ppc.npz"))
    assert sorted(a.files) == sorted(b.files) == ["model", "pit"] and all(a[k].tobytes() == b[k].tobytes() for k in a.files)
    z = np.load(str(tmp_path / "b_ppc_groups.npz"))
    assert sorted(z.files) == ["groups", "p_mean", "part"] and str(z["part"]) == "m" and list(z["groups"]) == ["m[0]", "m[1]"]
    assert main.PPC_GROUP_ARRAYS in flagged                              # (the caller's dict is left as it was)


def test_analyze_prints_the_group_line(tmp_path, capsys):
    from autoreparam_amd import analyze, main
    d = tmp_path / "radon_MA"
    d.mkdir()
    run = {key: 0.5 for key in main.PPC_KEYS + main.PPC_GROUP_KEYS}
    run.update(ppc_observations=1659, ppc_draws=8192, ppc_chains=256, ppc_draws_left_out=0, ppc_group_part="m", ppc_groups=13,
               ppc_groups_empty=0, ppc_group_observations_left_out=0, ppc_group_draws=8192, ppc_group_p_mean_min=0.31,
               ppc_group_p_mean_min_group="m[4]", ppc_group_p_mean_max=0.72, ppc_group_p_mean_max_group="m[9]",
               ppc_group_p_threshold=0.005 / 13, ppc_group_extreme_groups=[])
    (d / "CP_tied.json").write_text(json.dumps({k: [None, v] for k, v in run.items()}))
    both = dict(run)
    both.update({key: 0.5 for key in main.PPC_MIXED_KEYS + main.PPC_GROUP_MIXED_KEYS})
    both.update(ppc_mixed_parts=["m"], ppc_mixed_elements=13, ppc_mixed_draws=8192, ppc_mixed_draws_left_out=0,
                ppc_mixed_pit_extreme_observations=[], ppc_group_mixed_draws=8192, ppc_group_mixed_p_mean_min=0.0001,
                ppc_group_mixed_p_mean_min_group="m[2]", ppc_group_mixed_p_mean_max=0.9, ppc_group_mixed_p_mean_max_group="m[7]",
                ppc_group_mixed_extreme_groups=["m[2]"])
    (d / "NCP_tied.json").write_text(json.dumps({k: [v] for k, v in both.items()}))
    (d / "cVIP_eig_tied.json").write_text(json.dumps({k: [v] for k, v in run.items() if k in main.PPC_KEYS}))
    analyze.main(["--results_dir", str(tmp_path), "--model", "radon_MA", "--ppc"])
    lines = capsys.readouterr().out.splitlines()
    grouped = [l for l in lines if l.startswith("      grouped predictive by m: 13 groups (0 empty, 0 observations in none)")]
    assert len(grouped) == 2
    grouped.sort(key=lambda l: "mixed" in l)
    assert "smallest ... largest 0.31 (m[4]) ... 0.72 (m[9]);" in grouped[0] and "beyond the threshold 0.0003846: none;" in grouped[0]
    assert "mixed" not in grouped[0]
    assert ", mixed 0.0001 (m[2]) ... 0.9 (m[7]);" in grouped[1] and ": none, mixed m[2];" in grouped[1]
