"""GPU: --predictive_checks_groups end to end through main.main, on the helpers of tests/test_gpu_ppc.py (256 chains, 200
samples, --loo_draws=8192, one copied VI / tuning directory).  Radon MA, NCP, grouped by m (13 counties: 8 192 draws resolve
the threshold 0.005 / 13), three sampling runs: --predictive_checks alone, with the flag, and with --predictive_checks_redraw=m
too.  The flag adds exactly PPC_GROUP_KEYS and <method>_ppc_groups.npz and changes nothing else, bit for bit; the file's
arrays are diagnostics.ppc_group_summary of diagnostics.ppc_group_counts of diagnostics.group_predictive_check called
here on the same draws under the report's seed -- and, for the mixed block, on rows redrawn here under the mixed check's
seeds; the mixed block and PPC_GROUP_MIXED_KEYS exist only with the redraw.  Election grouped by a (Bernoulli data, 51 states
of which 3 are empty, 15 observations in no state): no sd, NaN rows for the empty groups, and no extreme groups named, since
8 192 draws do not resolve 0.005 / 48.  A refused part raises before the run."""
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

from test_gpu_ppc import HM, _cli

pytestmark = pytest.mark.gpu

STATS = ("mean", "sd", "min", "max", "deviance")
GROUP_ARRAYS = ["%s_%s" % (what, name) for what in ("p", "rep", "obs") for name in STATS]
RUN = ["--inference=HMC", "--predictive_checks", "--loo_draws=8192"] + HM


def common(model, extra, method):
    return ["--model=" + model, "--num_chains=256", "--seed=3", "--num_optimization_steps=400", "--method=" + method] + extra


def tuned(root, model, extra, method):
    """VI and one tuning run of `model` under `root`."""
    _cli(common(model, extra, method) + ["--results_dir=" + root, "--inference=VI"])
    _cli(common(model, extra, method) + ["--results_dir=" + root, "--inference=HMCtuning", "--num_leapfrog_steps=4"] + HM)


def same_files(a_dir, b_dir, method, suffixes):
    for suffix in suffixes:
        a, b = (np.load(os.path.join(d, method + "_tied" + suffix)) for d in (a_dir, b_dir))
        assert sorted(a.files) == sorted(b.files), suffix
        for name in a.files:
            assert a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), (suffix, name)


def direct(spec, part, out, seed, mixed_parts=None):
    """The per-group summary from the wrappers alone, on the recorded trace: the report's draws, seed and draw offset 0"""
    from autoreparam_amd import diagnostics, main as cli
    trace = out["kernel_results"].trace
    dev = trace.device
    picked = cli.loo_steps(int(trace.shape[0]), 256, 8192)
    draws = trace[torch.as_tensor(picked, device=dev), :256].contiguous()
    assert draws.shape[0] * draws.shape[1] == 8192
    host = spec.observation_table()
    table = diagnostics.upload_table(host, spec.D, dev)
    group_of, names = diagnostics.group_selection(host, spec, part)
    groups = diagnostics.upload_groups(*diagnostics.group_order(group_of, len(names)), host.y.size, dev)
    left = None
    if mixed_parts is None:
        stats, mask, _ = diagnostics.group_predictive_check(draws, table, groups, seed=cli.derived_seed(seed, cli.PPC_SEED))
        left = mask != 0
    else:
        s = cli.derived_seed(seed, cli.PPC_MIXED_SEED)
        redrawn = diagnostics.redraw_selection(spec.site_table(), spec.part_names, mixed_parts)
        site = diagnostics.upload_site_table(spec.site_table(), spec.D, dev)
        rows, undrawn = diagnostics.site_redraw(draws, site, redrawn, seed=s, draw_offset=0)
        stats, mask, _ = diagnostics.group_predictive_check(rows[None], table, groups, seed=cli.next_seed(s))
        left = (mask != 0) | (undrawn != 0)
    y = np.asarray(host.y, np.float32).reshape(-1)
    counts = diagnostics.ppc_group_counts(stats, y, group_of, left)
    return diagnostics.ppc_group_summary(counts, y, group_of, int(host.kind)), group_of, names


def check_block(z, prefix, summary):
    for what in ("p", "rep", "obs"):
        for name in STATS:
            got, want = z["%s%s_%s" % (prefix, what, name)], getattr(summary, what)[name]
            assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True), (prefix, what, name)


def check_keys(r, prefix, summary, names, cli, part, n_ungrouped):
    want = cli.ppc_group_keys(summary, part, names, n_ungrouped, mixed=prefix.endswith("mixed_"))
    for key, value in want.items():
        assert r[key] == [value], key
    return want


def test_radon_by_county(gpu, tmp_path, capsys):
    from autoreparam_amd import analyze, diagnostics, main as cli, models
    spec = models.spec_by_name("radon", "MA")
    method, extra = "NCP", ["--dataset=MA"]
    plain, flagged, both = (str(tmp_path / name) for name in ("plain", "flagged", "both"))
    tuned(plain, "radon", extra, method)
    shutil.copytree(plain, flagged)
    shutil.copytree(plain, both)
    args = common("radon", extra, method)
    capsys.readouterr()
    out_flagged, out_both = {}, {}
    _cli(args + ["--results_dir=" + plain] + RUN)
    _cli(args + ["--results_dir=" + flagged, "--predictive_checks_groups=m"] + RUN, out=out_flagged)
    _cli(args + ["--results_dir=" + both, "--predictive_checks_groups=m", "--predictive_checks_redraw=m"] + RUN, out=out_both)
    text = capsys.readouterr().out
    assert text.count("posterior predictive checks over 1659 observations") == 3
    assert text.count("grouped predictive checks by m: 13 groups (0 empty, 0 observations in none), 8192 draws") == 2
    assert sum(1 for l in text.splitlines() if "grouped predictive checks by m" in l and "; mixed " in l) == 1
    path = lambda root, suffix: os.path.join(root, method + "_tied" + suffix)
    base, r, rb = (json.load(open(path(d, ".json"))) for d in (plain, flagged, both))
    # without the flag: no group key, no file; with it: its keys and its file, and nothing else changes
    assert not any(k.startswith("ppc_group") for k in base) and not os.path.exists(path(plain, "_ppc_groups.npz"))
    assert set(r) - set(base) == set(cli.PPC_GROUP_KEYS) and set(base) <= set(r) and set(cli.PPC_KEYS) <= set(base)
    assert set(rb) - set(r) == set(cli.PPC_MIXED_KEYS + cli.PPC_GROUP_MIXED_KEYS) and set(r) <= set(rb)
    for small, large in ((base, r), (r, rb)):
        for key in small:
            if "time" not in key:
                assert small[key] == large[key], key
    same_files(plain, flagged, method, ("_ppc.npz", "_rhat.npz", "_ess.npz"))
    same_files(flagged, both, method, ("_ppc.npz", "_rhat.npz", "_ess.npz"))
    assert os.path.exists(path(both, "_ppc_mixed.npz")) and not os.path.exists(path(flagged, "_ppc_mixed.npz"))
    order = [k for k in rb if k.startswith("ppc_")]
    assert tuple(order) == cli.PPC_KEYS + cli.PPC_MIXED_KEYS + cli.PPC_GROUP_KEYS + cli.PPC_GROUP_MIXED_KEYS
    # the side file against the wrappers, called here on the same draws
    z, zb = np.load(path(flagged, "_ppc_groups.npz")), np.load(path(both, "_ppc_groups.npz"))
    head = ["group_of", "groups", "model", "n_obs", "part", "y"]
    assert sorted(z.files) == sorted(head + GROUP_ARRAYS)
    assert sorted(zb.files) == sorted(head + GROUP_ARRAYS + ["mixed_" + name for name in GROUP_ARRAYS])
    for name in z.files:                                                     # the posterior block is the same with the redraw
        assert z[name].tobytes() == zb[name].tobytes(), name
    summary, group_of, names = direct(spec, "m", out_flagged, 3)
    assert str(z["part"]) == "m" and str(z["model"]) == "radon" and list(z["groups"]) == names == ["m[%d]" % g for g in range(13)]
    assert z["group_of"].dtype == np.int32 and np.array_equal(z["group_of"], group_of) and np.array_equal(z["n_obs"], summary.sizes)
    assert np.array_equal(z["group_of"], np.asarray(spec.raw["county"]).reshape(-1)) and z["n_obs"].sum() == 1659 == z["y"].size
    check_block(z, "", summary)
    want = check_keys(r, "ppc_group_", summary, names, cli, "m", 0)
    assert summary.draws_used == 8192 and all(np.isfinite(z[name]).all() for name in GROUP_ARRAYS)
    assert all(np.all((z["p_" + name] >= 0) & (z["p_" + name] <= 1)) for name in STATS)
    assert want["ppc_group_p_threshold"] == 0.005 / 13 and isinstance(want["ppc_group_extreme_groups"], list)
    # the groups' observed means are the counties' own
    for g in range(13):
        assert z["obs_mean"][g] == float(np.mean(z["y"][group_of == g].astype(np.float64)))
    # the mixed block: the same wrappers on rows redrawn here under the mixed check's seeds
    mixed, _, _ = direct(spec, "m", out_both, 3, mixed_parts=["m"])
    check_block(zb, "mixed_", mixed)
    want_mixed = check_keys(rb, "ppc_group_mixed_", mixed, names, cli, "m", 0)
    assert mixed.draws_used + mixed.draws_left_out == 8192 and mixed.draws_used > 0.99 * 8192
    assert not np.array_equal(zb["mixed_p_mean"], zb["p_mean"])
    # the times nest
    assert 0 < r["ppc_group_time_sec"][0] < r["ppc_time_sec"][0] <= r["diagnostics_time_sec"][0]
    assert 0 < rb["ppc_group_mixed_time_sec"][0] < rb["ppc_group_time_sec"][0] < rb["ppc_time_sec"][0]
    # the warning names exactly the extreme groups; analyze --ppc prints the line for the runs with the keys
    warned = [l for l in text.splitlines() if "WARNING: predictive p-value of the group mean" in l]
    posterior_extreme, mixed_extreme = want["ppc_group_extreme_groups"], want_mixed["ppc_group_mixed_extreme_groups"]
    assert len(warned) == (1 if posterior_extreme else 0) + (1 if posterior_extreme or mixed_extreme else 0)      # (one per run)
    for groups in (posterior_extreme, mixed_extreme):
        assert all(any(name in l for l in warned) for name in groups[:8])
    root = os.path.dirname(plain)
    for name, lines, with_mixed in (("plain", 0, False), ("flagged", 1, False), ("both", 1, True)):
        analyze.main(["--results_dir=" + root, "--model=" + name, "--ppc"])
        shown = capsys.readouterr().out
        assert shown.count("%s_tied: predictive p-values mean" % method) == 1
        assert shown.count("grouped predictive by m: 13 groups (0 empty, 0 observations in none)") == lines
        assert (", mixed " in shown.split("grouped predictive by")[-1]) == with_mixed if lines else True
    with capsys.disabled():
        print("radon MA by m, 8192 draws: ppc_group_time_sec %.3f of ppc_time_sec %.3f; with the redraw %.3f (mixed pass %.3f) of %.3f; "
              "p mean %.4g (%s) ... %.4g (%s), mixed %.4g (%s) ... %.4g (%s); extreme %s, mixed %s" % (
                  r["ppc_group_time_sec"][0], r["ppc_time_sec"][0], rb["ppc_group_time_sec"][0], rb["ppc_group_mixed_time_sec"][0],
                  rb["ppc_time_sec"][0], want["ppc_group_p_mean_min"], want["ppc_group_p_mean_min_group"], want["ppc_group_p_mean_max"],
                  want["ppc_group_p_mean_max_group"], want_mixed["ppc_group_mixed_p_mean_min"], want_mixed["ppc_group_mixed_p_mean_min_group"],
                  want_mixed["ppc_group_mixed_p_mean_max"], want_mixed["ppc_group_mixed_p_mean_max_group"],
                  want["ppc_group_extreme_groups"], want_mixed["ppc_group_mixed_extreme_groups"]))


def test_election_by_state(gpu, tmp_path, capsys):
    """Bernoulli data, empty groups and observations in no group: the nulls and the sd rule"""
    from autoreparam_amd import main as cli, models
    spec = models.spec_by_name("election")
    root, out = str(tmp_path / "run"), {}
    tuned(root, "election", [], "CP")
    capsys.readouterr()
    _cli(common("election", [], "CP") + ["--results_dir=" + root, "--predictive_checks_groups=a"] + RUN, out=out)
    text = capsys.readouterr().out
    assert text.count("grouped predictive checks by a: 51 groups (3 empty, 15 observations in none), 8192 draws") == 1
    r = json.load(open(os.path.join(root, "CP_tied.json")))
    z = np.load(os.path.join(root, "CP_tied_ppc_groups.npz"))
    summary, group_of, names = direct(spec, "a", out, 3)
    check_block(z, "", summary)
    want = check_keys(r, "ppc_group_", summary, names, cli, "a", 15)
    assert r["ppc_groups"] == [51] and r["ppc_groups_empty"] == [3] and r["ppc_group_observations_left_out"] == [15]
    assert r["ppc_group_draws"] == [8192] and r["ppc_group_part"] == ["a"]
    empty = z["n_obs"] == 0
    assert empty.sum() == 3 and z["n_obs"].sum() == 11566 - 15 and int(np.sum(z["group_of"] < 0)) == 15
    for name in STATS:
        assert np.all(np.isnan(z["p_" + name][empty])) and np.all(np.isnan(z["rep_" + name][empty])), name
    for name in ("sd", "min", "max"):                                        # Bernoulli data define none of them
        assert all(np.all(np.isnan(z["%s_%s" % (what, name)])) for what in ("p", "rep", "obs")), name
    for name in ("mean", "deviance"):
        assert np.all(np.isfinite(z["p_" + name][~empty])) and np.all((z["p_" + name][~empty] >= 0) & (z["p_" + name][~empty] <= 1))
    for key in ("ppc_group_p_sd_min", "ppc_group_p_sd_min_group", "ppc_group_p_sd_max", "ppc_group_p_sd_max_group"):
        assert r[key] == [None], key
    for key in ("ppc_group_p_mean_min", "ppc_group_p_mean_max", "ppc_group_p_deviance_min", "ppc_group_p_deviance_max"):
        assert math.isfinite(r[key][0]) and r[key.replace("_min", "_min_group").replace("_max", "_max_group")][0] in names, key
    # 48 states share 0.005: 8 192 draws cannot resolve 1.04e-4, so no group is named and no warning is printed
    assert r["ppc_group_p_threshold"] == [0.005 / 48] and r["ppc_group_extreme_groups"] == [None]
    assert "WARNING: predictive p-value of the group mean" not in text
    assert not any(k.startswith("ppc_group_mixed") or k.startswith("ppc_mixed") for k in r)
    with capsys.disabled():
        print("election by a, 8192 draws: ppc_group_time_sec %.3f of ppc_time_sec %.3f; p mean %.4g (%s) ... %.4g (%s)" % (
            r["ppc_group_time_sec"][0], r["ppc_time_sec"][0], want["ppc_group_p_mean_min"], want["ppc_group_p_mean_min_group"],
            want["ppc_group_p_mean_max"], want["ppc_group_p_mean_max_group"]))


def test_a_refused_part_raises_before_the_run(gpu, tmp_path):
    with pytest.raises(ValueError, match="--predictive_checks_groups: b2 has one element"):
        _cli(["--model=radon", "--dataset=MA", "--num_chains=64", "--method=CP", "--inference=HMC", "--predictive_checks",
              "--predictive_checks_groups=b2", "--results_dir=" + str(tmp_path)] + HM)
    assert os.listdir(str(tmp_path)) == []
