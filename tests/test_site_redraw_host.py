"""CPU: the host half of the mixed predictive check -- diagnostics.redraw_selection on every model's real site table (the
natural selections and the refusals, with the parts a refusal names), the invariants of the float64 restatement of
arp_site_redraw (tests/site_redraw_ref.py), the share of undecided log-Gamma attempts among the FLAGGED elements of
every input the GPU parity test uses (the condition that test relies on), the flag with its refusals and its null keys,
the pure-Python keys, the wrapper's refusals, analyze --ppc's second line, and the ABI entry.

The inputs of tests/test_gpu_site_redraw.py are defined here (NATURAL, parity_cases, INPUT_SEED) so that both files speak
of the same ones; SEED, DRAWS and the cap are tests/test_prior_draw_host.py's."""
import json
import os
import re

import numpy as np
import pytest
import torch

import prior_draw_ref as pr
import site_redraw_ref as rr
from test_prior_draw_host import DRAWS, SEED, UNDECIDED_CAP, rounded, synthetic_chain
from test_site_table_host import SPECS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUT_SEED = SEED ^ 1                # the recorded rows of the GPU tests: site_prior_draws under ANOTHER seed than the redraw's
# the group-level parts of every model with data: what a mixed predictive check of it redraws
NATURAL = (("8schools", "theta"), ("radon_MN", "m"), ("radon_stddvs", "m"), ("election", "a"), ("electric", "a"),
           ("german_credit_lognormalcentered", "beta"), ("german_credit_lognormalcentered", "beta_log_scales,beta"),
           ("german_credit_gammascale", "beta"), ("german_credit_gammascale", "beta_log_scales,beta"))
TIME_SERIES_ALL = ",".join("alpha%d,mu%d" % (i, i) for i in range(60))


def selection(spec, text):
    from autoreparam_amd import diagnostics
    return diagnostics.redraw_selection(spec.site_table(), spec.part_names, text.split(","))


def parity_cases():
    """(what, models.SiteTable, D, flags [D] uint8) of every case of the GPU parity test"""
    from autoreparam_amd import models
    for name, text in NATURAL + (("time_series", TIME_SERIES_ALL),):
        spec = SPECS[name](models)
        yield "%s: %s" % (name, text if len(text) < 40 else text[:37] + "..."), spec.site_table(), spec.D, selection(spec, text)
    chain = synthetic_chain(255)
    yield "synthetic D=255, every third", chain, 255, (np.arange(255) % 3 == 2).astype(np.uint8)     # the log-Gamma elements
    yield "synthetic D=255, every third from 1", chain, 255, (np.arange(255) % 3 == 1).astype(np.uint8)
    yield "synthetic D=255, the tail", chain, 255, (np.arange(255) >= 100).astype(np.uint8)


@pytest.mark.parametrize("name,text", NATURAL)
def test_natural_selections_flag_whole_parts(name, text):
    from autoreparam_amd import models
    spec = SPECS[name](models)
    flags = selection(spec, text)
    assert flags.dtype == np.uint8 and flags.shape == (spec.D,)
    part = np.asarray(spec.site_table().part)
    want = np.isin(part, [spec.part_names.index(n) for n in text.split(",")])
    assert np.array_equal(flags != 0, want) and 0 < flags.sum() < spec.D
    if "," in text:                                                          # the order given does not matter
        assert np.array_equal(flags, selection(spec, ",".join(reversed(text.split(",")))))


def test_time_series_takes_its_parts_one_by_one():
    from autoreparam_amd import models
    spec = SPECS["time_series"](models)
    flags = selection(spec, TIME_SERIES_ALL)
    assert int(flags.sum()) == 120 and spec.D == 123
    assert int(selection(spec, "alpha59,mu59").sum()) == 2                   # the last step hangs on nothing that is redrawn
    with pytest.raises(ValueError, match=r"--predictive_checks_redraw: alpha1, alpha2, .*alpha59 would stay as recorded although "
                                         r"drawn from what is redrawn \(alpha0\).*add alpha1,alpha2,.*the model's parts: sigma_alpha"):
        selection(spec, "alpha0")


@pytest.mark.parametrize("name,text,missing", (
    ("radon_MN", "mua", "m"), ("radon_MN", "b1", "m"), ("radon_stddvs", "mua", "m"), ("8schools", "log_tau", "theta"),
    ("election", "log_sigma_a", "a"), ("german_credit_gammascale", "beta_log_scales", "beta"),
    ("german_credit_lognormalcentered", "beta_log_scales", "beta"),
    ("german_credit_lognormalcentered", "overall_log_scale", "beta_log_scales, beta")))
def test_a_selection_that_is_not_closed_is_refused_and_names_what_to_add(name, text, missing):
    from autoreparam_amd import models
    spec = SPECS[name](models)
    with pytest.raises(ValueError) as e:
        selection(spec, text)
    message = str(e.value)
    assert message.startswith("--predictive_checks_redraw: %s would stay as recorded" % missing)
    assert "add %s;" % missing.replace(", ", ",") in message and "the model's parts: " + ", ".join(spec.part_names) in message
    selection(spec, text + "," + missing.replace(", ", ","))                 # with them, it is taken


def test_the_log_gamma_form_does_not_hang_on_its_loc_terms():
    """A log-Gamma element's loc terms are not read (arp_site_logprior): a flagged element they point at does not bind it"""
    from autoreparam_amd import diagnostics
    table = synthetic_chain(6)                                               # forms 0 1 2 0 1 2; element 2 hangs on 0 and 1
    table.scale_w[2] = 0.0
    table.scale_w[3:], table.loc_w[3:] = 0.0, 0.0
    names = ["p%d" % d for d in range(6)]
    table = table._replace(part=np.arange(6, dtype=np.int32))
    assert diagnostics.redraw_selection(table, names, ["p1"]).tolist() == [0, 1, 0, 0, 0, 0]
    table.scale_w[2, 0] = 0.25                                               # idx[2] = (1, 0): now its RATE hangs on element 1
    with pytest.raises(ValueError, match="p2 would stay as recorded"):
        diagnostics.redraw_selection(table, names, ["p1"])


@pytest.mark.parametrize("text,word", (("theta,tau", "tau is no latent part of the model"), ("theta,theta", "theta is named twice"),
                                       ("theta,", "an empty name"), ("", "an empty name")))
def test_names_that_are_refused(text, word):
    from autoreparam_amd import models
    spec = SPECS["8schools"](models)
    with pytest.raises(ValueError, match="--predictive_checks_redraw: %s.*the model's parts: mu, log_tau, theta" % word):
        selection(spec, text)


def test_reference_invariants():
    """All flagged: prior_draw_ref.draw without parents, whatever the input holds; none flagged: the input; teacher
    forcing on the reference's own rows changes nothing; a flagged element reads its parents from the row being built"""
    table = rounded(synthetic_chain(12), 12)
    n = 70
    own = pr.draw(table, n, SEED, 5)
    nan = np.full((n, 12), np.nan)
    every = rr.redraw(table, nan, np.ones(12), SEED, 5)
    assert np.array_equal(every.x, own.x) and not every.undrawn.any()
    x = pr.draw(table, n, INPUT_SEED, 0).x.astype(np.float32).astype(np.float64)
    none = rr.redraw(table, x, np.zeros(12), SEED, 5)
    assert np.array_equal(none.x, x)
    flags = (np.arange(12) >= 7).astype(np.uint8)
    tail = rr.redraw(table, x, flags, SEED, 5)
    assert np.array_equal(tail.x[:, :7], x[:, :7]) and not np.array_equal(tail.x[:, 7:], x[:, 7:])
    assert not np.array_equal(tail.x[:, 7:], own.x[:, 7:])                   # other parents than the prior draw's own
    assert np.array_equal(rr.redraw(table, x, flags, SEED, 5, parents=tail.x).x, tail.x)
    # element 7 is form 1 and hangs on 5 and 6, which are recorded: loc + sigma z from THOSE
    want = pr.draw(table, n, SEED, 5, parents=x).x[:, 7]
    assert np.array_equal(tail.x[:, 7], want)
    # element 8 (form 2) hangs on 6 (recorded) and 7 (redrawn)
    mixed = x.copy()
    mixed[:, 7] = want
    assert np.array_equal(tail.x[:, 8], pr.draw(table, n, SEED, 5, parents=mixed).x[:, 8])


def test_undecided_share_among_the_flagged_elements_of_the_gpu_tests_inputs():
    """The condition the GPU parity test relies on.  The accept test of the log-Gamma form reads the Philox words alone,
    not the parents: the undecided attempts of a redraw under (SEED, offset 0) are those of prior_draw_ref.draw under the
    same, whatever rows are recorded -- here counted over the FLAGGED log-Gamma elements of every case, at most 1 in 1 000."""
    seen = 0
    drawn = {}
    for what, table, D, flags in parity_cases():
        host = rounded(table, D)
        key = (D, np.asarray(host.loc0).tobytes())
        if key not in drawn:
            drawn[key] = pr.draw(host, DRAWS, SEED, 0)
        d = drawn[key]
        flagged_gamma = (np.asarray(host.form) == pr.LOG_GAMMA) & (flags != 0)
        assert not d.undrawn.any(), what
        if not flagged_gamma.any():
            continue
        marks = rr.undecided(host, d, flags)
        assert not marks[:, ~flagged_gamma].any()
        share = marks[:, flagged_gamma].mean()
        seen += int(flagged_gamma.sum()) * DRAWS
        print("%s: %d of %d flagged log-Gamma elements undecided (share %.2g)" % (what, int(marks.sum()), int(flagged_gamma.sum()) * DRAWS, share))
        assert share <= UNDECIDED_CAP, (what, share)
        # ... and the recorded rows do not enter: the same marks from a redraw of other rows
        if D <= 125:
            x = pr.draw(host, 256, INPUT_SEED, 0).x
            again = rr.undecided(host, rr.redraw(host, x, flags, SEED, 0), flags)
            assert np.array_equal(again, marks[:256]), what
    assert seen > 0


def test_flag_refusals_and_unchanged_keys(capsys):
    from autoreparam_amd import main, models
    from autoreparam_amd.flags import FlagValues
    f = FlagValues()
    assert f.predictive_checks_redraw == "" and main.redraw_parts(f) == []
    main.check_predictive_redraw(f)
    f.parse(["--model=radon", "--predictive_checks_redraw=m"])
    with pytest.raises(ValueError, match="--predictive_checks_redraw is read with --predictive_checks only"):
        main.check_predictive_redraw(f)
    with pytest.raises(ValueError, match="--predictive_checks_redraw is read with --predictive_checks only"):
        main.main([], flags=f)
    f.parse(["--predictive_checks"])
    main.check_predictive_redraw(f)
    f.parse(["--predictive_checks_redraw=mua"])
    with pytest.raises(ValueError, match="--predictive_checks_redraw: m would stay as recorded .*add m; the model's parts: mua, b1, b2, m"):
        main.main([], flags=f)
    f.parse(["--predictive_checks_redraw=m,sigma"])
    with pytest.raises(ValueError, match="sigma is no latent part of the model; the model's parts: mua, b1, b2, m"):
        main.check_predictive_redraw(f)
    f.parse(["--model=neals_funnel", "--predictive_checks_redraw=x2", "--nopredictive_checks"])
    with pytest.raises(ValueError, match="read with --predictive_checks only"):
        main.check_predictive_redraw(f)
    f.parse(["--predictive_checks"])
    with pytest.raises(ValueError, match="--predictive_checks_redraw: neals_funnel has no observations"):
        main.check_predictive_redraw(f)

    # the null path: the posterior check's keys and message, the mixed keys behind them without a message of their own
    class Results(object):
        trace = None
    cfg = type("Cfg", (), {"model": models._spec_eight_schools()})()
    f = FlagValues()
    f.parse(["--predictive_checks", "--predictive_checks_redraw=theta"])
    capsys.readouterr()
    keys, arrays = main._convergence_report(Results(), cfg, f, None)
    assert arrays is None and tuple(keys) == main.PPC_KEYS + main.PPC_MIXED_KEYS and all(v is None for v in keys.values())
    text = capsys.readouterr().out
    assert text.count("posterior predictive checks: not computed") == 1 and "mixed" not in text
    f.parse(["--predictive_checks_redraw="])
    keys, _ = main._convergence_report(Results(), cfg, f, None)
    assert tuple(keys) == main.PPC_KEYS                                      # without the flag: the key set as it was
    assert main.PPC_KEYS == ("ppc_draws", "ppc_draws_left_out", "ppc_chains", "ppc_steps", "ppc_observations", "ppc_p_mean",
                             "ppc_p_sd", "ppc_p_min", "ppc_p_max", "ppc_p_deviance", "ppc_rep_mean", "ppc_rep_sd", "ppc_obs_mean",
                             "ppc_obs_sd", "ppc_pit_ks", "ppc_coverage_90", "ppc_time_sec")
    assert all(k.startswith("ppc_mixed_") for k in main.PPC_MIXED_KEYS) and not set(main.PPC_MIXED_KEYS) & set(main.PPC_KEYS)


def test_the_side_file_is_written_next_to_the_posterior_one(tmp_path):
    """The mixed arrays wait under PPC_MIXED_ARRAYS among those of <base>_ppc.npz; save_ppc gives them a file of their own
    and <base>_ppc.npz holds what it holds without the flag"""
    from collections import OrderedDict
    from autoreparam_amd import main
    plain = OrderedDict([("pit", np.arange(3.0)), ("model", np.asarray("radon"))])
    flagged = OrderedDict(plain)
    flagged[main.PPC_MIXED_ARRAYS] = OrderedDict([("parts", np.asarray(["m"])), ("redrawn", np.ones(4, np.uint8)), ("pit", np.ones(3))])
    main.save_ppc(str(tmp_path / "a"), plain)
    main.save_ppc(str(tmp_path / "b"), flagged)
    assert sorted(os.listdir(str(tmp_path))) == ["a_ppc.npz", "b_ppc.npz", "b_ppc_mixed.npz"]
    a, b, mixed = (np.load(str(tmp_path / name)) for name in ("a_ppc.npz", "b_ppc.npz", "b_ppc_mixed.npz"))
    assert sorted(a.files) == sorted(b.files) == ["model", "pit"] and all(a[k].tobytes() == b[k].tobytes() for k in a.files)
    assert sorted(mixed.files) == ["parts", "pit", "redrawn"] and list(mixed["parts"]) == ["m"]
    assert main.PPC_MIXED_ARRAYS in flagged                                  # (the caller's dict is left as it was)
    assert main.PPC_MIXED_ARRAYS not in [row.tag for row in main.SIDE_REPORTS]


def columns(y_rep):
    N, R = y_rep.shape
    zero = np.zeros(R)
    return np.stack([y_rep.sum(0), (y_rep ** 2).sum(0), y_rep.min(0), y_rep.max(0), zero, zero, zero, np.full(R, float(N))], axis=1)


def test_mixed_keys_from_a_summary():
    from autoreparam_amd import diagnostics, main
    y = np.array([0.0, 1.0, 2.0, 3.0])
    y_rep = np.arange(1.0, 21.0)[None, :] + np.array([-1.5, -0.5, 0.5, 1.5])[:, None]
    sums = np.zeros((4, 4))
    sums[:, 2] = 20 * np.array([0.5, 0.004, 0.995, 0.2])                     # the PIT sums over 20 draws
    keys = main.ppc_mixed_keys(diagnostics.ppc_summary(columns(y_rep), sums, y, 0), ["theta"], 8, 0)
    assert tuple(keys) == main.PPC_MIXED_KEYS[:-1]
    assert keys["ppc_mixed_parts"] == ["theta"] and keys["ppc_mixed_elements"] == 8 and keys["ppc_mixed_draws"] == 20
    assert keys["ppc_mixed_p_mean"] == 19 / 20.0 and keys["ppc_mixed_draws_left_out"] == 0
    assert keys["ppc_mixed_pit_extreme_observations"] == [1, 2] and keys["ppc_mixed_pit_min_observation"] == 1
    json.dumps(keys)
    # Bernoulli data: the nulls of the posterior keys, and no per-observation PIT keys either
    yb = np.array([1.0, 0.0, 0.0, 1.0])
    kb = main.ppc_mixed_keys(diagnostics.ppc_summary(columns((y_rep > 9).astype(float)), sums, yb, 1), ["beta"], 62, 1)
    posterior = main.ppc_keys(diagnostics.ppc_summary(columns((y_rep > 9).astype(float)), sums, yb, 1), 4, 5)
    for name in ("p_mean", "p_sd", "p_min", "p_max", "p_deviance", "rep_mean", "rep_sd", "pit_ks", "coverage_90"):
        assert (kb["ppc_mixed_" + name] is None) == (posterior["ppc_" + name] is None), name
    assert kb["ppc_mixed_p_sd"] is None and kb["ppc_mixed_p_mean"] is not None
    assert kb["ppc_mixed_pit_extreme_observations"] is None and kb["ppc_mixed_pit_min_observation"] is None
    # no draw used: everything that is a figure is null
    none = main.ppc_mixed_keys(diagnostics.ppc_summary(columns(y_rep), sums, y, 0, np.ones(20)), ["theta"], 8, 0)
    assert none["ppc_mixed_draws"] == 0 and none["ppc_mixed_p_mean"] is None and none["ppc_mixed_pit_extreme_observations"] is None


def test_analyze_prints_the_second_line(tmp_path, capsys):
    from autoreparam_amd import analyze, main
    d = tmp_path / "radon_MA"
    d.mkdir()
    run = {key: 0.5 for key in main.PPC_KEYS + main.PPC_MIXED_KEYS}
    run.update(ppc_observations=1659, ppc_draws=5120, ppc_chains=256, ppc_draws_left_out=0, ppc_p_sd=0.48, ppc_pit_ks=0.021,
               ppc_mixed_parts=["m"], ppc_mixed_elements=13, ppc_mixed_draws=5119, ppc_mixed_draws_left_out=1,
               ppc_mixed_p_sd=0.003, ppc_mixed_pit_ks=0.087, ppc_mixed_pit_extreme_observations=[4, 77, 1003],
               ppc_mixed_pit_min_observation=77)
    (d / "NCP_tied.json").write_text(json.dumps({k: [None, v] for k, v in run.items()}))
    plain = {k: [v] for k, v in run.items() if k in main.PPC_KEYS}
    (d / "CP_tied.json").write_text(json.dumps(plain))
    (d / "cVIP_eig_tied.json").write_text(json.dumps({k: [None] for k in main.PPC_KEYS + main.PPC_MIXED_KEYS}))
    analyze.main(["--results_dir", str(tmp_path), "--model", "radon_MA", "--ppc"])
    out = capsys.readouterr().out
    lines = out.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("NCP_tied:")]
    assert len(at) == 1 and lines[at[0] + 1].startswith("      mixed predictive, m redrawn (13 elements):")
    second = lines[at[0] + 1]
    assert "sd 0.003 (posterior 0.48)" in second and "PIT Kolmogorov distance 0.087 (posterior 0.021)" in second
    assert "3 observation(s) with an extreme mixed PIT" in second and "5119 draws, 1 left out" in second
    assert second.endswith("<-- EXTREME: sd")
    assert out.count("mixed predictive") == 1                                # not for the run without the keys
    assert "CP_tied: predictive p-values" in out and "cVIP_eig_tied: posterior predictive checks not computed" in out


def test_symbol_is_declared_and_listed():
    from autoreparam_amd import _lib
    src = open(os.path.join(ROOT, "include", "autoreparam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)                          # as tests/test_abi.py reads the header
    declared = sorted(set(re.findall(r"\b(arp_[a-z_0-9]+)\s*\(", src)))
    assert "arp_site_redraw" in declared and "arp_site_redraw" in _lib.SYMBOLS
    assert sorted(declared) == sorted(_lib.SYMBOLS)
    csrc = os.path.join(ROOT, "autoreparam_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "site_redraw.hip"))
    # one copy of the drawing code: both kernels call the header's function and neither holds a Philox call of its own
    for name in ("prior_draw.hip", "site_redraw.hip"):
        code = re.sub(r"//.*", "", open(os.path.join(csrc, name)).read())
        assert '#include "site_draw.h"' in code and "site_draw_element(" in code and "philox4x32_10" not in code, name


def test_wrapper_refuses_what_the_kernel_refuses():
    from autoreparam_amd import diagnostics
    up = diagnostics.upload_site_table(synthetic_chain(6), 6, "cpu")
    trace = torch.zeros(2, 3, 6)
    flags = np.array([0, 0, 0, 1, 1, 1], np.uint8)
    with pytest.raises(ValueError, match="DeviceSiteTable"):
        diagnostics.site_redraw(trace, synthetic_chain(6), flags)
    with pytest.raises(ValueError, match="draw_offset"):
        diagnostics.site_redraw(trace, up, flags, draw_offset=-1)
    for bad in (flags[:5], np.zeros((6, 1), np.uint8), np.zeros(6), torch.zeros(6)):
        with pytest.raises(ValueError, match=r"redraw must be \[6\] flags"):
            diagnostics.site_redraw(trace, up, bad)
    with pytest.raises(ValueError, match="on the GPU"):
        diagnostics.site_redraw(trace, up, flags)
    with pytest.raises(ValueError, match="on the GPU"):
        diagnostics.site_redraw(trace, up, flags.astype(bool))
