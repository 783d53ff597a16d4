"""Pretty-printer for the result files main.py writes (reference analyze.py:30-185):

    python -m autoreparam_amd.analyze --results_dir=. --model=radon_MN --elbos --ess --rhat --energy --trajectory --geometry --loo --ppc --vi --sbc --reparams
    python -m autoreparam_amd.analyze --loo_compare=radon_MN/CP_tied_loo.npz,radon_stddvs_MN/CP_tied_loo.npz
    python -m autoreparam_amd.analyze --logo_compare=radon_MN/CP_tied_logo.npz,radon_stddvs_MN/CP_tied_logo.npz

The reference's method list is stale (`cVIP_exp_tied`, analyze.py:19-26) and it expects a
`num_leapfrog_steps` key that main.py only writes for interleaved runs; here every
`<method>.json` found in the model's directory is reported and the leapfrog count of a
plain HMC run is recovered from its best tuning run (main.py:292-294).
"""
import argparse
import glob
import json
import os

import numpy as np


def _fmt(v, spec="{:.4g}"):
    return "n/a" if v is None else spec.format(v)


def _secs(t):
    return _fmt(t, "{:.3f}s")


def _last(r, prefixes):
    return {k: v[-1] for k, v in r.items() if k.startswith(prefixes)}


def load(results_dir, model_name):
    out = {}
    for path in sorted(glob.glob(os.path.join(results_dir, model_name, "*.json"))):
        with open(path) as f:
            out[os.path.basename(path)[:-5]] = json.load(f)
    return out


def leapfrog_steps(res):
    if "num_leapfrog_steps" in res:
        return res["num_leapfrog_steps"][-1]
    runs = res.get("tuning_runs")
    return max(runs, key=lambda d: d["ess_min"])["num_leapfrog_steps"] if runs else None


def report_elbos(results):
    lines = []
    for m, r in results.items():
        if "elbo" in r:
            lines.append("{0:.4f} +/- {1:.2f}   : {2}".format(r["elbo"], r["estimated_elbo_std"], m))
    return lines


def report_reparams(results):
    lines = []
    for m, r in results.items():
        if m.startswith("cVIP") and r.get("learned_reparam"):
            lines.append("   {}".format(m))
            for k, v in r["learned_reparam"].items():
                lines.append("{:>10}: {}".format(k, np.array(v, np.float32)))
    return lines


def report_ess(results, normalize_times=False, num_samples=10000):
    lines = []
    vi_times = {m: r.get("variational_fit_time_secs") for m, r in results.items()}
    base = next((m for m in results if m.startswith("CP")), None)
    for m, r in results.items():
        if "ess_min" not in r:
            continue
        L = leapfrog_steps(r)
        ess, sem, t = r["ess_min"][-1], r["sem_min"][-1], r["mcmc_time_sec"][-1]
        if not normalize_times:
            lines.append("{} +/- {} : {} ({} leapfrog steps)".format(r["ess_min"], r["sem_min"], m, L))
            continue
        per_sample = 2 * L if m.startswith("i") else L
        if m.startswith("i"):
            vi = sum(v for k, v in vi_times.items() if k.startswith(("CP", "NCP")) and v)
        else:
            vi = vi_times.get(m) or 0.0
        grads = per_sample * float(num_samples)
        line = "{} +/- {} in {}s ({}s VI + {}s MCMC): {} ({} leapfrog steps".format(
            ess * grads / 1000.0, sem * grads / 1000.0, vi + t, vi, t, m, L)
        if base and "mcmc_time_sec" in results[base] and vi_times.get(base):
            Lb = leapfrog_steps(results[base])
            rel_vi = (vi / 3000.0) / (vi_times[base] / 3000.0) if vi else float("nan")
            rel_mc = (t / (num_samples * per_sample)) / (results[base]["mcmc_time_sec"][-1] / (num_samples * Lb))
            line += ", {:.2f}x/{:.2f}x CP time per VI/MCMC step".format(rel_vi, rel_mc)
        lines.append(line + ")")
    return lines


def report_rhat(results, results_dir=None, model_name=None, threshold=1.01):
    """Build-specific: the convergence diagnostics of every sampling run that recorded them (split R-hat over the chains
    whose trace was kept; for a streaming run the un-split R-hat of all chains next to it), the last run of each file,
    and -- where <method>_rhat.npz is at hand -- the elements above the customary threshold."""
    lines = []
    for m, r in results.items():
        if "split_rhat_max" not in r:
            continue
        fmt = lambda v: _fmt(v, "{:.4f}")
        ranked = "rank_rhat_max" in r                      # (--rank_normalized_rhat runs only)
        worst = max((v for v in (r["split_rhat_max"][-1], r["rhat_max_all_chains"][-1],
                                 r["rank_rhat_max"][-1] if ranked else None) if v is not None), default=None)
        rank_cols = "" if not ranked else " rank-normalised max {} (bulk {}, tail {}) over {} chains, {};".format(
            fmt(r["rank_rhat_max"][-1]), fmt(r["rank_rhat_bulk_max"][-1]), fmt(r["rank_rhat_tail_max"][-1]),
            r["rank_rhat_chains"][-1],
            _secs(r["rank_rhat_time_sec"][-1]))
        line = "split R-hat max {} over {} chains; all chains (un-split) {};{} {:.3f}s : {}{}".format(
            fmt(r["split_rhat_max"][-1]), r["split_rhat_chains"][-1], fmt(r["rhat_max_all_chains"][-1]), rank_cols,
            r["diagnostics_time_sec"][-1], m, "" if worst is None or worst <= threshold else "   <-- NOT CONVERGED")
        lines.append(line)
        if "ess_bulk_min" in r:                            # (--bulk_tail_ess runs only)
            num = lambda v: _fmt(v, "{:.1f}")
            lines.append("      multi-chain ESS min: bulk {}, tail {}, mean {}; largest MCSE of a mean {} sd; over {} chains, {}".format(
                num(r["ess_bulk_min"][-1]), num(r["ess_tail_min"][-1]), num(r["ess_mean_min"][-1]),
                fmt(r["mcse_mean_over_sd_max"][-1]), r["bulk_tail_ess_chains"][-1],
                _secs(r["bulk_tail_ess_time_sec"][-1])))
        if "nested_rhat_max" in r:                         # (--superchain_size runs only)
            lines.append("      nested R-hat max {} over {} superchains of {} ({} chains, {} left out; stationary floor {}); "
                         "by step: first {}, last {}; {}".format(
                fmt(r["nested_rhat_max"][-1]), r["nested_rhat_superchains"][-1], r["nested_rhat_superchain_size"][-1],
                r["nested_rhat_chains"][-1], r["nested_rhat_left_out"][-1], fmt(r["nested_rhat_floor"][-1]),
                fmt(r["nested_rhat_first_step_max"][-1]), fmt(r["nested_rhat_last_step_max"][-1]),
                _secs(r["nested_rhat_time_sec"][-1])))
        path = os.path.join(results_dir or ".", model_name or "", m + "_rhat.npz")
        if os.path.exists(path):
            z = np.load(path)
            for key in z.files:
                if key.startswith(("split_rhat/", "rhat_all_chains/", "rank_rhat_bulk/", "rank_rhat_tail/")):
                    v = np.asarray(z[key], np.float64)
                    bad = np.argwhere(v > threshold)
                    if len(bad):
                        lines.append("      {}: {} element(s) above {}, worst {:.4f} at {}".format(
                            key, len(bad), threshold, np.nanmax(v), tuple(int(i) for i in np.unravel_index(np.nanargmax(v), v.shape))))
    return lines


def report_energy(results, results_dir=None, model_name=None):
    """Build-specific: the energy probe of every sampling run that recorded one (--energy_diagnostics; the last run of each
    file): fresh-momentum trajectories from the run's final and recorded states, not a replay of the transitions the
    sampler took -- and, where <method>_energy.npz is at hand, where the divergent ones started."""
    lines = []

    def row(d):
        return ("{} of {} trajectories divergent (rate {}, {} not finite); energy error {} +/- {}; expected acceptance {}; "
                "kinetic share of the energy variance {}").format(
                    d["divergent_trajectories"], d["energy_probe_trajectories"], _fmt(d["divergence_rate"]), d["energy_nonfinite"],
                    _fmt(d["energy_error_mean"]), _fmt(d["energy_error_sd"]), _fmt(d["energy_accept_prob"]),
                    _fmt(d["energy_kinetic_share"]))
    for m, r in results.items():
        if "divergence_rate" not in r:
            continue
        last = _last(r, ("divergen", "energy_"))
        lines.append("{}; {:.3f}s : {}{}".format(row(last), last["energy_time_sec"], m,
                                                 "   <-- DIVERGENT" if last["divergent_trajectories"] else ""))
        for j, d in enumerate(last.get("energy_by_kernel") or []):
            lines.append("      kernel {}: {}".format(j, row(d)))
        path = os.path.join(results_dir or ".", model_name or "", m + "_energy.npz")
        if os.path.exists(path) and last["divergent_trajectories"]:
            z = np.load(path)
            for key in z.files:
                if key.startswith("divergent_where/") and len(z[key]):
                    v = np.asarray(z[key], np.float64).reshape(len(z[key]), -1)
                    lines.append("      {}: over {} divergent start(s), mean {:.4g}, min {:.4g}, max {:.4g}".format(
                        key, len(v), np.nanmean(v), np.nanmin(v), np.nanmax(v)))
    return lines


def report_trajectory(results, results_dir=None, model_name=None):
    """Build-specific: the trajectory-length profile of every sampling run that recorded one (--trajectory_profile; the
    last run of each file), one table per inner kernel: for every leapfrog count the expected acceptance, the rate of
    divergent trajectories and the worst element's expected squared jump distance, whole and per gradient.  Fresh-momentum
    trajectories with the step sizes the run adapted for its own count, not a replay of the sampler's transitions; a
    one-transition criterion, not an ESS."""
    lines = []
    for m, r in results.items():
        if "trajectory_leapfrogs_max" not in r:
            continue
        last = _last(r, "trajectory_")
        kernels = last.get("trajectory_by_kernel") or [last]
        for j, d in enumerate(kernels):
            lines.append("{}{}: trajectory profile over {} trajectories, {:.3f}s: best {} leapfrog step(s), the run took {} "
                         "(efficiency against the best {})".format(
                             m, "" if len(kernels) == 1 else " kernel %d" % j, last["trajectory_probe_trajectories"],
                             last["trajectory_time_sec"], _fmt(d["trajectory_best_leapfrogs"]), d["trajectory_run_leapfrogs"],
                             _fmt(d["trajectory_efficiency_vs_best"])))
            lines.append("    leapfrogs  accept  divergent  esjd_min (element)  per gradient")
            for l in range(last["trajectory_leapfrogs_max"]):
                mark = "  <-- best" if d["trajectory_best_leapfrogs"] == l + 1 else ""
                mark += "  <-- this run" if d["trajectory_run_leapfrogs"] == l + 1 else ""
                lines.append("    {:9d}  {:>6}  {:>9}  {:>8} ({:d})  {:>12}{}".format(
                    l + 1, _fmt(d["trajectory_accept_prob"][l]), _fmt(d["trajectory_divergence_rate"][l]),
                    _fmt(d["trajectory_esjd_min"][l]), d["trajectory_esjd_min_element"][l],
                    _fmt(d["trajectory_esjd_min_per_gradient"][l]), mark))
    return lines


def report_geometry(results, results_dir=None, model_name=None):
    """Build-specific: the posterior geometry report of every sampling run that recorded one (--geometry_diagnostics; the
    last run of each file), one line per inner kernel: the three condition numbers, the most correlated pair and the
    strongest scale coupling -- and, where <method>_geometry.npz is at hand, the elements that carry the stiff direction.
    A second-order summary pooled over chains, not a local metric; unconverged chains inflate it."""
    lines = []
    for m, r in results.items():
        if "geometry_rows" not in r:
            continue
        last = _last(r, "geometry_")
        kernels = last.get("geometry_by_kernel") or [last]
        for j, d in enumerate(kernels):
            lines.append("{}{}: condition number {} in the sampler's coordinates ({} scaled by its steps), {} centred; largest "
                         "|correlation| {} ({}); largest scale coupling {} ({}); {} draws of {} chains, {} left out; {}".format(
                             m, "" if len(kernels) == 1 else " kernel %d" % j, _fmt(d["geometry_condition_number"]),
                             _fmt(d["geometry_condition_number_step_scaled"]), _fmt(last["geometry_condition_number_centred"]),
                             _fmt(d["geometry_max_abs_correlation"]), " ~ ".join(d["geometry_max_correlation_pair"] or ["n/a"]),
                             _fmt(d["geometry_max_scale_coupling"]), " -> ".join(d["geometry_max_scale_coupling_pair"] or ["n/a"]),
                             last["geometry_rows"], last["geometry_chains"], last["geometry_rows_left_out"],
                             _secs(last.get("geometry_time_sec"))))
        path = os.path.join(results_dir or ".", model_name or "", m + "_geometry.npz")
        if os.path.exists(path):
            z = np.load(path)
            names = [str(n) for n in z["elements"]]
            for j in range(len(kernels)):
                tag = "" if j == 0 else "_%d" % j
                parts = [np.asarray(z[key], np.float64).reshape(-1) for key in z.files
                         if key.startswith("stiffest_direction%s/" % tag)]
                if not parts:
                    continue
                v = np.concatenate(parts)
                top = np.argsort(-np.abs(v))[:3]
                lines.append("      stiffest direction{}: {}".format(
                    "" if len(kernels) == 1 else " of kernel %d" % j,
                    ", ".join("{} {:+.3f}".format(names[i] if i < len(names) else i, v[i]) for i in top)))
    return lines


def report_loo(results):
    """Build-specific: the predictive report of every sampling run that recorded one (--predictive_diagnostics; the last
    run of each file): elpd_loo and elpd_waic with their standard errors, the effective numbers of parameters, and the
    worst Pareto k-hat against its threshold.  No r_eff correction, no moment matching, no K-fold.  A run with
    --loo_predictive gets a second line: the calibration of the LOO-PIT (with the posterior PIT's of --predictive_checks
    next to it where recorded), RMSE and R^2 or Brier score and accuracy, and the smallest importance-sampling ESS; a run
    with --loo_moment_match a line per moment-matched report: the matched total and worst k-hat next to the plain ones."""
    lines = []
    for m, r in results.items():
        if "loo_observations" not in r:
            continue
        last = _last(r, ("elpd_", "p_loo", "p_waic", "loo_", "pareto_k_", "logo_", "p_logo"))
        if last["loo_observations"] is None:
            lines.append("{}: PSIS-LOO / WAIC not computed".format(m))
            continue
        lines.append("{}: elpd_loo {} +/- {}, p_loo {}; elpd_waic {} +/- {}, p_waic {}; worst Pareto k-hat {} (observation {}; "
                     "{} above {}); {} observations, {} draws of {} chains, {} left out, {} observation(s) not finite; {}".format(
                         m, _fmt(last["elpd_loo"]), _fmt(last["elpd_loo_se"]), _fmt(last["p_loo"]), _fmt(last["elpd_waic"]),
                         _fmt(last["elpd_waic_se"]), _fmt(last["p_waic"]), _fmt(last["pareto_k_max"]),
                         last["pareto_k_max_observation"], last["pareto_k_above_threshold"], _fmt(last["pareto_k_threshold"]),
                         last["loo_observations"], last["loo_draws"], last["loo_chains"], last["loo_draws_left_out"],
                         last["loo_nonfinite_observations"],
                         _secs(last.get("loo_time_sec"))))
        if last.get("loo_pred_observations") is not None:
            # the leave-one-out predictive report (--loo_predictive); next to the posterior figures of --predictive_checks
            # where the run recorded them: a posterior PIT that looks better calibrated than the LOO-PIT is the optimism
            # of checking an observation against a posterior that has seen it
            post = _last(r, "ppc_")
            beside = lambda key: " (posterior {})".format(_fmt(post[key])) if post.get(key) is not None else ""
            shown = [("LOO-PIT Kolmogorov distance", "loo_pit_ks", beside("ppc_pit_ks")),
                     ("90 % coverage", "loo_coverage_90", beside("ppc_coverage_90")), ("RMSE", "loo_rmse", ""),
                     ("R^2", "loo_r2", ""), ("Brier score", "loo_brier", ""), ("accuracy", "loo_accuracy", ""),
                     ("balanced accuracy", "loo_balanced_accuracy", "")]
            lines.append("      LOO predictive: {}; {} observations, {} left out; smallest importance-sampling ESS {} "
                         "(observation {}); {}".format(
                             ", ".join("{} {}{}".format(name, _fmt(last[key]), more) for name, key, more in shown
                                       if last.get(key) is not None) or "no figure is defined",
                             last["loo_pred_observations"], last.get("loo_pred_observations_left_out"),
                             _fmt(last.get("loo_is_ess_min")), last.get("loo_is_ess_min_observation"),
                             _secs(last.get("loo_pred_time_sec"))))
        if last.get("logo_groups") is not None:
            # leave-one-group-out (--loo_groups): the marginal form next to the conditional one -- that comparison is the report
            form = lambda pre, e: "{} +/- {}, worst Pareto k-hat {} ({}; {} above {})".format(
                _fmt(last.get(e)), _fmt(last.get(e + "_se")), _fmt(last.get(pre + "pareto_k_max")), last.get(pre + "pareto_k_max_group"),
                last.get(pre + "pareto_k_above_threshold"), _fmt(last.get("logo_pareto_k_threshold")))
            lines.append("      leave-one-group-out by {}: {} groups ({} empty, {} observations in none); marginal elpd_logo {}; "
                         "conditional elpd {}; {} group(s) not finite; {} draws; {}".format(
                             last.get("logo_part"), last["logo_groups"], last.get("logo_groups_empty"),
                             last.get("logo_observations_left_out"),
                             form("logo_", "elpd_logo") if last.get("logo_marginal") else "n/a (no closed marginal form)",
                             form("logo_conditional_", "logo_conditional_elpd"), last.get("logo_nonfinite_groups"),
                             last.get("logo_draws"), _secs(last.get("logo_time_sec"))))
        for pre, e, plain, plain_k, what in (("loo", "elpd_loo_mm", "elpd_loo", "pareto_k_max", "observation(s)"),
                                             ("logo", "elpd_logo_mm", "logo_conditional_elpd", "logo_conditional_pareto_k_max",
                                              "group(s), conditional form")):
            if last.get(pre + "_mm_observations") is None:
                continue
            # moment matching (--loo_moment_match): the matched total and worst k-hat next to the plain ones
            lines.append("      moment matching over {} {} ({} more above the threshold not attempted): k-hat fell for {}, resolved "
                         "{}, at most {} map(s); {} {} +/- {} (plain {}), worst Pareto k-hat {} (plain {}; {} still above the "
                         "threshold); full-posterior k-hat up to {}; {}".format(
                             last[pre + "_mm_observations"], what, last.get(pre + "_mm_not_attempted"), last.get(pre + "_mm_improved"),
                             last.get(pre + "_mm_resolved"), last.get(pre + "_mm_iterations_max"), e, _fmt(last.get(e)),
                             _fmt(last.get(e + "_se")), _fmt(last.get(plain)), _fmt(last.get(pre + "_mm_pareto_k_max")),
                             _fmt(last.get(plain_k)), last.get(pre + "_mm_pareto_k_above_threshold"),
                             _fmt(last.get(pre + "_mm_full_pareto_k_max")), _secs(last.get(pre + "_mm_time_sec"))))
    return lines


def report_ppc(results):
    """Build-specific: the posterior predictive checks of every sampling run that recorded them (--predictive_checks; the
    last run of each file): the predictive p-values of mean, sd, min, max and deviance, the replicated against the
    observed mean and sd, and the calibration of the PIT values.  The posterior PIT, not LOO-PIT; an extreme p-value is
    marked by the customary reading (outside [0.01, 0.99]), not by a derived threshold.  A run with
    --predictive_checks_redraw gets a second line: the mixed predictive check's figures, each with the posterior one."""
    lines = []
    for m, r in results.items():
        if "ppc_observations" not in r:
            continue
        last = _last(r, "ppc_")
        if last["ppc_observations"] is None:
            lines.append("{}: posterior predictive checks not computed".format(m))
            continue
        stats = ("mean", "sd", "min", "max", "deviance")
        extreme = [s for s in stats if last["ppc_p_" + s] is not None and not 0.01 <= last["ppc_p_" + s] <= 0.99]
        lines.append("{}: predictive p-values {}; replicated mean {} (observed {}), sd {} (observed {}); PIT Kolmogorov "
                     "distance {}, 90 % coverage {}; {} observations, {} draws of {} chains, {} left out; {}{}".format(
                         m, ", ".join("{} {}".format(s, _fmt(last["ppc_p_" + s])) for s in stats), _fmt(last["ppc_rep_mean"]),
                         _fmt(last["ppc_obs_mean"]), _fmt(last["ppc_rep_sd"]), _fmt(last["ppc_obs_sd"]), _fmt(last["ppc_pit_ks"]),
                         _fmt(last["ppc_coverage_90"]), last["ppc_observations"], last["ppc_draws"], last["ppc_chains"],
                         last["ppc_draws_left_out"], _secs(last.get("ppc_time_sec")),
                         "   <-- EXTREME: " + ", ".join(extreme) if extreme else ""))
        if last.get("ppc_mixed_draws") is not None:
            # the mixed predictive check (--predictive_checks_redraw), with the posterior figure next to each of its own: a
            # mixed p-value or PIT distance that is extreme where the posterior one is not is a misfit of the redrawn layer,
            # which a check at group effects fitted to the data cannot see
            pair = lambda key: "{} (posterior {})".format(_fmt(last.get("ppc_mixed_" + key)), _fmt(last.get("ppc_" + key)))
            mixed_extreme = [s for s in stats if last.get("ppc_mixed_p_" + s) is not None
                             and not 0.01 <= last["ppc_mixed_p_" + s] <= 0.99]
            outliers = last.get("ppc_mixed_pit_extreme_observations")
            lines.append("      mixed predictive, {} redrawn ({} elements): p-values {}; replicated sd {}; PIT Kolmogorov distance "
                         "{}, 90 % coverage {}; {} observation(s) with an extreme mixed PIT; {} draws, {} left out; {}{}".format(
                             ",".join(last.get("ppc_mixed_parts") or []), last.get("ppc_mixed_elements"),
                             ", ".join("{} {}".format(s, pair("p_" + s)) for s in stats), pair("rep_sd"), pair("pit_ks"),
                             pair("coverage_90"), "n/a" if outliers is None else len(outliers), last["ppc_mixed_draws"],
                             last.get("ppc_mixed_draws_left_out"), _secs(last.get("ppc_mixed_time_sec")),
                             "   <-- EXTREME: " + ", ".join(mixed_extreme) if mixed_extreme else ""))
        if last.get("ppc_group_draws") is not None:
            # the grouped check (--predictive_checks_groups): the ends of the groups' p-values of the mean, and the groups
            # beyond the Bonferroni threshold; the mixed figures next to them where the run has both flags
            ends = lambda pre: "{} ({}) ... {} ({})".format(_fmt(last.get(pre + "p_mean_min")), last.get(pre + "p_mean_min_group"),
                                                            _fmt(last.get(pre + "p_mean_max")), last.get(pre + "p_mean_max_group"))
            flagged = lambda pre: "n/a" if last.get(pre + "extreme_groups") is None else (", ".join(last[pre + "extreme_groups"]) or "none")
            mixed = last.get("ppc_group_mixed_draws") is not None
            lines.append("      grouped predictive by {}: {} groups ({} empty, {} observations in none); p-value of the group mean, "
                         "smallest ... largest {}{}; beyond the threshold {}: {}{}; {} draws; {}".format(
                             last.get("ppc_group_part"), last.get("ppc_groups"), last.get("ppc_groups_empty"),
                             last.get("ppc_group_observations_left_out"), ends("ppc_group_"),
                             ", mixed " + ends("ppc_group_mixed_") if mixed else "", _fmt(last.get("ppc_group_p_threshold")),
                             flagged("ppc_group_"), ", mixed " + flagged("ppc_group_mixed_") if mixed else "",
                             last["ppc_group_draws"], _secs(last.get("ppc_group_time_sec"))))
    return lines


def report_psens(results):
    """Build-specific: the power-scaling sensitivity report of every sampling run that recorded one
    (--sensitivity_diagnostics; the last run of each file): the largest prior and likelihood sensitivity with their
    elements, and the flagged elements -- prior-data conflicts, and elements with a weak likelihood or a strong prior
    (sensitivity above 0.05; Kallioinen et al. 2023).  The prior is the joint density of all latent sites; a run with
    --sensitivity_prior_parts gets a second line, for the priors of the named parts alone."""
    lines = []
    for m, r in results.items():
        if "psens_draws" not in r:
            continue
        last = _last(r, "psens_")
        if last["psens_draws"] is None:
            lines.append("{}: power-scaling sensitivity not computed".format(m))
            continue
        conflict, weak = last["psens_conflict_elements"] or [], last["psens_weak_likelihood_elements"] or []
        lines.append("{}: power-scaling sensitivity: prior max {} ({}), likelihood max {} ({}); prior-data conflict: {}; weak "
                     "likelihood / strong prior: {}; worst Pareto k-hat {} (threshold {}); {} draws of {} chains, {} left "
                     "out, {} constant element(s); {}".format(
                         m, _fmt(last["psens_prior_max"]), last["psens_prior_max_element"], _fmt(last["psens_likelihood_max"]),
                         last["psens_likelihood_max_element"], ", ".join(conflict) or "none", ", ".join(weak) or "none",
                         _fmt(last["psens_pareto_k_max"]), _fmt(last["psens_pareto_k_threshold"]), last["psens_draws"],
                         last["psens_chains"], last["psens_draws_left_out"], last["psens_elements_left_out"],
                         _secs(last.get("psens_time_sec"))))
        if last.get("psens_sites"):
            # --sensitivity_prior_parts: the same draws with the priors of the named parts power-scaled alone
            conflict = last["psens_sites_conflict_elements"] or []
            weak = last["psens_sites_weak_likelihood_elements"] or []
            lines.append("{}: power-scaling sensitivity to the priors of {} alone: prior max {} ({}); prior-data conflict: {}; "
                         "weak likelihood / strong prior: {}; worst Pareto k-hat {}; {} left out; joint gap {}; {}".format(
                             m, ", ".join(last["psens_sites"]), _fmt(last["psens_sites_prior_max"]),
                             last["psens_sites_prior_max_element"], ", ".join(conflict) or "none", ", ".join(weak) or "none",
                             _fmt(last["psens_sites_pareto_k_max"]), last["psens_sites_draws_left_out"],
                             _fmt(last["psens_sites_joint_gap_max"]), _secs(last.get("psens_sites_time_sec"))))
    return lines


def report_prior(results):
    """Build-specific: the prior predictive checks of every sampling run that recorded them (--prior_predictive_checks; the
    last run of each file), two lines each: where the observed mean and sd sit among the prior-predicted ones with the
    prior 90 % band of the replicated mean and sd next to the observed values; and the least contracted element with the
    largest |z-score|.  Nothing is marked: no threshold can be derived for a prior predictive p-value -- a weak prior is
    meant to be wider than the data."""
    lines = []
    for m, r in results.items():
        if "prior_draws" not in r:
            continue
        last = _last(r, "prior_")
        if last["prior_draws"] is None:
            lines.append("{}: prior predictive checks not computed".format(m))
            continue
        stats = ("mean", "sd", "min", "max", "deviance")
        lines.append("{}: prior predictive p-values {}; prior 90 % band of the replicated mean {} ... {} (median {}, observed "
                     "{}), of the replicated sd {} ... {} (median {}, observed {}); replicated min above {}, max below {} in "
                     "95 % of the draws; {} observations, {} prior draws, {} left out; {}".format(
                         m, ", ".join("{} {}".format(s, _fmt(last["prior_p_" + s])) for s in stats),
                         _fmt(last["prior_rep_mean_q05"]), _fmt(last["prior_rep_mean_q95"]), _fmt(last["prior_rep_mean_q50"]),
                         _fmt(last["prior_obs_mean"]), _fmt(last["prior_rep_sd_q05"]), _fmt(last["prior_rep_sd_q95"]),
                         _fmt(last["prior_rep_sd_q50"]), _fmt(last["prior_obs_sd"]), _fmt(last["prior_rep_min_q05"]),
                         _fmt(last["prior_rep_max_q95"]), last["prior_observations"], last["prior_draws"],
                         last["prior_draws_left_out"], _secs(last.get("prior_time_sec"))))
        lines.append("{}: prior to posterior: least contraction {} ({}), largest |z-score| {} ({}); {} element(s) left out "
                     "(quantile scale of the prior, moment scale of the posterior)".format(
                         m, _fmt(last["prior_contraction_min"]), last["prior_contraction_min_element"],
                         _fmt(last["prior_z_score_max_abs"]), last["prior_z_score_max_element"],
                         last["prior_elements_left_out"]))
    return lines


def report_vi(results):
    """Build-specific: the fit check of every VI result file that holds one (--vi_diagnostics): the Pareto k-hat of the
    importance ratios p / q against its threshold, the ELBO of the final parameters next to the optimiser's own figure, the
    evidence and KL estimates, the largest ELBO gradients and the spread of the importance-corrected sd.  k-hat is the only
    figure with a threshold; above it the importance-corrected figures are marked unreliable."""
    lines = []
    for m, r in results.items():
        if "vi_check_draws" not in r:
            continue
        k, cap = r["vi_pareto_k"], r["vi_pareto_k_threshold"]
        far = k is None or cap is None or k > cap
        lines.append("{}: Pareto k-hat {} (threshold {}); ELBO of the final parameters {} +/- {} (optimiser: {} +/- {}); log "
                     "evidence {} +/- {}, KL(q || p) {} +/- {}; largest ELBO gradient along loc {} +/- {} ({}), along log scale "
                     "{} +/- {} ({}); largest score gap {} ({}), loc shift {} sd ({}); sd ratio {} ({}) ... {} ({}); {} draws, "
                     "{} left out; {}{}".format(
                         m, _fmt(k), _fmt(cap), _fmt(r["vi_elbo_final"], "{:.4f}"), _fmt(r["vi_elbo_final_se"]),
                         _fmt(r.get("elbo"), "{:.4f}"), _fmt(r.get("estimated_elbo_std")), _fmt(r["vi_log_evidence"], "{:.4f}"),
                         _fmt(r["vi_log_evidence_se"]), _fmt(r["vi_kl_estimate"]), _fmt(r["vi_kl_estimate_se"]),
                         _fmt(r["vi_elbo_grad_loc_max"]), _fmt(r["vi_elbo_grad_loc_max_se"]), r["vi_elbo_grad_loc_max_element"],
                         _fmt(r["vi_elbo_grad_scale_max"]), _fmt(r["vi_elbo_grad_scale_max_se"]),
                         r["vi_elbo_grad_scale_max_element"], _fmt(r["vi_score_gap_max"]), r["vi_score_gap_max_element"],
                         _fmt(r["vi_loc_shift_max"]), r["vi_loc_shift_max_element"], _fmt(r["vi_sd_ratio_min"]),
                         r["vi_sd_ratio_min_element"], _fmt(r["vi_sd_ratio_max"]), r["vi_sd_ratio_max_element"],
                         r["vi_check_draws"], r["vi_check_draws_left_out"], _secs(r.get("vi_check_time_sec")),
                         "   <-- q IS FAR FROM THE POSTERIOR: the importance-corrected figures are unreliable" if far else ""))
    return lines


def report_loo_compare(path_a, path_b):
    """Build-specific: the paired difference in elpd_loo of two models fitted to the same observations, from their
    <method>_loo.npz files (diagnostics.loo_compare): positive favours the first.  Refused unless y agrees."""
    from . import diagnostics
    with np.load(path_a) as a, np.load(path_b) as b:
        diff, se = diagnostics.loo_compare(a, b)
        return ["elpd_loo({}) - elpd_loo({}) = {:.4g} +/- {:.4g} over {} observations".format(
            str(a["model"]), str(b["model"]), diff, se, int(np.asarray(a["y"]).size))]


def report_logo_compare(path_a, path_b):
    """Build-specific: the paired difference in leave-one-group-out elpd of two models fitted to the same observations
    and grouped the same way, from their <method>_logo.npz files (diagnostics.loo_compare over the non-empty groups, so the
    se is over groups): positive favours the first.  The marginal form where both files have it, the conditional one
    otherwise.  Refused unless y, group_of and part agree."""
    from . import diagnostics
    with np.load(path_a) as a, np.load(path_b) as b:
        for name in ("part", "y", "group_of"):
            if not np.array_equal(np.asarray(a[name]), np.asarray(b[name])):
                raise ValueError("logo_compare: the two files differ in %s -- the groups are not the same, and the pairing is "
                                 "what the se rests on" % name)
        filled = np.asarray(a["n_obs"]) > 0
        marginal = all(np.any(np.isfinite(np.asarray(z["elpd_logo_g"], np.float64)[filled])) for z in (a, b))
        name = "elpd_logo_g" if marginal else "conditional_elpd_logo_g"
        pair = [{"elpd_loo_i": np.asarray(z[name], np.float64)[filled], "y": np.flatnonzero(filled)} for z in (a, b)]
        diff, se = diagnostics.loo_compare(*pair)
        return ["elpd_logo({}) - elpd_logo({}) = {:.4g} +/- {:.4g} over {} groups of {} ({})".format(
            str(a["model"]), str(b["model"]), diff, se, int(filled.sum()), str(a["part"]), "marginal" if marginal else "conditional")]


def report_sbc(results):
    """Build-specific: simulation-based calibration of every method that recorded it (--inference=SBC writes
    <method>_sbc.json next to the method's own file): the worst quantity with its p-value and the two shape figures, then
    the quantities whose ranks are not uniform (p below 1 % over the quantities, Bonferroni: a convention)."""
    lines = []
    for m, r in results.items():
        if "sbc_replications" not in r:
            continue
        name = m[:-len("_sbc")] if m.endswith("_sbc") else m
        lines.append("{}: simulation-based calibration: worst {} with p = {} (Kolmogorov distance {} of {}; threshold {}); "
                     "largest |rank mean z| {} ({}); rank variance ratio {} ({}) ... {} ({}); posterior z-score mean within "
                     "{}, sd {} ... {}; {} replicates, {} left out, {} chains x {} step(s) = {} draws, {} leapfrog steps; "
                     "acceptance {}, median smallest ESS {}; fit {}, mcmc {}, fold {}, all {}".format(
                         name, r["sbc_p_min_element"], _fmt(r["sbc_p_min"]), _fmt(r["sbc_ks_max"]), r["sbc_ks_max_element"],
                         _fmt(r["sbc_p_threshold"]), _fmt(r["sbc_rank_mean_z_max_abs"]), r["sbc_rank_mean_z_max_abs_element"],
                         _fmt(r["sbc_rank_var_ratio_min"]), r["sbc_rank_var_ratio_min_element"],
                         _fmt(r["sbc_rank_var_ratio_max"]), r["sbc_rank_var_ratio_max_element"],
                         _fmt(r["sbc_post_z_mean_max_abs"]), _fmt(r["sbc_post_z_sd_min"]), _fmt(r["sbc_post_z_sd_max"]),
                         r["sbc_replications"], r["sbc_replications_left_out"], r["sbc_chains"], r["sbc_steps"], r["sbc_draws"],
                         r["sbc_leapfrog_steps"], _fmt(r["sbc_accept_rate_mean"]), _fmt(r["sbc_ess_min_median"]),
                         _secs(r["sbc_fit_time_sec"]), _secs(r["sbc_mcmc_time_sec"]), _secs(r["sbc_fold_time_sec"]),
                         _secs(r["sbc_time_sec"])))
        lines.append("{}: ranks not uniform: {}".format(name, ", ".join(r["sbc_miscalibrated_elements"]) or "none"))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    for f in ("elbos", "ess", "reparams", "normalize_times", "rhat", "energy", "trajectory", "geometry", "loo", "ppc", "vi", "psens", "prior",
              "sbc"):
        ap.add_argument("--" + f, action="store_true")
    ap.add_argument("--loo_compare", default="", help="A_loo.npz,B_loo.npz: the paired elpd_loo difference of two models")
    ap.add_argument("--logo_compare", default="", help="A_logo.npz,B_logo.npz: the paired leave-one-group-out elpd difference of two models")
    ap.add_argument("--model", default="all")
    ap.add_argument("--results_dir", default="")
    args = ap.parse_args(argv)
    if args.logo_compare:
        paths = [p for p in args.logo_compare.split(",") if p]
        if len(paths) != 2:
            ap.error("--logo_compare takes two files: A_logo.npz,B_logo.npz")
        print("\n".join(report_logo_compare(*paths)) + "\n")
        return
    if args.loo_compare:
        paths = [p for p in args.loo_compare.split(",") if p]
        if len(paths) != 2:
            ap.error("--loo_compare takes two files: A_loo.npz,B_loo.npz")
        print("\n".join(report_loo_compare(*paths)) + "\n")
        return
    root = args.results_dir or "."
    names = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d))) if args.model == "all" \
        else [args.model]
    for name in names:
        results = load(root, name)
        if not results:
            continue
        # <method>_sbc.json is a report of its own, not a method's result file: only --sbc reads it
        calibration = {m: r for m, r in results.items() if m.endswith("_sbc") and "sbc_replications" in r}
        results = {m: r for m, r in results.items() if m not in calibration}
        print(" ******  {}  ****** ".format(name))
        for flag, lines in (("elbos", lambda: report_elbos(results)), ("reparams", lambda: report_reparams(results)),
                            ("ess", lambda: report_ess(results, args.normalize_times)),
                            ("rhat", lambda: report_rhat(results, root, name)),
                            ("energy", lambda: report_energy(results, root, name)),
                            ("trajectory", lambda: report_trajectory(results, root, name)),
                            ("geometry", lambda: report_geometry(results, root, name)), ("loo", lambda: report_loo(results)),
                            ("ppc", lambda: report_ppc(results)), ("vi", lambda: report_vi(results)),
                            ("psens", lambda: report_psens(results)), ("prior", lambda: report_prior(results)),
                            ("sbc", lambda: report_sbc(calibration))):
            if getattr(args, flag):
                print("\n".join(lines()) + "\n")


if __name__ == "__main__":
    main()
