"""Simulation-based calibration (--inference=SBC; Talts, Betancourt, Simpson, Vehtari, Gelman 2018): does the flow --
the VI fit, the initial population, HMC with its adaptation, the centred trace -- return the posterior of the model it was
given?  A self-consistency check that needs no reference.  For each of N replicates: a truth drawn from the prior
(diagnostics.site_prior_draws over ModelSpec.site_table), a data set drawn from the likelihood at that truth
(diagnostics.predictive_check over ModelSpec.observation_table), the whole flow on that data, and the rank of the truth
among the posterior draws.  The ranks are uniform if and only if the sampler samples the posterior of that model.  The two
generating kernels are restatements of the model that share nothing with the sampling kernels, which is what makes the
check mean something.

Build-specific: the reference never refits on simulated data.  main.py holds the dispatch and the call of check_sbc only.
"""
import os
import time
from collections import OrderedDict

import numpy as np

from . import diagnostics, inference, models, util
from . import engine as _engine
from .report_common import (_finite_or_none, _fmt, _nan_max, _write_json_atomic, derived_seed, element_names, joint_loglik,
                            loo_tile_rows, next_seed, probe_steps, replicate_tiles)

SBC_SEED = 0x53424331                # the report's own seed constant, as PRIOR_SEED is the prior predictive checks'
SBC_REPLICATIONS_MIN, SBC_REPLICATIONS_MAX = 8, 16384
SBC_P_LEVEL = 0.01                   # the customary 1 %, split over the quantities (Bonferroni): a convention, not a derived threshold
SBC_SHOWN = 8                        # quantities the warning names
SBC_MEMORY_SHARE = 0.6               # of the free device memory the draws buffer and the replicated data may take
LOG_LIKELIHOOD = "log_likelihood"    # the name of the data-dependent test quantity, column D
SBC_KEYS = ("sbc_replications", "sbc_replications_left_out", "sbc_chains", "sbc_steps", "sbc_draws", "sbc_leapfrog_steps",
            "sbc_quantities", "sbc_ks_max", "sbc_ks_max_element", "sbc_p_min", "sbc_p_min_element", "sbc_p_threshold",
            "sbc_miscalibrated_elements", "sbc_rank_mean_z_max_abs", "sbc_rank_mean_z_max_abs_element",
            "sbc_rank_var_ratio_min", "sbc_rank_var_ratio_min_element", "sbc_rank_var_ratio_max",
            "sbc_rank_var_ratio_max_element", "sbc_post_z_mean_max_abs", "sbc_post_z_sd_min", "sbc_post_z_sd_max",
            "sbc_accept_rate_mean", "sbc_ess_min_median", "sbc_fit_time_sec", "sbc_mcmc_time_sec", "sbc_fold_time_sec",
            "sbc_time_sec")
SBC_SUFFIX = "_sbc"                  # <base>_sbc.json, <base>_sbc.npz


def recorded_steps(flags):
    """The recorded steps of one refit: --num_samples, counted in gradient evaluations under --count_in_leapfrog_steps (as
    main._settle_leapfrog_count counts them)."""
    S = int(flags.num_samples)
    if getattr(flags, "count_in_leapfrog_steps", False) and flags.num_leapfrog_steps:
        S = int(S / float(flags.num_leapfrog_steps))
    return S


def check_sbc(flags):
    """--inference=SBC against the job, before anything is drawn or launched: raises ValueError, with a message that names
    the flag, for a --method other than CP or NCP, for neals_funnel, for a missing --num_leapfrog_steps, for
    --sbc_replications outside 8 ... 16384, for --sbc_steps outside 1 ... the recorded steps of the run, and for a job of
    more than one process.  Any other --inference passes."""
    if getattr(flags, "inference", None) != "SBC":
        return
    if flags.method not in ("CP", "NCP"):
        raise ValueError("--inference=SBC: --method must be CP or NCP, not {} (cVIP, dVIP and i need a stored fit per data "
                         "set -- a learned parameterisation, tuned leapfrog counts -- and are not covered)".format(flags.method))
    if flags.model == "neals_funnel":
        raise ValueError("--inference=SBC: --model=neals_funnel has no observations, so there is no data to simulate and refit")
    if not flags.num_leapfrog_steps or int(flags.num_leapfrog_steps) < 1:
        raise ValueError("--inference=SBC: --num_leapfrog_steps is required (there are no tuning runs per replicate)")
    n = int(flags.sbc_replications)
    if not SBC_REPLICATIONS_MIN <= n <= SBC_REPLICATIONS_MAX:
        raise ValueError("--sbc_replications must lie in %d ... %d, not %d" % (SBC_REPLICATIONS_MIN, SBC_REPLICATIONS_MAX, n))
    S = recorded_steps(flags)
    if not 1 <= int(flags.sbc_steps) <= S:
        raise ValueError("--sbc_steps must lie in 1 ... %d (the recorded steps of the run, --num_samples), not %d"
                         % (S, int(flags.sbc_steps)))
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    if ws > 1:
        raise ValueError("--inference=SBC runs in one process: WORLD_SIZE=%d (no sharded job)" % ws)


def sbc_steps_of(S, k):
    """The recorded steps whose draws are ranked: k evenly spaced of S, the last among them (report_common.loo_steps' rule:
    counted from the end, a single step is the last)."""
    return sorted(int(S) - 1 - s for s in probe_steps(int(S), int(k)))


def _direction(mean_z, var_z, var_ratio):
    """Which way a miscalibrated quantity is off, from the larger of its two shape figures."""
    if np.isfinite(mean_z) and (not np.isfinite(var_z) or abs(mean_z) >= abs(var_z)):
        return "shifted {}".format("above the truth" if mean_z < 0 else "below the truth")
    return "too narrow" if var_ratio > 1.0 else "too wide"


def sbc_keys(summary):
    """The JSON keys that come from a diagnostics.SbcSummary (the run's own -- chains, steps, leapfrog steps, the
    per-replicate figures and the clocks -- are run_sbc's); pure Python.  Of every per-quantity family the entry that
    stands out, with the quantity's name.  sbc_p_threshold = SBC_P_LEVEL / Q, Bonferroni at the customary 1 %: a
    convention.  sbc_miscalibrated_elements: the quantities with ks_p below it, smallest p first."""
    s = summary
    Q = len(s.names)
    keys = OrderedDict([("sbc_replications", int(s.replications + s.left_out)), ("sbc_replications_left_out", int(s.left_out)),
                        ("sbc_draws", int(s.draws)), ("sbc_quantities", int(Q))])

    def stands_out(key, values, rank):
        _, at = _nan_max(rank)
        keys[key] = _finite_or_none(values[at]) if at >= 0 else None
        keys[key + "_element"] = s.names[at] if at >= 0 else None
    stands_out("sbc_ks_max", s.ks, s.ks)
    stands_out("sbc_p_min", s.ks_p, -np.asarray(s.ks_p))
    keys["sbc_p_threshold"] = SBC_P_LEVEL / Q
    p = np.asarray(s.ks_p, np.float64)
    below = [int(q) for q in np.argsort(np.where(np.isfinite(p), p, np.inf), kind="stable") if np.isfinite(p[q])
             and p[q] < keys["sbc_p_threshold"]]
    keys["sbc_miscalibrated_elements"] = [s.names[q] for q in below]
    stands_out("sbc_rank_mean_z_max_abs", np.abs(s.rank_mean_z), np.abs(s.rank_mean_z))
    stands_out("sbc_rank_var_ratio_min", s.rank_var_ratio, -np.asarray(s.rank_var_ratio))
    stands_out("sbc_rank_var_ratio_max", s.rank_var_ratio, s.rank_var_ratio)
    keys["sbc_post_z_mean_max_abs"] = _finite_or_none(_nan_max(np.abs(s.post_z_mean))[0])
    keys["sbc_post_z_sd_min"] = _finite_or_none(-_nan_max(-np.asarray(s.post_z_sd))[0])
    keys["sbc_post_z_sd_max"] = _finite_or_none(_nan_max(s.post_z_sd)[0])
    return keys


def sbc_line(keys, summary):
    """The one printed line: the worst quantity, its p and its two shape figures."""
    name = keys["sbc_p_min_element"]
    at = summary.names.index(name) if name is not None else -1
    fig = lambda v: _fmt(float(v[at]) if at >= 0 and np.isfinite(v[at]) else None)
    return ("    simulation-based calibration over {} replicates ({} left out), {} draws each, {} quantities: worst {} with "
            "p = {} (Kolmogorov distance {}; Bonferroni threshold {}), rank mean z {}, rank variance ratio {}; posterior "
            "z-score mean within {}, sd in {} ... {}".format(
                keys["sbc_replications"], keys["sbc_replications_left_out"], keys["sbc_draws"], keys["sbc_quantities"], name,
                _fmt(keys["sbc_p_min"]), fig(summary.ks), _fmt(keys["sbc_p_threshold"]), fig(summary.rank_mean_z),
                fig(summary.rank_var_ratio), _fmt(keys["sbc_post_z_mean_max_abs"]), _fmt(keys["sbc_post_z_sd_min"]),
                _fmt(keys["sbc_post_z_sd_max"])))


def sbc_warning(keys, summary):
    """The one warning, or None: up to SBC_SHOWN quantities with p below the threshold, and which way each is off."""
    names = keys["sbc_miscalibrated_elements"]
    if not names:
        return None
    shown = []
    for name in names[:SBC_SHOWN]:
        q = summary.names.index(name)
        shown.append("{} (p = {}, {})".format(name, _fmt(float(summary.ks_p[q])), _direction(
            summary.rank_mean_z[q], summary.rank_var_z[q], summary.rank_var_ratio[q])))
    more = len(names) - len(shown)
    return ("    WARNING: the ranks of {} quantit{} are not uniform (p below {}, 1 % over the quantities: a convention): {}{}.  "
            "The flow does not return the posterior of this model for them -- the sampler, the fit it starts from, or the "
            "tables the data were simulated from.".format(
                len(names), "y" if len(names) == 1 else "ies", _fmt(keys["sbc_p_threshold"]), "; ".join(shown),
                " and {} more".format(more) if more > 0 else ""))


def _replicate_flags(flags, r, chains):
    """The flags of replicate r's refit: its own seed, the run's chains, every diagnostic off."""
    f = flags.copy()
    f.seed = int(flags.seed) + 1 + int(r)
    f.num_chains = int(chains)
    f.num_samples = recorded_steps(flags)
    if getattr(flags, "count_in_leapfrog_steps", False):
        for name in ("num_burnin_steps", "num_adaptation_steps"):
            setattr(f, name, int(getattr(flags, name) / float(flags.num_leapfrog_steps)))
        f.count_in_leapfrog_steps = False
    f.num_chains_to_save = 0
    f.superchain_size = 0
    f.trace_chunk_rows = None
    for name in ("convergence_diagnostics", "rank_normalized_rhat", "bulk_tail_ess", "energy_diagnostics", "geometry_diagnostics",
                 "predictive_diagnostics", "predictive_checks", "loo_predictive", "sensitivity_diagnostics",
                 "prior_predictive_checks", "vi_diagnostics"):
        setattr(f, name, False)
    f.trajectory_profile = 0
    return f


def _joint_loglik(rows, table, y, ll_buffer, tile_rows):
    """joint_loglik of the data `y` [n] at the rows [R, D]: the uploaded table with only y replaced, one reused `ll_buffer`."""
    return joint_loglik(rows[None], table._replace(y=y, y_host=None), ll_buffer, tile_rows)


def run_sbc(model_config, results_dir, file_path, flags, out=None):
    """--inference=SBC.  N = --sbc_replications truths are drawn from the uploaded site table under a seed derived from
    --seed and SBC_SEED, one replicated data set each under the next seed (main._prior_report says why not the same), in
    replicate_tiles' tiles of observations.  A replicate whose draw is undrawn or masked or whose data hold a non-finite
    value is left out before any refit, and counted.  Every other replicate r is refitted the way run_vi and run_hmc fit:
    ModelSpec.with_observations -> models.model_config_for -> main.create_target_graph -> inference.find_best_learning_rate
    -> util.variational_inits_from_params -> inference.hmc with seed --seed + 1 + r and chain_offset r M, so that no two
    replicates share a random stream; --sbc_steps evenly spaced recorded steps of its centred trace, the last among them,
    go into its block of the draws buffer [N, L, D + 1], L = steps * M.  Column D is the joint log-likelihood of the
    replicate's own data (Modrak et al. 2023: ranks of parameters alone miss whole classes of errors) at its draws and at
    its truth, rounded to float32; a masked row leaves the replicate out.  A replicate none of whose learning rates gives
    a finite ELBO is left out and said so; a relay error of its run is not swallowed.  Then one diagnostics.sbc_fold over
    the whole buffer and diagnostics.sbc_summary.  Writes <base>_sbc.json (SBC_KEYS) and <base>_sbc.npz next to the
    method's files; the fit file of the real data is neither read nor written.  With `out`, out["sbc"] holds the device
    buffer ("draws"), the truth tensor ("truth"), the replicated data [observations, N] ("data") and the summary."""
    import torch
    from .main import create_target_graph        # the refit is what the command line builds (main imports this module)
    base = file_path[:-5] + SBC_SUFFIX
    if os.path.exists(base + ".json"):
        util.print_("Already ran experiment {}-{} on model {} with dataset {}. Skipping".format(
            flags.inference, flags.method, flags.model, flags.dataset))
        return None
    clock = time.time()
    spec = model_config.model
    D = int(spec.D)
    if D > diagnostics.LOGLIK_MAX_D:
        raise ValueError("--inference=SBC: model {} has {} elements, more than the {} the table kernels take".format(
            flags.model, D, diagnostics.LOGLIK_MAX_D))
    N, M, S = int(flags.sbc_replications), int(flags.num_chains), recorded_steps(flags)
    steps = sbc_steps_of(S, int(flags.sbc_steps))
    L, Q = len(steps) * M, D + 1
    host_table = spec.observation_table()
    n_obs = int(np.asarray(host_table.y).size)
    dev = torch.device(flags.device)
    need = 4 * N * L * Q + 4 * n_obs * N
    free, _ = torch.cuda.mem_get_info(dev)
    if need > SBC_MEMORY_SHARE * free:
        raise MemoryError("--inference=SBC: the draws buffer [N={}, L={}, D + 1={}] and the replicated data need {:.1f} GB of "
                          "device memory ({:.1f} GB free); lower --sbc_replications, --sbc_steps or --num_chains".format(
                              N, L, Q, need / 1e9, free / 1e9))
    util.print_("simulation-based calibration of {}-{} on model {} with dataset {}: {} replicates of {} chains, {} leapfrog "
                "steps, {} recorded step(s) ranked".format(flags.inference, flags.method, flags.model, flags.dataset, N, M,
                                                           flags.num_leapfrog_steps, len(steps)))
    # ---- 1. truths and data ----
    seed = derived_seed(flags.seed, SBC_SEED)
    site = diagnostics.upload_site_table(spec.site_table(), D, dev)
    x, undrawn = diagnostics.site_prior_draws(site, N, seed=seed)
    table = diagnostics.upload_table(host_table, D, dev)
    y_all = torch.empty(n_obs, N, dtype=torch.float32, device=dev)
    _, _, mask = replicate_tiles(x[None], table, next_seed(seed), y_rep_out=y_all)   # (the statistics: not wanted here)
    skipped = ((mask != 0) | (undrawn != 0) | ~torch.isfinite(y_all).all(dim=0)).cpu().numpy()
    y_host = y_all.t().contiguous().cpu().numpy()                                   # [N, n_obs]
    buffer = torch.zeros(N, L, Q, dtype=torch.float32, device=dev)
    truth = torch.full((N, Q), float("nan"), dtype=torch.float32, device=dev)       # (NaN: left out by the fold itself)
    # ---- 2., 3. the refits and the data-dependent quantity ----
    nan = np.full(N, np.nan)
    accept_rate, ess_min, elbo = nan.copy(), nan.copy(), nan.copy()
    fit_time = mcmc_time = 0.0
    step_index = torch.as_tensor(steps, device=dev)
    ll_rows = loo_tile_rows(n_obs, L + 1)
    ll_buffer = torch.empty(ll_rows, L + 1, dtype=torch.float32, device=dev)
    for r in range(N):
        if skipped[r]:
            continue
        spec_r = spec.with_observations(y_host[r])
        config_r = models.model_config_for(spec_r)
        flags_r = _replicate_flags(flags, r, M)
        try:
            target, _, elbo_graph, vp, lp, reparam = create_target_graph(config_r, results_dir, flags_r)
            tick = time.time()
            try:
                fit = inference.find_best_learning_rate(elbo_graph, vp, learnable_parameters_prior=None, learnable_parameters=lp,
                                                        flags=flags_r)
            except RuntimeError as e:
                if "no learning rate gave a finite ELBO" not in str(e):
                    raise
                util.print_("    replicate {}: no learning rate gave a finite ELBO on its simulated data: left out".format(r))
                fit_time += time.time() - tick
                continue
            fit_time += time.time() - tick
            elbo[r] = float(fit[0])
            initial = list(util.variational_inits_from_params(fit[4], param_names=list(spec.part_names), num_inits=M,
                                                              seed=flags_r.seed).values())
            tick = time.time()
            _, kernel_results, _, ess = inference.hmc(target, config_r, fit[3], initial_states=initial, reparam=reparam,
                                                      flags=flags_r, chain_offset=r * M)
            mcmc_time += time.time() - tick
            trace = kernel_results.trace
            if trace is None or tuple(trace.shape) != (S, M, D):
                raise MemoryError("--inference=SBC: the trace [S={}, C={}, D={}] of a replicate does not fit the device next to "
                                  "the draws buffer; lower --num_samples or --num_chains".format(S, M, D))
            block = buffer[r].view(len(steps), M, Q)
            block[:, :, :D] = trace[step_index]
            truth[r, :D] = x[r]
            accept_rate[r] = float(np.sum(kernel_results.inner_results.is_accepted)) / float(S * M)
            per_chain = np.minimum.reduce([np.nan_to_num(np.asarray(e)).reshape(M, -1).min(axis=1) for e in ess])
            ess_min[r] = float(per_chain.min())
            del trace, kernel_results
            state = torch.cat([buffer[r, :, :D], x[r:r + 1]], dim=0)                # [L + 1, D]: the draws, then the truth
            total, ll_mask = _joint_loglik(state, table, y_all[:, r].contiguous(), ll_buffer, ll_rows)
            if bool((ll_mask != 0).any().item()):
                truth[r, D] = float("nan")
                continue
            column = total.to(torch.float32)
            buffer[r, :, D] = column[:L]
            truth[r, D] = column[L]
        finally:
            _engine.release(spec_r)
    del ll_buffer
    # ---- 4. the fold ----
    torch.cuda.synchronize(dev)
    tick = time.time()
    counts, sums, left_out, _ = diagnostics.sbc_fold(buffer, truth)
    left_host = left_out.cpu().numpy()
    summary = diagnostics.sbc_summary(counts, sums, L, left_host, element_names(spec) + [LOG_LIKELIHOOD])
    fold_time = time.time() - tick
    # ---- 5. outputs ----
    keys = sbc_keys(summary)
    kept = left_host == 0
    kept_only = lambda fold, v: _finite_or_none(fold(v[kept & np.isfinite(v)])) if np.any(kept & np.isfinite(v)) else None
    keys.update([("sbc_chains", M), ("sbc_steps", len(steps)), ("sbc_leapfrog_steps", int(flags.num_leapfrog_steps)),
                 ("sbc_accept_rate_mean", kept_only(np.mean, accept_rate)), ("sbc_ess_min_median", kept_only(np.median, ess_min)),
                 ("sbc_fit_time_sec", fit_time), ("sbc_mcmc_time_sec", mcmc_time), ("sbc_fold_time_sec", fold_time)])
    util.print_(sbc_line(keys, summary))
    warning = sbc_warning(keys, summary)
    if warning:
        util.print_(warning)
    counts_host = counts.cpu().numpy()
    truth_host = truth.cpu().numpy()
    arrays = OrderedDict([
        ("elements", np.asarray(summary.names)), ("truth", truth_host), ("rank_less", counts_host[:, :, 0]),
        ("rank_equal", counts_host[:, :, 1]), ("u", summary.u), ("post_mean", truth_host.astype(np.float64) + summary.post_bias),
        ("post_sd", summary.post_sd), ("left_out", left_host), ("ks", summary.ks), ("ks_p", summary.ks_p),
        ("rank_mean_z", summary.rank_mean_z), ("rank_var_ratio", summary.rank_var_ratio), ("rank_var_z", summary.rank_var_z),
        ("accept_rate", accept_rate), ("ess_min", ess_min), ("elbo", elbo)])
    save_sbc(base, arrays)
    keys["sbc_time_sec"] = time.time() - clock
    record = OrderedDict((key, keys[key]) for key in SBC_KEYS)
    _write_json_atomic(base + ".json", record)
    if out is not None:
        out["sbc"] = {"draws": buffer, "truth": truth, "data": y_all, "summary": summary}
    return record


def save_sbc(file_path_base, arrays):
    """`<base>.npz` next to `<base>.json`, <base> = <method>_sbc (build-specific, --inference=SBC): `elements` [Q], the
    elements' names in trace order, then log_likelihood; `truth` [N, Q] float32 (NaN rows: left out before the refit);
    `rank_less`, `rank_equal` [N, Q] int32; `u`, `post_mean`, `post_sd` [N, Q] float64 (NaN rows for a replicate left out);
    `left_out` [N]; `ks`, `ks_p`, `rank_mean_z`, `rank_var_ratio`, `rank_var_z` [Q]; per replicate `accept_rate`,
    `ess_min` (the smallest per-chain ESS) and `elbo` [N] (NaN where there was no refit)."""
    np.savez(file_path_base + ".npz", **arrays)

