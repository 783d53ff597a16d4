"""Command line of the reference (main.py:37-589) on the HIP engine:

    python -m autoreparam_amd.main --model=radon --dataset=MN --inference=VI --method=CP
    python -m autoreparam_amd.main --model=radon --dataset=MN --inference=HMCtuning --method=CP --num_leapfrog_steps=4
    python -m autoreparam_amd.main --model=radon --dataset=MN --inference=HMC --method=CP

Same flags, result directory, file names, JSON keys and run sequencing (VI before
HMC, cVIP before dVIP, tuning runs before an untuned HMC).  Two defects of the
reference's interleaved entry point are not reproduced: the
NameError at main.py:515 and the CP.json / CP_tied.json file-name mismatch (both
spellings are looked up).
"""
import collections
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np

from . import _lib, diagnostics, graphs, inference, models, parallel, report_common, util
from . import engine as _engine
from . import sbc as _sbc
from .flags import FLAGS, check_vi_check_draws
from .report_common import (LOO_CHUNK_BYTES, _above, _finite_or_none, _fmt, _nan_max, _null_keys, _shown, _write_json_atomic,
                            data_tail, derived_seed, element_names, grouped_head, joint_loglik, loo_steps, next_seed,
                            ppc_tile_rows, probe_steps, replicate_groups, replicate_tiles, select_draws)


def _vip_suffix(flags):
    return "{}{}{}{}".format(flags.learnable_parameterisation_type,
                             "_tied" if flags.tied_pparams else "",
                             "_reparam_variational" if flags.reparameterise_variational else "",
                             "_discrete_prior" if flags.discrete_prior else "")


TargetBundle = collections.namedtuple("TargetBundle", ["target", "model", "elbo", "variational_parameters",
                                                         "learnable_parameters", "reparam"])


def _stored_cvip_reparam(results_dir, flags, required_for):
    """`learned_reparam` of the cVIP fit this results directory holds (the dVIP / cVIP-HMC steps start from it)."""
    path = os.path.join(results_dir, "cVIP_{}.json".format(_vip_suffix(flags)))
    if not os.path.exists(path):
        raise Exception("Run cVIP first to find reparameterisation" if required_for == "dVIP" else
                        "no cVIP fit at {}: run --inference=VI --method=cVIP first".format(path))
    with open(path, "r") as f:
        return json.load(f)["learned_reparam"]


def _bundle_fixed(kind):
    """CP / NCP: a fixed parameterisation."""
    def build(model_config, results_dir, flags):
        make = graphs.make_cp_graph if kind == "CP" else graphs.make_ncp_graph
        return TargetBundle(*make(model_config, flags=flags), reparam=kind)
    return build


def _bundle_interleaved(model_config, results_dir, flags):
    """`i`: the pair (centred, non-centred) for the interleaved sampler; there is nothing to fit."""
    if flags.inference == "VI":
        raise Exception("Cannot run interleaved VI. Use `i` method with HMC only.")
    cp = graphs.make_cp_graph(model_config, flags=flags)
    ncp = graphs.make_ncp_graph(model_config, flags=flags)
    return TargetBundle((cp[0], ncp[0]), (cp[1], ncp[1]), None, None, None, None)


def _bundle_cvip(model_config, results_dir, flags):
    """cVIP: the learnable parameterisation while fitting; the fitted (continuous) one when sampling."""
    ptype = flags.learnable_parameterisation_type
    if flags.inference == "VI":
        return TargetBundle(*graphs.make_cvip_graph(model_config, parameterisation_type=ptype,
                                                    tied_pparams=flags.tied_pparams, flags=flags), reparam=None)
    fitted = _stored_cvip_reparam(results_dir, flags, "cVIP")
    return TargetBundle(*graphs.make_dvip_graph(model_config, fitted, parameterisation_type=ptype, flags=flags),
                        reparam=fitted)


def _bundle_dvip(model_config, results_dir, flags):
    """dVIP: the cVIP fit rounded to {0, 1} element by element (reference main.py:170-172)."""
    fitted = _stored_cvip_reparam(results_dir, flags, "dVIP")
    rounded = collections.OrderedDict((name, (np.array(value) >= 0.5).astype(np.float32)) for name, value in fitted.items())
    util.print_("dVIP parameterisation (cVIP fit thresholded at 0.5): {}".format(rounded))
    return TargetBundle(*graphs.make_dvip_graph(model_config, rounded,
                                                parameterisation_type=flags.learnable_parameterisation_type, flags=flags),
                        reparam=rounded)


_BUNDLES = {"CP": _bundle_fixed("CP"), "NCP": _bundle_fixed("NCP"), "i": _bundle_interleaved, "cVIP": _bundle_cvip,
            "dVIP": _bundle_dvip}


def create_target_graph(model_config, results_dir, flags=FLAGS):
    """The target (log joint under the method's parameterisation), ELBO and variational parameters of a run -- the
    reference's create_target_graph (main.py:117-187), same 6-tuple; one builder per --method."""
    try:
        build = _BUNDLES[flags.method]
    except KeyError:
        raise Exception("unknown method {}".format(flags.method))
    return tuple(build(model_config, results_dir, flags))


def _clean_dict(d):
    if d is None:
        return None
    return OrderedDict([(k, np.asarray(d[k]).item() if np.ndim(d[k]) == 0 else np.asarray(d[k]).tolist())
                        for k in d.keys()])


VI_CHECK_SEED = 0x56494348           # the check's own seed constant (the probes and the predictive checks have theirs)
VI_CHECK_FAMILIES = ("elbo_grad_loc", "elbo_grad_loc_se", "elbo_grad_scale", "elbo_grad_scale_se", "score_gap", "loc_shift",
                     "sd_ratio", "is_mean", "is_sd")
VI_CHECK_KEYS = ("vi_check_draws", "vi_check_draws_left_out", "vi_pareto_k", "vi_pareto_k_threshold", "vi_tail_length",
                 "vi_is_ess", "vi_elbo_final", "vi_elbo_final_se", "vi_log_evidence", "vi_log_evidence_se", "vi_kl_estimate",
                 "vi_kl_estimate_se", "vi_elbo_grad_loc_max", "vi_elbo_grad_loc_max_se", "vi_elbo_grad_loc_max_element",
                 "vi_elbo_grad_scale_max", "vi_elbo_grad_scale_max_se", "vi_elbo_grad_scale_max_element", "vi_score_gap_max",
                 "vi_score_gap_max_element", "vi_loc_shift_max", "vi_loc_shift_max_element", "vi_sd_ratio_min",
                 "vi_sd_ratio_min_element", "vi_sd_ratio_max", "vi_sd_ratio_max_element", "vi_check_time_sec")


def check_vi_diagnostics(flags):
    """--vi_diagnostics against the job, before anything runs: raises ValueError for --vi_check_draws outside its range."""
    if getattr(flags, "vi_diagnostics", False):
        check_vi_check_draws(getattr(flags, "vi_check_draws", 65536))


def vi_check_keys(summary, draws, left_out, names):
    """The JSON keys of the fit check (all but vi_check_time_sec) from a diagnostics.ViCheckSummary; pure Python.  Of every
    per-element family the entry that stands out, with the element's name: the largest |gradient| (with its own value,
    signed, and its standard error), the largest score gap and |loc shift|, the smallest and the largest sd ratio."""
    s = summary
    keys = OrderedDict([("vi_check_draws", int(draws)), ("vi_check_draws_left_out", int(left_out)),
                        ("vi_pareto_k", s.pareto_k), ("vi_pareto_k_threshold", s.pareto_k_threshold),
                        ("vi_tail_length", int(s.tail_length)), ("vi_is_ess", s.is_ess), ("vi_elbo_final", s.elbo_final),
                        ("vi_elbo_final_se", s.elbo_final_se), ("vi_log_evidence", s.log_evidence),
                        ("vi_log_evidence_se", s.log_evidence_se), ("vi_kl_estimate", s.kl_estimate),
                        ("vi_kl_estimate_se", s.kl_estimate_se)])

    def stands_out(key, values, rank, extra=()):
        _, at = _nan_max(rank)
        keys[key] = _finite_or_none(values[at]) if at >= 0 else None
        for suffix, other in extra:
            keys[key + suffix] = _finite_or_none(other[at]) if at >= 0 else None
        keys[key + "_element"] = names[at] if at >= 0 else None
    stands_out("vi_elbo_grad_loc_max", s.elbo_grad_loc, np.abs(s.elbo_grad_loc), (("_se", s.elbo_grad_loc_se),))
    stands_out("vi_elbo_grad_scale_max", s.elbo_grad_scale, np.abs(s.elbo_grad_scale), (("_se", s.elbo_grad_scale_se),))
    stands_out("vi_score_gap_max", s.score_gap, s.score_gap)
    stands_out("vi_loc_shift_max", s.loc_shift, np.abs(s.loc_shift))
    stands_out("vi_sd_ratio_min", s.sd_ratio, -np.asarray(s.sd_ratio))
    stands_out("vi_sd_ratio_max", s.sd_ratio, s.sd_ratio)
    return keys


def vi_check_warning(keys):
    """The one warning of the fit check, or None: k-hat above its threshold, or no tail fitted.  No threshold is tied to
    the gradient figures: none can be derived (the rule of the trajectory and geometry reports)."""
    k, cap = keys["vi_pareto_k"], keys["vi_pareto_k_threshold"]
    if k is not None and cap is not None and k <= cap:
        return None
    return ("    WARNING: Pareto k-hat of the importance ratios p / q is {} (reliable up to {}): q is far from the posterior "
            "in this parameterisation.  The importance-corrected figures (vi_loc_shift_*, vi_sd_ratio_*, is_mean, is_sd) and "
            "vi_log_evidence / vi_kl_estimate are then unreliable (they are still written); try another --method.".format(
                "not fitted" if k is None else _fmt(k), _fmt(cap)))


def _fixed(v):
    return "n/a" if v is None else "{:.4f}".format(v)


def _fitted_q(spec, fit):
    """(loc, scale) float32 [D] of the stored `learned_variational_params`."""
    p = fit["learned_variational_params"]
    flat = lambda suffix: np.concatenate([np.asarray(p[name + suffix], np.float32).reshape(-1) for name in spec.part_names])
    return flat("_loc"), flat("_scale")


def _vi_check_report(model_config, fit, actual_reparam, file_path, flags):
    """--vi_diagnostics: is the mean-field fit `fit` (the keys run_vi writes) any good?  Draws from the fitted q in the
    coordinates of the parameterisation the fit ended in -- the method's (a, b) for CP, NCP and dVIP, the learned a with b
    as arp_vi_run read it for cVIP --, their importance ratios against that density on the device (diagnostics.vi_check)
    and the statistics of diagnostics.vi_check_summary.  The seed is derived from --seed and VI_CHECK_SEED.  Reads nothing
    but the stored fit, so a result file from a run without the flag gives the bits of a run with it (JSON round-trips
    float32 exactly).  Returns the JSON keys; writes <base>_vicheck.npz."""
    clock = time.time()
    spec = model_config.model
    reparam = fit.get("learned_reparam") if fit.get("learned_reparam") is not None else actual_reparam
    a, b = spec.ab_from_reparam(reparam)
    loc, scale = _fitted_q(spec, fit)
    import torch
    eng = _engine.engine_for(spec, torch.device(flags.device))
    eng.set_param(0, (a, b))
    draws = check_vi_check_draws(flags.vi_check_draws)
    seed = derived_seed(flags.seed, VI_CHECK_SEED)
    chk = diagnostics.vi_check(eng, loc, scale, which=0, draws=draws, seed=seed)
    summary = diagnostics.vi_check_summary(chk.elem, chk.tot, chk.out8, loc, scale, chk.e0, chk.logp_const)
    keys = vi_check_keys(summary, draws, chk.left_out, element_names(spec))
    util.print_("    fit check over {} draws from q ({} left out): Pareto k-hat {} (threshold {}), ELBO of the final parameters "
                "{} +- {}, log evidence {} +- {}, KL(q || p) {} +- {}; largest ELBO gradient along loc {} ({}), along log scale "
                "{} ({}); largest score gap {} ({}); importance-corrected sd / q's sd in {} ... {}".format(
                    draws, chk.left_out, _fmt(keys["vi_pareto_k"]), _fmt(keys["vi_pareto_k_threshold"]), _fixed(keys["vi_elbo_final"]),
                    _fmt(keys["vi_elbo_final_se"]), _fixed(keys["vi_log_evidence"]), _fmt(keys["vi_log_evidence_se"]),
                    _fmt(keys["vi_kl_estimate"]), _fmt(keys["vi_kl_estimate_se"]), _fmt(keys["vi_elbo_grad_loc_max"]),
                    keys["vi_elbo_grad_loc_max_element"], _fmt(keys["vi_elbo_grad_scale_max"]),
                    keys["vi_elbo_grad_scale_max_element"], _fmt(keys["vi_score_gap_max"]), keys["vi_score_gap_max_element"],
                    _fmt(keys["vi_sd_ratio_min"]), _fmt(keys["vi_sd_ratio_max"])))
    warning = vi_check_warning(keys)
    if warning:
        util.print_(warning)
    arrays = OrderedDict()
    _by_part(spec, arrays, [(family, getattr(summary, family)) for family in VI_CHECK_FAMILIES])
    arrays.update([("log_ratio", np.asarray(chk.log_ratio, np.float32)), ("log_weight", np.asarray(chk.log_weight, np.float64)),
                   ("left_out", np.asarray(chk.left_out, np.int64))])
    save_vicheck(file_path[:-5], arrays)
    keys["vi_check_time_sec"] = time.time() - clock
    return keys


def save_vicheck(file_path_base, arrays):
    """`<base>_vicheck.npz` (build-specific, --vi_diagnostics): per latent part `elbo_grad_loc/`, `elbo_grad_loc_se/`,
    `elbo_grad_scale/`, `elbo_grad_scale_se/`, `score_gap/`, `loc_shift/`, `sd_ratio/`, `is_mean/`, `is_sd/`; `log_ratio` [R]
    float32 (log p - log q of every draw, without the density's constant), `log_weight` [R] (its Pareto-smoothed,
    max-shifted log weight; -inf for a draw left out) and `left_out`."""
    np.savez(file_path_base + "_vicheck.npz", **arrays)


def run_vi(model_config, results_dir, file_path, flags=FLAGS):
    """reference main.py:234-290; with --vi_diagnostics the fit check after the fit's clock has stopped, or, for a result
    file that lacks it, from the stored fit."""
    target, model, elbo, vp, lp, actual_reparam = create_target_graph(model_config, results_dir, flags)
    want_check = getattr(flags, "vi_diagnostics", False)
    if os.path.exists(file_path):
        if want_check:
            with open(file_path, "r") as f:
                stored = json.load(f)
            if "vi_check_draws" not in stored:
                util.print_("fit check of the stored {}-{} fit of model {} with dataset {} (no refit)".format(
                    flags.inference, flags.method, flags.model, flags.dataset))
                stored.update(_vi_check_report(model_config, stored, actual_reparam, file_path, flags))
                _write_json_atomic(file_path, stored)
                return stored
        util.print_("Already ran experiment {}-{} on model {} with dataset {}. Skipping".format(
            flags.inference, flags.method, flags.model, flags.dataset))
        return
    prior = None
    if flags.discrete_prior:
        # a mixture of Laplace (not Beta or Kumaraswamy): finite at 0 and 1 (reference main.py:244-253)
        prior = inference.DiscretePrior()
    start_time = time.time()
    (elbo_final, elbo_timeline, learning_rate, initial_step_size, learned_variational_params,
     learned_reparam) = inference.find_best_learning_rate(
         elbo, vp, learnable_parameters_prior=prior, learnable_parameters=lp, flags=flags)
    end_time = time.time()
    if learned_reparam is None and isinstance(actual_reparam, dict):
        learned_reparam = actual_reparam
    results = {
        "elbo": float(elbo_final),
        "variational_fit_time_secs": end_time - start_time,
        "actual_num_variational_steps": len(elbo_timeline),
        "estimated_elbo_std": float(np.std(elbo_timeline[-32:])),
        "learning_rate": learning_rate,
        "initial_step_size": [np.asarray(i).item() if np.ndim(i) == 0 else np.asarray(i).tolist()
                              for i in initial_step_size],
        "learned_reparam": _clean_dict(learned_reparam),
        "learned_variational_params": _clean_dict(learned_variational_params),
    }
    if want_check:
        results.update(_vi_check_report(model_config, results, actual_reparam, file_path, flags))
    _write_json_atomic(file_path, results)
    return results


def get_best_num_leapfrog_steps_from_tuning_runs(tuning_runs):
    best_run = max(tuning_runs, key=lambda d: d["ess_min"])
    return best_run["num_leapfrog_steps"]


def _param_names(model_config):
    return list(model_config.model.part_names)


def _ess_chain_count(info, model_config, flags):
    """Chains of the whole job the ESS parts cover: all of them, or None for the chain subset of a streaming run
    (inference.EssInfo; the per-rank block lengths are then gathered with the values)."""
    if info is not None and info.batch_means is not None and info.estimator == "autocorrelation":
        return None
    return flags.num_chains


def _ess_report(info, model_config, flags, dev, ess_parts=None):
    """Build-specific keys next to the reference's `ess_min`: which estimator it is and on how many chains, how many of
    them never moved after burn-in, and -- for a streaming run -- the batch-means figure of ALL chains from the in-kernel
    accumulators.  (A collective when ws > 1: every rank calls it.)"""
    if info is None:
        return {}
    n_const = None
    if ess_parts is not None:
        # A chain that accepts nothing after burn-in has a constant recorded series: tfp's estimator gives 0 / 0 = nan and
        # util.get_min_ess counts the chain as 0.  With a step size frozen at the end of adaptation that happens to a few
        # chains per thousand in funnel-shaped posteriors (profiles/r05_stuck_chains.txt: the algorithm, not the
        # arithmetic) -- the summary says so instead of hiding them in the mean.
        parts = [np.asarray(e) for e in ess_parts]
        n = parts[0].shape[0] if parts else 0
        stuck = np.zeros(n, bool)
        for p in parts:                                        # [C, *event] each: one vector pass per part, not one per chain
            if n:                                              # (a rank can hold no ESS chains in a streaming run)
                stuck |= np.isnan(p.reshape(n, int(np.prod(p.shape[1:], dtype=np.int64)))).any(axis=1)
        local = int(stuck.sum())
        n_const = int(parallel.all_reduce_sum(float(local), dev).item())
        if n_const:
            util.print_("    {} chain(s) never moved after burn-in (constant series: ESS nan, counted as 0 by get_min_ess)".format(n_const))
    # every per-run key is a list with one entry per run (the reference's contract): whole-trace runs append None here
    out = {"ess_estimator": info.estimator, "ess_min_batch_means": None, "sem_min_batch_means": None,
           "batch_means_batch": None, "ess_constant_chains": n_const}
    n_local = int(info.chains)
    out["ess_chains"] = int(parallel.all_reduce_sum(float(n_local), dev).item())
    if info.batch_means is not None:
        norm = 1000.0 / (flags.num_samples * flags.num_leapfrog_steps)
        bm = np.nan_to_num(info.batch_means.cpu().numpy()) * norm          # [C_local, D]
        mins = parallel.all_gather_chains(bm.min(axis=1).astype(np.float32), flags.num_chains, dev).cpu().numpy()
        m, sem = parallel.mean_sem(mins)
        out.update(ess_min_batch_means=m, sem_min_batch_means=sem, batch_means_batch=int(info.batch))
        util.print_("    batch-means ESS of all {} chains (batches of {}): {} +/- {}".format(len(mins), info.batch, m, sem))
    return out


RHAT_WARN = 1.01          # the customary threshold above which chains are said not to have mixed


def _reduced(blocks, dev):
    """The `blocks` (arrays, tensors or scalars), summed over the ranks of the job in ONE all-reduce of their ravelled
    concatenation, as float64 numpy arrays of their own shapes."""
    local = [_lib.host64(b) for b in blocks]
    t = parallel.all_reduce_sum(np.concatenate([b.ravel() for b in local]), dev).cpu().numpy()
    return [part.reshape(b.shape) for part, b in zip(np.split(t, np.cumsum([b.size for b in local])[:-1]), local)]


def _by_part(spec, arrays, rows):
    """arrays["<key>/<part>"] = that latent part of the flat [..., D] array, for every (key, flat) of `rows`."""
    for key, flat in rows:
        for name, part in zip(spec.part_names, spec.unpack(flat)):
            arrays["%s/%s" % (key, name)] = part


def _convergence_report(kernel_results, model_config, flags, dev):
    """Build-specific (--convergence_diagnostics): do the chains of this run agree with each other?  Split R-hat of every
    element over the chains whose trace is on the device (all of them in a whole-trace run; the --ess_chains subset of a
    streaming run) and, for a streaming run, the un-split R-hat of ALL chains from the in-kernel statistics next to it
    (autoreparam_amd/diagnostics.py).  Returns (JSON keys, arrays for <base>_rhat.npz); ({}, None) when the run offers
    no device trace or the flag is off.  Called after the mcmc clock has stopped: its own wall time is a key of its own.
    Never raises on a short run, a rank without chains or constant series: those end in NaN (null in the JSON).
    (A collective when ws > 1: every rank calls it.)"""
    trace = getattr(kernel_results, "trace", None)
    if not getattr(flags, "convergence_diagnostics", True) or trace is None:
        keys = OrderedDict()
        for row in SIDE_REPORTS if getattr(flags, "convergence_diagnostics", True) else ():
            if row.null is not None and getattr(flags, row.flag, False):      # asked for, and says that it cannot run
                keys.update(row.null(flags))
        return keys, None
    clock = time.time()
    spec = model_config.model
    S, C_local, D = (int(v) for v in trace.shape)
    info, moments = kernel_results.ess_info, kernel_results.moments
    streaming = moments is not None
    k = C_local
    if streaming:
        # the kept trace also holds the --num_chains_to_save chains: the ESS subset is its leading block
        k = int(info.chains) if info is not None and info.estimator == "autocorrelation" else 0

    def reduced(sums, count):
        # the five [D] vectors and the chain count in ONE all-reduce per statistic
        sums, count = _reduced([sums, float(count)], dev)
        return sums, int(round(float(count)))

    by_part = lambda arrays, rows: _by_part(spec, arrays, rows)

    none = trace.new_empty(0, D)
    local = diagnostics.fold(*diagnostics.split_moments(trace[:, :k], split=True)) if k > 0 else diagnostics.fold(none, none)
    sums, n_split = reduced(local, k)
    split = diagnostics.rhat_from_sums(sums, S // 2)
    split_max, at = _nan_max(split.rhat)
    arrays = OrderedDict()
    by_part(arrays, (("split_rhat", split.rhat), ("posterior_mean", split.mean), ("posterior_sd", split.sd)))
    util.print_("    split R-hat over {} chains: max {:.4f} (element {})".format(n_split, split_max, at))
    all_max = float("nan")
    if streaming:
        sums_all, n_all = reduced(diagnostics.from_stats(*moments), int(moments[0].shape[0]))     # (the kept trace is narrower)
        whole = diagnostics.rhat_from_sums(sums_all, S)
        all_max, at_all = _nan_max(whole.rhat)
        by_part(arrays, (("rhat_all_chains", whole.rhat), ("posterior_mean_all_chains", whole.mean),
                         ("posterior_sd_all_chains", whole.sd)))
        util.print_("    R-hat of all {} chains (un-split, in-kernel statistics): max {:.4f} (element {})".format(
            n_all, all_max, at_all))
    if max(np.nan_to_num(split_max), np.nan_to_num(all_max)) > RHAT_WARN:
        util.print_("    WARNING: R-hat above {}: the chains have not converged to one distribution "
                    "(the elements: <base>_rhat.npz)".format(RHAT_WARN))
    rank_keys = {}
    if getattr(flags, "rank_normalized_rhat", False):
        rank_keys = _rank_report(trace, k, spec, arrays, by_part)
    keys = {"split_rhat_max": _finite_or_none(split_max), "split_rhat_chains": n_split,
            "rhat_max_all_chains": _finite_or_none(all_max) if streaming else None}
    keys.update(rank_keys)
    if getattr(flags, "bulk_tail_ess", False):
        keys.update(_bulk_tail_report(trace, k, spec, arrays, by_part))
    if int(getattr(flags, "superchain_size", 0) or 0) >= 2:
        keys.update(_nested_report(trace, moments, int(flags.superchain_size), dev, arrays, by_part))
    # the reports with a side file of their own: the file's arrays wait under a tag (_save_diagnostics takes them out again)
    pooled = whole if streaming else split                        # (n_split, the means and the sds: already all-reduced)
    run = _Run(kernel_results, trace, k, n_split, spec, flags, dev, arrays, split.mean, pooled.mean, pooled.sd)
    for row in SIDE_REPORTS:
        if row.report is not None and getattr(flags, row.flag, False):
            side_keys, side_arrays = row.report(run)
            keys.update(side_keys)
            if side_arrays is not None:
                arrays[row.tag] = side_arrays
    keys["diagnostics_time_sec"] = time.time() - clock
    return keys, arrays


ENERGY_ARRAYS = "energy/"            # where _convergence_report leaves the arrays of <base>_energy.npz among those of _rhat.npz
ENERGY_WHERE_MAX = 1024              # divergent rows whose states <base>_energy.npz keeps


def _probe_walk(ctx, trace, flags, seed_constant):
    """The rows both probe reports visit, so that they are the same rows: returns (steps, seed, visits).  `steps` is -1 for
    the final state of every chain of this rank, then --energy_probe_steps evenly spaced recorded steps of the device trace
    (the same on every rank); `seed` is derived from --seed and the report's own `seed_constant`.  `visits` yields, for
    every inner kernel j and every step s = steps[i] that has rows on this rank, (j, kn, i, s, centred, x, n, row_offset):
    the n rows centred and in kernel kn's coordinates (recorded states are centred and go through the existing transform)
    and the momentum-stream key of the first, the global chain id + num_chains x step index (the final state counts as
    step S)."""
    eng, S = ctx.engine, int(trace.shape[0])
    steps = [-1] + probe_steps(S, int(getattr(flags, "energy_probe_steps", 8)))
    seed = derived_seed(flags.seed, seed_constant)
    centred_final = eng.transform(ctx.q, which=0, to_centered=True) if int(ctx.q.shape[0]) > 0 else ctx.q

    def visits():
        for j, kn in enumerate(ctx.kernels):
            for i, s in enumerate(steps):
                centred = centred_final if s < 0 else trace[s].contiguous()
                n = int(centred.shape[0])
                if n == 0:
                    continue
                x = ctx.q if (s < 0 and kn.which == 0) else eng.transform(centred, which=kn.which, to_centered=False)
                yield j, kn, i, s, centred, x, n, ctx.chain_offset + int(flags.num_chains) * (S if s < 0 else s)
    return steps, seed, visits()


def _energy_summary(e):
    """The eight JSON keys of one diagnostics.Energy."""
    return OrderedDict([
        ("divergence_rate", _finite_or_none(e.divergence_rate)), ("divergent_trajectories", e.divergent),
        ("energy_probe_trajectories", e.rows), ("energy_nonfinite", e.nonfinite),
        ("energy_error_mean", _finite_or_none(e.error_mean)), ("energy_error_sd", _finite_or_none(e.error_sd)),
        ("energy_accept_prob", _finite_or_none(e.accept_prob)), ("energy_kinetic_share", _finite_or_none(e.kinetic_share))])


def _energy_report(kernel_results, trace, spec, flags, dev):
    """--energy_diagnostics: probe the finished run's integrator (Engine.energy_probe) -- one fresh-momentum trajectory with
    the run's own base steps, leapfrog count and per-chain step multipliers, NOT a replay of the transitions the sampler
    took -- from (a) the final state of every chain of this rank and (b) --energy_probe_steps evenly spaced recorded steps
    of the device trace (its chains are the rank's leading ones; recorded states are centred and go through the existing
    transform).  The momentum stream of a row is keyed by the global chain id + num_chains x step index (the final state
    counts as step S), under a seed derived from --seed.  --method=i probes both inner kernels, each with its own steps;
    the top-level keys then pool the two.  The nine sums are additive: a sharded job reports real numbers.
    Returns (JSON keys, arrays of <base>_energy.npz or None).  (A collective when ws > 1: every rank calls it.)"""
    import torch
    ctx = getattr(kernel_results, "probe", None)
    if ctx is None:
        return {}, None
    clock = time.time()
    eng, D = ctx.engine, int(spec.D)
    steps, seed, visits = _probe_walk(ctx, trace, flags, 0x454E5247)
    totals = [torch.zeros(9, dtype=torch.float64, device=ctx.q.device) for _ in ctx.kernels]
    errors = [np.full((len(steps), int(ctx.q.shape[0])), np.nan, np.float32) for _ in ctx.kernels]
    where = []
    for j, kn, i, s, centred, x, n, row_offset in visits:
        out = eng.energy_probe(x, kn.eps0, kn.n_leapfrog, which=kn.which, kappa=kn.kappa[:n], seed=seed + j,
                               row_offset=row_offset, lanes=flags.lanes_per_chain)
        totals[j] += diagnostics.energy_sums(out)
        o = out.to(torch.float64)
        dh = (o[:, 0] - o[:, 2]) + (o[:, 3] - o[:, 1])
        errors[j][i, :n] = dh.to(torch.float32).cpu().numpy()
        bad = torch.nonzero(~torch.isfinite(dh) | (dh > diagnostics.DIVERGENCE_THRESHOLD)).reshape(-1)[:ENERGY_WHERE_MAX]
        if bad.numel():
            rows = torch.cat([centred[bad].to(torch.float64), (bad + ctx.chain_offset).to(torch.float64)[:, None],
                              torch.full((bad.numel(), 1), float(s), dtype=torch.float64, device=bad.device),
                              torch.full((bad.numel(), 1), float(j), dtype=torch.float64, device=bad.device)], dim=1)
            where.append(rows.cpu().numpy())
    t = _reduced(totals, dev)
    by_kernel = [diagnostics.energy_from_sums(row, D) for row in t]
    pooled = diagnostics.energy_from_sums(np.sum(t, axis=0), D)
    keys = _energy_summary(pooled)
    if len(by_kernel) > 1:
        keys["energy_by_kernel"] = [_energy_summary(e) for e in by_kernel]
    util.print_("    energy probe over {} trajectories ({} probed step(s) and the final state): {} divergent, energy error "
                "{:.4f} +/- {:.4f}, expected acceptance {:.4f}, kinetic share of the energy variance {:.4f}".format(
                    pooled.rows, len(steps) - 1, pooled.divergent, pooled.error_mean, pooled.error_sd, pooled.accept_prob,
                    pooled.kinetic_share))
    if pooled.divergent > 0:
        util.print_("    WARNING: {} of {} probed trajectories diverged (rate {:.4g}: energy error not finite or above {:g}): "
                    "the integrator fails in part of this posterior -- try another parameterisation or a smaller step "
                    "(where: <base>_energy.npz)".format(pooled.divergent, pooled.rows, pooled.divergence_rate,
                                                        diagnostics.DIVERGENCE_THRESHOLD))
    # the arrays: every chain of the job in chain order, the divergent rows of all ranks in rank order
    local_where = np.concatenate(where, axis=0)[:ENERGY_WHERE_MAX] if where else np.zeros((0, D + 3))
    all_where = parallel.all_gather_chains(local_where, None, dev).cpu().numpy()[:ENERGY_WHERE_MAX]
    arrays = OrderedDict(steps=np.asarray(steps, np.int64))
    for j, err in enumerate(errors):
        whole = parallel.all_gather_chains(np.ascontiguousarray(err.T), int(flags.num_chains), dev).cpu().numpy().T
        arrays["energy_error" if j == 0 else "energy_error_%d" % j] = np.ascontiguousarray(whole)
    _by_part(spec, arrays, (("divergent_where", all_where[:, :D].astype(np.float32)),))
    arrays["divergent_chain"] = all_where[:, D].astype(np.int64)
    arrays["divergent_step"] = all_where[:, D + 1].astype(np.int64)
    arrays["divergent_kernel"] = all_where[:, D + 2].astype(np.int64)
    keys["energy_time_sec"] = time.time() - clock
    return keys, arrays


TRAJECTORY_ARRAYS = "trajectory/"    # where _convergence_report leaves the arrays of <base>_trajectory.npz


def _trajectory_summary(p, run_leapfrogs):
    """The per-kernel JSON keys of one diagnostics.Profile of a kernel that ran with `run_leapfrogs` leapfrog steps."""
    vec = lambda a: [_finite_or_none(v) for v in a]
    best, run = int(p.best_leapfrogs), int(run_leapfrogs)
    efficiency = None                                      # (the run's count is not among the profiled ones)
    if 1 <= run <= len(p.per_gradient) and best >= 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            efficiency = _finite_or_none(p.per_gradient[run - 1] / p.per_gradient[best - 1])
    return OrderedDict([
        ("trajectory_accept_prob", vec(p.accept_prob)), ("trajectory_divergence_rate", vec(p.divergence_rate)),
        ("trajectory_esjd_min", vec(p.esjd_min)), ("trajectory_esjd_min_element", [int(v) for v in p.esjd_min_element]),
        ("trajectory_esjd_min_per_gradient", vec(p.per_gradient)),
        ("trajectory_best_leapfrogs", best if best >= 1 else None), ("trajectory_run_leapfrogs", run),
        ("trajectory_efficiency_vs_best", efficiency)])


def _trajectory_report(kernel_results, trace, spec, flags, dev, pooled_sd):
    """--trajectory_profile=LMAX: did the run use the right number of leapfrog steps?  From the rows the energy report
    probes (both walk _probe_walk) -- the final state of every chain of this rank and --energy_probe_steps recorded steps of
    the device trace, the same row offsets, a seed constant of its own -- one fresh-momentum trajectory of LMAX steps with
    the run's own base steps and per-chain multipliers, every step recorded (Engine.trajectory_sums): the Metropolis-weighted expected
    squared jump distance of every element, in units of the run's pooled posterior variance, for every leapfrog count
    1 ... LMAX at once, the worst element's per gradient, and the count that maximises it.  NOT a replay of the sampler's
    transitions; the step sizes are those the run adapted for its own leapfrog count (a run at another count would adapt
    others); a one-transition (lag-one) criterion, not an ESS.  --method=i profiles both inner kernels, each with its own
    steps, and does not pool them into one recommendation.  The sums are additive: one all-reduce carries them.
    Returns (JSON keys, arrays of <base>_trajectory.npz or None).  (A collective when ws > 1: every rank calls it.)"""
    import torch
    from .flags import check_trajectory_profile
    Lmax = check_trajectory_profile(flags.trajectory_profile)
    ctx = getattr(kernel_results, "probe", None)
    if ctx is None or Lmax == 0:
        return {}, None
    clock = time.time()
    eng, D = ctx.engine, int(spec.D)
    _, seed, visits = _probe_walk(ctx, trace, flags, 0x54524A50)
    totals = [torch.zeros(Lmax, 5 + D, dtype=torch.float64, device=ctx.q.device) for _ in ctx.kernels]
    for j, kn, _, _, _, x, n, row_offset in visits:
        part, _ = eng.trajectory_sums(x, kn.eps0, Lmax, which=kn.which, kappa=kn.kappa[:n], seed=seed + j,
                                      row_offset=row_offset, lanes=flags.lanes_per_chain)
        totals[j] += part.to(totals[j].device)
    var = np.asarray(pooled_sd, np.float64) ** 2
    profiles = [diagnostics.profile_from_sums(row, var) for row in _reduced(totals, dev)]
    summaries = [_trajectory_summary(p, kn.n_leapfrog) for p, kn in zip(profiles, ctx.kernels)]
    keys = OrderedDict([("trajectory_leapfrogs_max", Lmax),
                        ("trajectory_probe_trajectories", int(round(sum(float(p.rows[0]) for p in profiles))))])
    if len(profiles) == 1:
        keys.update(summaries[0])
    else:
        keys["trajectory_by_kernel"] = summaries
    for j, (p, d) in enumerate(zip(profiles, summaries)):
        best, run = d["trajectory_best_leapfrogs"], d["trajectory_run_leapfrogs"]
        fig = lambda l: "n/a" if not (l and 1 <= l <= Lmax and np.isfinite(p.per_gradient[l - 1])) else "{:.4g}".format(p.per_gradient[l - 1])
        util.print_("    trajectory profile{} over {} trajectories of {} leapfrog steps: the worst element's expected squared "
                    "jump per gradient is largest at {} leapfrog step(s) ({}); this run took {} ({})".format(
                        "" if len(profiles) == 1 else " of kernel %d" % j, int(round(float(p.rows[0]))) if len(p.rows) else 0,
                        Lmax, best if best else "n/a", fig(best), run, fig(run)))
    arrays = OrderedDict(leapfrogs=np.arange(1, Lmax + 1, dtype=np.int64))
    for j, p in enumerate(profiles):
        tag = "" if j == 0 else "_%d" % j
        _by_part(spec, arrays, (("esjd" + tag, np.ascontiguousarray(p.esjd)),))
        arrays["accept_prob" + tag] = np.asarray(p.accept_prob, np.float64)
        arrays["divergence_rate" + tag] = np.asarray(p.divergence_rate, np.float64)
    keys["trajectory_time_sec"] = time.time() - clock
    return keys, arrays


GEOMETRY_ARRAYS = "geometry/"        # where _convergence_report leaves the arrays of <base>_geometry.npz
GEOMETRY_CHUNK_BYTES = 256 << 20     # a chunk's transformed [n, D] rows and their [n, 2 D] companion stay below this
GEOMETRY_KEYS = ("geometry_rows", "geometry_rows_left_out", "geometry_chains", "geometry_elements_left_out",
                 "geometry_condition_number", "geometry_condition_number_step_scaled", "geometry_condition_number_centred",
                 "geometry_max_abs_correlation", "geometry_max_correlation_pair", "geometry_max_scale_coupling",
                 "geometry_max_scale_coupling_pair")
GEOMETRY_KERNEL_KEYS = tuple(key for key in GEOMETRY_KEYS if key not in (
    "geometry_rows", "geometry_rows_left_out", "geometry_chains", "geometry_condition_number_centred"))


def geometry_chunk_steps(S, k, D, budget=GEOMETRY_CHUNK_BYTES):
    """Whole recorded steps per chunk of the geometry report: k chains of D floats each, three times over (the
    transformed rows and their [n, 2 D] companion), within `budget` bytes; at least one."""
    return int(max(1, min(max(int(S), 1), budget // max(1, 12 * int(k) * int(D)))))


def _geometry_summary(g, K, names):
    """The per-kernel JSON keys of one diagnostics.Geometry and its coupling matrix K (None: not computed)."""
    pair = [names[i] for i in g.max_correlation_pair] if g.max_correlation_pair[0] >= 0 else None
    worst_k, pair_k = None, None
    if K is not None and K.size:
        i, j = np.unravel_index(int(np.abs(K).argmax()), K.shape)
        worst_k, pair_k = _finite_or_none(abs(K[i, j])), [names[i], names[j]]      # the driving element first
    return OrderedDict([
        ("geometry_elements_left_out", int(len(g.left_out))),
        ("geometry_condition_number", _finite_or_none(g.condition_number)),
        ("geometry_condition_number_step_scaled", _finite_or_none(g.step_scaled_condition_number)),
        ("geometry_max_abs_correlation", _finite_or_none(g.max_abs_correlation)),
        ("geometry_max_correlation_pair", pair),
        ("geometry_max_scale_coupling", worst_k), ("geometry_max_scale_coupling_pair", pair_k)])


def _full(matrix, kept, D):
    """A [k, k] matrix over the kept elements as [D, D], NaN at the elements left out."""
    out = np.full((D, D), np.nan)
    out[np.ix_(kept, kept)] = matrix
    return out


def _geometry_report(kernel_results, trace, k, spec, flags, dev, pooled_mean):
    """--geometry_diagnostics: WHY does this parameterisation mix the way it does?  The cross moments of the recorded draws
    (diagnostics.gram_sums: arp_gram_sums on the matrix cores) over the leading `k` chains of the device trace -- the
    chains split R-hat covers -- in two coordinate systems: centred, the trace as it is, and the sampler's own, through
    the engine's transform, for every inner kernel of the run (--method=i has two).  From them the correlation matrix, its
    condition number, the stiff and the soft direction, the condition number of the covariance scaled by the run's own
    base steps, and -- a second pass with the first's mean and sd -- the scale coupling K (diagnostics.scale_coupling:
    the funnel detector).  The rows are taken in chunks of whole recorded steps (GEOMETRY_CHUNK_BYTES).  `pooled_mean`:
    the all-reduced pooled centred mean [D]; its transform is the shift of pass 1, identical on every rank, so the sums
    add: each pass ends in one all-reduce and a sharded job reports real numbers.  A second-order summary pooled over
    chains, not a local metric; unconverged chains inflate it.  No warning threshold is applied: none can be derived.
    Returns (JSON keys, arrays of <base>_geometry.npz or None).  (A collective when ws > 1: every rank calls it.)"""
    import torch
    ctx = getattr(kernel_results, "probe", None)
    if ctx is None:
        return {}, None
    clock = time.time()
    eng, D = ctx.engine, int(spec.D)
    S = int(trace.shape[0])
    k = int(k) if S > 0 else 0
    kernels = list(ctx.kernels)
    nk = len(kernels)
    device = trace.device
    null = OrderedDict((key, None) for key in GEOMETRY_KEYS)
    if D > diagnostics.GRAM_MAX_D:
        util.print_("    posterior geometry: not computed for more than {} elements".format(diagnostics.GRAM_MAX_D))
        null["geometry_time_sec"] = time.time() - clock
        return null, None
    couple = 2 * D <= diagnostics.GRAM_MAX_D
    centre = np.nan_to_num(np.asarray(pooled_mean, np.float64).reshape(D), nan=0.0, posinf=0.0, neginf=0.0).astype(np.float32)
    shift_c = torch.as_tensor(centre, device=device)
    # one row through the engine's transform: the shift of every kernel's coordinates (a finite guess is all it has to be)
    shifts = [eng.transform(shift_c[None, :], which=kn.which, to_centered=False)[0].contiguous() for kn in kernels]
    shifts = [torch.where(torch.isfinite(s), s, torch.zeros_like(s)) for s in shifts]
    steps = geometry_chunk_steps(S, k, D)

    def chunks():
        for s0 in range(0, S if k > 0 else 0, steps):
            yield trace[s0:s0 + steps, :k]

    # pass 1: the cross moments, centred and in every kernel's coordinates
    total = [torch.zeros(D + 2, D, dtype=torch.float64, device=device) for _ in range(1 + nk)]
    for chunk in chunks():
        total[0] += diagnostics.gram_sums(chunk, shift_c)
        rows = chunk.reshape(-1, D)
        for j, kn in enumerate(kernels):
            total[1 + j] += diagnostics.gram_sums(eng.transform(rows, which=kn.which, to_centered=False), shifts[j])
    sums = _reduced(total + [float(k)], dev)
    n_chains = int(round(float(sums.pop())))
    if sums[0][D + 1, 0] < 1:                      # no chain with a device trace anywhere in the job
        null["geometry_time_sec"] = time.time() - clock
        return null, None
    centred = diagnostics.geometry_from_sums(sums[0], shift=centre)
    geo = [diagnostics.geometry_from_sums(sums[1 + j], eps0=kn.eps0, shift=shifts[j]) for j, kn in enumerate(kernels)]

    # pass 2: the scale coupling in every kernel's coordinates, with pass 1's mean and sd
    Ks = [None] * nk
    if couple:
        total2 = [torch.zeros(2 * D + 2, 2 * D, dtype=torch.float64, device=device) for _ in range(nk)]
        for chunk in chunks():
            rows = chunk.reshape(-1, D)
            for j, kn in enumerate(kernels):
                x = eng.transform(rows, which=kn.which, to_centered=False)
                total2[j] += diagnostics.scale_coupling(x, geo[j].mean, geo[j].sd)
        Ks = [diagnostics.coupling_from_sums(s) for s in _reduced(total2, dev)]

    names = element_names(spec)
    summaries = [_geometry_summary(g, K, names) for g, K in zip(geo, Ks)]
    left = sums[0][D + 1, 1] if D > 1 else float(S) * n_chains - sums[0][D + 1, 0]
    keys = OrderedDict([("geometry_rows", int(round(sums[0][D + 1, 0]))), ("geometry_rows_left_out", int(round(left))),
                        ("geometry_chains", n_chains)])
    keys.update(summaries[0])
    keys["geometry_condition_number_centred"] = _finite_or_none(centred.condition_number)
    if nk > 1:
        keys["geometry_by_kernel"] = summaries
    for j, d in enumerate(summaries):
        util.print_("    posterior geometry{} over {} draws of {} chains: condition number of the correlation matrix {} in the "
                    "sampler's coordinates ({} scaled by its steps), {} centred; largest |correlation| {} ({}); largest scale "
                    "coupling {} ({})".format(
                        "" if nk == 1 else " of kernel %d" % j, keys["geometry_rows"], n_chains,
                        _fmt(d["geometry_condition_number"]), _fmt(d["geometry_condition_number_step_scaled"]),
                        _fmt(keys["geometry_condition_number_centred"]), _fmt(d["geometry_max_abs_correlation"]),
                        " ~ ".join(d["geometry_max_correlation_pair"] or ["n/a"]), _fmt(d["geometry_max_scale_coupling"]),
                        " -> ".join(d["geometry_max_scale_coupling_pair"] or ["n/a"])))
    arrays = OrderedDict(elements=np.asarray(names))
    arrays["correlation_centred"] = _full(centred.correlation, centred.kept, D)
    arrays["eigenvalues_centred"] = centred.eigenvalues
    for j, (g, K) in enumerate(zip(geo, Ks)):
        tag = "" if j == 0 else "_%d" % j
        arrays["mean" + tag], arrays["sd" + tag] = g.mean, g.sd
        arrays["correlation" + tag] = _full(g.correlation, g.kept, D)
        arrays["eigenvalues" + tag] = g.eigenvalues
        arrays["step_scaled_eigenvalues" + tag] = g.step_scaled_eigenvalues
        arrays["scale_coupling" + tag] = np.full((D, D), np.nan) if K is None else K
        _by_part(spec, arrays, (("stiffest_direction" + tag, g.stiffest_direction), ("softest_direction" + tag, g.softest_direction)))
    keys["geometry_time_sec"] = time.time() - clock
    return keys, arrays


LOO_ARRAYS = "loo/"                  # where _convergence_report leaves the arrays of <base>_loo.npz
LOO_KEYS = ("loo_draws", "loo_draws_left_out", "loo_chains", "loo_steps", "loo_observations", "elpd_loo", "elpd_loo_se",
            "p_loo", "elpd_waic", "elpd_waic_se", "p_waic", "pareto_k_max", "pareto_k_max_observation",
            "pareto_k_threshold", "pareto_k_above_threshold", "loo_nonfinite_observations", "loo_time_sec")
LOO_PRED_ARRAYS = "loopred/"         # where _loo_report leaves the arrays of <base>_loopred.npz (--loo_predictive)
LOO_PRED_KEYS = ("loo_pred_observations", "loo_pred_observations_left_out", "loo_pit_ks", "loo_coverage_90", "loo_rmse",
                 "loo_r2", "loo_brier", "loo_accuracy", "loo_balanced_accuracy", "loo_is_ess_min",
                 "loo_is_ess_min_observation", "loo_pred_time_sec")


LOGO_ARRAYS = "logo/"                # where _loo_report leaves the arrays of <base>_logo.npz among those of _loo.npz (--loo_groups)
LOGO_SHOWN = 8                       # groups with a high marginal k-hat the warning names
_LOGO_FORM = ("elpd", "elpd_se", "p", "pareto_k_max", "pareto_k_max_group", "pareto_k_above_threshold")
LOGO_MARGINAL_KEYS = ("elpd_logo", "elpd_logo_se", "p_logo", "logo_pareto_k_max", "logo_pareto_k_max_group",
                      "logo_pareto_k_above_threshold")
LOGO_KEYS = (("logo_part", "logo_groups", "logo_groups_empty", "logo_observations_left_out", "logo_draws") + LOGO_MARGINAL_KEYS
             + tuple("logo_conditional_" + name for name in _LOGO_FORM)
             + ("logo_pareto_k_threshold", "logo_nonfinite_groups", "logo_marginal", "logo_time_sec"))


def loo_groups_part(flags):
    """The part --loo_groups names; "" without the flag."""
    return getattr(flags, "loo_groups", "") or ""


def _check_extends(flags, name, parent, nothing):
    """The two refusals every flag that extends a report over the data opens with: --`name` without --`parent`, and
    neals_funnel, which has no observations and hence no `nothing`."""
    if not getattr(flags, parent, False):
        raise ValueError("--%s is read with --%s only" % (name, parent))
    if flags.model == "neals_funnel":
        raise ValueError("--%s: neals_funnel has no observations, so there is no %s" % (name, nothing))


def check_loo_groups(flags):
    """--loo_groups against the job, before anything runs -- raises ValueError, naming the flag: _check_extends' two
    refusals (--predictive_diagnostics), and whatever diagnostics.group_selection refuses: a name that is no part, a part of
    one element, a part no observation reads, a part whose elements do not group the data."""
    part = loo_groups_part(flags)
    if not part:
        return
    _check_extends(flags, "loo_groups", "predictive_diagnostics", "group to leave out")
    spec = models.spec_by_name(flags.model, dataset=getattr(flags, "dataset", None))
    diagnostics.group_selection(spec.observation_table(), spec, part, flag=diagnostics.LOGO_FLAG)


def check_predictive(flags):
    """--predictive_diagnostics and --loo_predictive against the job, before anything runs: raises ValueError for a model
    without observations (neals_funnel), whose pointwise log-likelihood does not exist, and for --loo_predictive without
    the report it extends."""
    if getattr(flags, "loo_predictive", False) and not getattr(flags, "predictive_diagnostics", False):
        raise ValueError("--loo_predictive: --predictive_diagnostics is required (the report folds the predictive "
                         "quantities with the weights of its Pareto fits)")
    if getattr(flags, "predictive_diagnostics", False) and flags.model == "neals_funnel":
        raise ValueError("--predictive_diagnostics: neals_funnel has no observations, so there is no pointwise "
                         "log-likelihood to cross-validate")


def _centred_engine(spec, dev):
    """An engine of a report's own, set to CP: the centred log joint at recorded draws; the run's handles stay as they are."""
    eng = _engine.Engine(spec, dev)
    eng.set_param(0, "CP")
    return eng


def loo_tile_rows(N, R, budget=None):
    """report_common.loo_tile_rows within THIS module's LOO_CHUNK_BYTES, the budget of every tile the reports here size."""
    return report_common.loo_tile_rows(N, R, LOO_CHUNK_BYTES if budget is None else budget)


def _loo_null(why, flags=None):
    """Every key of the predictive report, and with --loo_predictive, --loo_groups and --loo_moment_match of those reports
    too, as null; one message says why."""
    mm = loo_moment_match(flags)
    return _null_keys("PSIS-LOO / WAIC", why, LOO_KEYS + (LOO_PRED_KEYS if getattr(flags, "loo_predictive", False) else ())
                      + (LOGO_KEYS if loo_groups_part(flags) else ()) + (LOO_MM_KEYS if mm else ())
                      + (LOGO_MM_KEYS if mm and loo_groups_part(flags) else ()))


def loo_pred_keys(summary):
    """The JSON keys of the leave-one-out predictive report (all but loo_pred_time_sec) from a
    diagnostics.LooPredSummary; pure Python."""
    num = lambda v: None if v is None else _finite_or_none(v)
    at = int(summary.is_ess_min_observation)
    return OrderedDict([
        ("loo_pred_observations", int(summary.observations)), ("loo_pred_observations_left_out", int(summary.left_out)),
        ("loo_pit_ks", num(summary.pit_ks)), ("loo_coverage_90", num(summary.coverage_90)), ("loo_rmse", num(summary.rmse)),
        ("loo_r2", num(summary.r2)), ("loo_brier", num(summary.brier)), ("loo_accuracy", num(summary.accuracy)),
        ("loo_balanced_accuracy", num(summary.balanced_accuracy)), ("loo_is_ess_min", num(summary.is_ess_min)),
        ("loo_is_ess_min_observation", at if at >= 0 else None)])


def loo_keys(columns, R, left_out, n_chains, n_steps):
    """The JSON keys of the predictive report from the [N, 8] per-observation columns of diagnostics.psis_loo (host
    float64), the draws taken `R` and how many of them were left out; pure numpy."""
    c = np.asarray(columns, np.float64).reshape(-1, 8)
    used = int(R) - int(left_out)
    total = diagnostics.loo_summary(c[:, 0], c[:, 2], c[:, 3])
    threshold = diagnostics.pareto_k_threshold(used)
    k_max, at = _nan_max(c[:, 1])
    above = int(np.sum(_above(c[:, 1], threshold)))
    return OrderedDict([
        ("loo_draws", used), ("loo_draws_left_out", int(left_out)), ("loo_chains", int(n_chains)), ("loo_steps", int(n_steps)),
        ("loo_observations", int(c.shape[0])),
        ("elpd_loo", _finite_or_none(total.elpd_loo)), ("elpd_loo_se", _finite_or_none(total.elpd_loo_se)),
        ("p_loo", _finite_or_none(total.p_loo)), ("elpd_waic", _finite_or_none(total.elpd_waic)),
        ("elpd_waic_se", _finite_or_none(total.elpd_waic_se)), ("p_waic", _finite_or_none(total.p_waic)),
        ("pareto_k_max", _finite_or_none(k_max)), ("pareto_k_max_observation", at if at >= 0 else None),
        ("pareto_k_threshold", _finite_or_none(threshold)), ("pareto_k_above_threshold", above),
        ("loo_nonfinite_observations", int(np.sum(~np.isfinite(c[:, 0]))))])


def _logo_form_keys(columns, names, threshold, prefix):
    """The six keys of one form (marginal: prefix "", conditional: "logo_conditional_") from its [G, 8] columns, the empty
    groups' rows NaN; all null without columns (no marginal form)."""
    keys = LOGO_MARGINAL_KEYS if not prefix else tuple(prefix + name for name in _LOGO_FORM)
    if columns is None:
        return OrderedDict((key, None) for key in keys)
    total = diagnostics.logo_summary(columns).total
    filled = ~np.all(np.isnan(columns), axis=1)
    k = np.where(filled, columns[:, 1], np.nan)
    k_max, at = _nan_max(k)
    above = int(np.sum(_above(k, threshold, filled)))
    return OrderedDict(zip(keys, (_finite_or_none(total.elpd_loo), _finite_or_none(total.elpd_loo_se), _finite_or_none(total.p_loo),
                                  _finite_or_none(k_max), names[at] if at >= 0 else None, above)))


def logo_keys(conditional, marginal, part, names, n_ungrouped, R, left_out):
    """The JSON keys of leave-one-group-out (all but logo_time_sec) from the [G, 8] per-group columns of diagnostics.psis_loo
    on the conditional and on the marginal group log-likelihood (host float64, an empty group's row NaN; marginal: None when
    the model has no closed marginal form, its six keys are then null and logo_marginal is false); pure numpy.  elpd, its se
    over groups and p = sum_g (lppd_g - elpd_g) per form; the worst k-hat is named by its group (`m[17]`);
    logo_nonfinite_groups counts the non-empty groups whose elpd is not finite in a form that was computed."""
    c = np.asarray(conditional, np.float64).reshape(-1, 8)
    m = None if marginal is None else np.asarray(marginal, np.float64).reshape(-1, 8)
    used = int(R) - int(left_out)
    threshold = diagnostics.pareto_k_threshold(used)
    filled = ~np.all(np.isnan(c), axis=1)
    bad = ~np.isfinite(c[:, 0]) if m is None else (~np.isfinite(c[:, 0]) | ~np.isfinite(m[:, 0]))
    keys = OrderedDict([("logo_part", part), ("logo_groups", int(c.shape[0])), ("logo_groups_empty", int(np.sum(~filled))),
                        ("logo_observations_left_out", int(n_ungrouped)), ("logo_draws", used)])
    keys.update(_logo_form_keys(m, names, threshold, ""))
    keys.update(_logo_form_keys(c, names, threshold, "logo_conditional_"))
    keys.update([("logo_pareto_k_threshold", _finite_or_none(threshold)), ("logo_nonfinite_groups", int(np.sum(filled & bad))),
                 ("logo_marginal", m is not None)])
    return keys


def logo_columns(draws, table, groups, site, sizes, budget=None):
    """(conditional [G, 8], marginal [G, 8] or None, mask) host float64: diagnostics.psis_loo on the conditional and (with
    `site`) the marginal group log-likelihood of every group at the draws `draws` [S, C, D] (diagnostics.group_loglik), in
    ascending ranges of groups whose lc, lm and PSIS workspace stay within `budget` (report_common.logo_range_size) -- a
    group's row does not depend on the range it came in.  The rows of empty groups (sizes [G] == 0) are NaN throughout."""
    import torch
    R = int(draws.shape[0]) * int(draws.shape[1])
    forms = 2 if site is not None else 1
    per = report_common.logo_range_size(groups.G, R, forms, diagnostics.psis_workspace_bytes,
                                        LOO_CHUNK_BYTES if budget is None else budget)
    buffer = torch.empty(forms * per, R, dtype=torch.float32, device=draws.device)
    cond, marg, mask = [], [], None
    for g0 in range(0, groups.G, per):
        lc, lm, mask, _ = diagnostics.group_loglik(draws, table, groups, site, g0, min(groups.G, g0 + per), out=buffer)
        cond.append(diagnostics.psis_loo(lc, mask).cpu().numpy())
        if lm is not None:
            marg.append(diagnostics.psis_loo(lm, mask).cpu().numpy())
    del buffer
    empty = np.asarray(sizes).reshape(-1) == 0
    out = []
    for blocks in (cond, marg):
        c = np.concatenate(blocks, axis=0) if blocks else None
        if c is not None:
            c[empty] = np.nan
        out.append(c)
    return out[0], out[1], mask


def _logo_report(draws, table, spec, part, R, left_out, flags=None):
    """--loo_groups=PART, the second half of _loo_report, on its draws: PSIS leave-one-GROUP-out, the groups being the
    observations that read one element of the latent part (diagnostics.marginal_selection: group_selection's rule).  Per
    group and draw the joint log-likelihood of the group's observations at the recorded effect (conditional) and, Normal
    data with a Normal leaf prior, with the group's own effect integrated against its conditional prior in closed form
    (marginal; diagnostics.group_loglik, one kernel for both) -- the per-(observation, draw) matrix is never materialised;
    diagnostics.psis_loo reads either in the place of a pointwise log-likelihood (logo_columns), its lppd and p_waic
    columns becoming the group WAIC.  The conditional ratio's k-hat is usually high -- the other draws' effect of a county
    says little about the posterior without the county -- and is the contrast the marginal form is read against (Merkle,
    Furr, Rabe-Hesketh 2019).  Returns (LOGO_KEYS, the arrays of <base>_logo.npz).
    Without a marginal form (Bernoulli data, ...) its keys are null and one message says why.
    With --loo_moment_match (`flags`) the groups whose CONDITIONAL k-hat is above the threshold are moment matched (_mm_run ->
    LOGO_MM_KEYS; the arrays of <base>_logo_mm.npz wait under LOGO_MM_ARRAYS for save_logo); no key or array above changes."""
    clock = time.time()
    dev, D = draws.device, int(draws.shape[2])
    site_host = spec.site_table()
    group_of, names, slope, elem, ok, why = diagnostics.marginal_selection(site_host, spec.observation_table(), spec, part)
    G = len(names)
    order, start = diagnostics.group_order(group_of, G)
    groups = diagnostics.upload_logo_groups(order, start, slope, elem, table.N, D, dev)
    if not ok:
        util.print_("    marginal leave-one-group-out by {}: not computed, {}".format(part, why))
    site = diagnostics.upload_site_table(site_host, D, dev) if ok else None
    cond, marg, mask = logo_columns(draws, table, groups, site, groups.sizes)
    keys = logo_keys(cond, marg, part, names, int(np.sum(group_of < 0)), R, left_out)
    form = lambda pre, e: "{} +/- {}, worst Pareto k-hat {} ({})".format(
        _fmt(keys[e]), _fmt(keys[e + "_se"]), _fmt(keys[pre + "pareto_k_max"]), keys[pre + "pareto_k_max_group"])
    util.print_("    PSIS leave-one-group-out by {}: {} groups ({} empty, {} observations in none), {} draws: marginal elpd_logo {}; "
                "conditional elpd {}".format(part, G, keys["logo_groups_empty"], keys["logo_observations_left_out"], keys["logo_draws"],
                                             form("logo_", "elpd_logo") if ok else "n/a",
                                             form("logo_conditional_", "logo_conditional_elpd")))
    if ok and keys["logo_pareto_k_above_threshold"]:
        threshold = keys["logo_pareto_k_threshold"]
        high = [names[g] for g in np.flatnonzero(_above(marg[:, 1], threshold, groups.sizes > 0))]
        util.print_("    WARNING: marginal Pareto k-hat above {} for {} group(s) of {}: {} -- their leave-group-out estimates "
                    "are unreliable (which: <base>_logo.npz)".format(_fmt(threshold), len(high), part, _shown(high, LOGO_SHOWN)))
    nan = np.full(G, np.nan)
    column = lambda c, j: nan.copy() if c is None else c[:, j]
    arrays = OrderedDict(
        grouped_head(part, names, group_of, groups.sizes)
        + [(pre + name, column(c, j)) for pre, c in (("", marg), ("conditional_", cond))
           for name, j in (("elpd_logo_g", 0), ("pareto_k", 1), ("lppd_g", 2), ("p_waic_g", 3))]
        + data_tail(table.y_host, spec))
    if loo_moment_match(flags):
        more, merged = _mm_run(draws, mask, left_out, spec, flags, cond, _TableLoglik(table, groups), "logo",
                               "group(s) of {}, conditional form".format(part), keys["logo_conditional_elpd"], names)
        merged.update([(name, arrays[name]) for name in ("part", "groups", "group_of", "y", "model")])
        arrays[LOGO_MM_ARRAYS] = merged                                    # (save_logo takes them out again)
        keys.update(more)
    keys["logo_time_sec"] = time.time() - clock
    return keys, arrays


LOO_MM_ARRAYS = "loo_mm/"            # where _loo_report leaves the arrays of <base>_loo_mm.npz among those of _loo.npz (--loo_moment_match)
LOGO_MM_ARRAYS = "logo_mm/"          # ... and _logo_report those of <base>_logo_mm.npz among those of _logo.npz
MM_MAX_RANGE = (1, 4096)             # --loo_moment_match_max
MM_SHOWN = 8                         # targets still above the threshold the warning names
_MM_FORM = ("observations", "not_attempted", "improved", "resolved", "iterations_max")
LOO_MM_KEYS = (tuple("loo_mm_" + name for name in _MM_FORM) + ("elpd_loo_mm", "elpd_loo_mm_se", "p_loo_mm", "loo_mm_pareto_k_max",
               "loo_mm_pareto_k_max_observation", "loo_mm_pareto_k_above_threshold", "loo_mm_full_pareto_k_max", "loo_mm_time_sec"))
LOGO_MM_KEYS = (tuple("logo_mm_" + name for name in _MM_FORM) + ("elpd_logo_mm", "elpd_logo_mm_se", "p_logo_mm",
                "logo_mm_pareto_k_max", "logo_mm_pareto_k_max_group", "logo_mm_pareto_k_above_threshold",
                "logo_mm_full_pareto_k_max", "logo_mm_time_sec"))


def loo_moment_match(flags):
    """Whether --loo_moment_match is set."""
    return bool(getattr(flags, "loo_moment_match", False))


def check_loo_moment_match(flags):
    """--loo_moment_match and --loo_moment_match_max against the job, before anything runs -- raises ValueError, naming the
    flag: _check_extends' two refusals (--predictive_diagnostics), and a cap outside MM_MAX_RANGE."""
    if not loo_moment_match(flags):
        return
    _check_extends(flags, "loo_moment_match", "predictive_diagnostics", "leave-one-out ratio to repair")
    cap = getattr(flags, "loo_moment_match_max", 64)
    if not (isinstance(cap, int) and MM_MAX_RANGE[0] <= cap <= MM_MAX_RANGE[1]):
        raise ValueError("--loo_moment_match_max: %r is outside %d ... %d" % (cap, MM_MAX_RANGE[0], MM_MAX_RANGE[1]))


def mm_select(pareto_k, threshold, cap):
    """(chosen, not_attempted): the indices of the targets whose k-hat is above `threshold` -- those without a fitted tail
    (+inf) included, NaN rows (empty groups) not -- the worst first (ties in ascending index), at most `cap` of them, and
    how many above the threshold lie past the cap; pure numpy."""
    k = np.asarray(pareto_k, np.float64).reshape(-1)
    above = np.flatnonzero(_above(k, threshold, ~np.isnan(k)))          # (a k-hat is finite or +inf, psis.hip; NaN: an empty group)
    ranked = above[np.argsort(-k[above], kind="stable")]
    return ranked[:int(cap)], int(max(0, ranked.size - int(cap)))


def mm_merge(columns, chosen, result):
    """The per-target arrays of <base>_loo_mm.npz / _logo_mm.npz from the plain [T, 8] columns (host float64), the targets
    handed to diagnostics.moment_match (`chosen`) and its MomentMatch over THEM: every figure is the plain one where the
    target was not attempted, the matched `elpd_loo_i` replaces the plain one where a map was accepted; pure numpy."""
    c = np.asarray(columns, np.float64).reshape(-1, 8)
    T, chosen = c.shape[0], np.asarray(chosen, np.int64).reshape(-1)
    D = int(result.scale.shape[1])
    attempted = np.zeros(T, bool)
    attempted[chosen] = True
    full = lambda values, fill, dtype=np.float64: _scatter(np.full(T, fill, dtype), chosen, values)
    wide = lambda values: _scatter(np.full((T, D), np.nan), chosen, values)
    return OrderedDict([
        ("attempted", attempted), ("elpd_loo_i", _scatter(c[:, 0].copy(), chosen, result.elpd)),
        ("pareto_k", _scatter(c[:, 1].copy(), chosen, result.pareto_k)), ("pareto_k_full", full(result.pareto_k_full, np.nan)),
        ("pareto_k_split", full(result.pareto_k_split, np.nan)), ("is_ess", full(result.is_ess, np.nan)),
        ("iterations", full(result.iterations, 0, np.int64)), ("maps", _scatter(np.full(T, "", object), chosen, result.maps).astype(str)),
        ("shift", wide(result.shift)), ("scale", wide(result.scale))])


def _scatter(into, at, values):
    if len(at):
        into[at] = np.asarray(values)[:len(at)]
    return into


def mm_keys(prefix, columns, merged, not_attempted, threshold, names=None):
    """The JSON keys of moment matching (all but the time) from the plain [T, 8] columns and mm_merge's arrays; pure numpy.
    prefix "loo": LOO_MM_KEYS, the worst k-hat named by its observation's index; "logo": LOGO_MM_KEYS, by its group's name
    (`names`), totals over the non-empty groups (diagnostics.logo_summary).  The totals go through loo_summary with the
    merged elpd column in the plain one's place: nothing is restated."""
    c = np.asarray(columns, np.float64).reshape(-1, 8).copy()
    tried = merged["attempted"]
    k_plain, k = c[:, 1].copy(), merged["pareto_k"]
    c[:, 0], c[:, 1] = merged["elpd_loo_i"], k
    grouped = prefix == "logo"
    total = diagnostics.logo_summary(c).total if grouped else diagnostics.loo_summary(c[:, 0], c[:, 2], c[:, 3])
    filled = ~np.all(np.isnan(c), axis=1)
    k_max, at = _nan_max(np.where(filled, k, np.nan))
    above = _above(k, threshold, filled)
    with np.errstate(invalid="ignore"):
        improved = int(np.sum(tried & (k < k_plain)))
        resolved = int(np.sum(tried & (k <= threshold)))
    kf_max, _ = _nan_max(np.where(tried, merged["pareto_k_full"], np.nan))
    e = "elpd_%s_mm" % prefix
    named = ("%s_mm_pareto_k_max_group" % prefix, names[at] if at >= 0 else None) if grouped else \
        ("%s_mm_pareto_k_max_observation" % prefix, at if at >= 0 else None)
    return OrderedDict([
        (prefix + "_mm_observations", int(tried.sum())), (prefix + "_mm_not_attempted", int(not_attempted)),
        (prefix + "_mm_improved", improved), (prefix + "_mm_resolved", resolved),
        (prefix + "_mm_iterations_max", int(merged["iterations"].max()) if tried.any() else 0),
        (e, _finite_or_none(total.elpd_loo)), (e + "_se", _finite_or_none(total.elpd_loo_se)),
        ("p_%s_mm" % prefix, _finite_or_none(total.p_loo)), (prefix + "_mm_pareto_k_max", _finite_or_none(k_max)), named,
        (prefix + "_mm_pareto_k_above_threshold", int(np.sum(above))), (prefix + "_mm_full_pareto_k_max", _finite_or_none(kf_max))])


def _mm_run(draws, mask, left_out, spec, flags, columns, loglik_fn, prefix, what, plain_total, names=None):
    """--loo_moment_match over the targets of one report (observations: prefix "loo"; groups in their conditional form:
    "logo") whose plain k-hat in `columns` [T, 8] is above the threshold, the worst --loo_moment_match_max first:
    diagnostics.moment_match on the report's draws, with the centred log joint of a _centred_engine and
    `loglik_fn(target, rows [1, n, D])` for the left-out term.
    mask [R], left_out: the report's left-out draws (moment_match adds those whose log joint is not finite).
    Prints the line that sets the matched total next to the plain one (`plain_total`), and one warning naming what is still above the
    threshold.  Returns (keys, mm_merge's arrays)."""
    import torch
    clock = time.time()
    dev, D = draws.device, int(draws.shape[2])
    R = int(draws.shape[0]) * int(draws.shape[1])
    x = draws.reshape(R, D)
    threshold = diagnostics.pareto_k_threshold(R - int(left_out))
    chosen, past = mm_select(columns[:, 1], threshold, getattr(flags, "loo_moment_match_max", 64))
    eng = _centred_engine(spec, dev)
    result = diagnostics.moment_match(
        x, mask, lambda rows: eng.logp_grad(rows, which=0)[0], lambda t, rows: loglik_fn(int(t), rows[None]), list(chosen),
        columns[chosen, 1], columns[chosen, 0], threshold, batch=report_common.mm_batch_size(max(len(chosen), 1), R, D, LOO_CHUNK_BYTES))
    del eng
    merged = mm_merge(columns, chosen, result)
    keys = mm_keys(prefix, columns, merged, past, threshold, names)
    label = (lambda t: names[t]) if names is not None else str
    plain_k, _ = _nan_max(columns[:, 1])
    e = "elpd_%s_mm" % prefix
    util.print_("    moment matching over {} {} ({} more above the threshold not attempted): k-hat fell for {}, at or below {} "
                "for {}; {} {} +/- {} (plain {}), worst Pareto k-hat {} (plain {}); full-posterior k-hat up to {}".format(
                    keys[prefix + "_mm_observations"], what, past, keys[prefix + "_mm_improved"], _fmt(_finite_or_none(threshold)),
                    keys[prefix + "_mm_resolved"], e, _fmt(keys[e]), _fmt(keys[e + "_se"]), _fmt(plain_total), _fmt(keys[prefix + "_mm_pareto_k_max"]),
                    _fmt(_finite_or_none(plain_k)), _fmt(keys[prefix + "_mm_full_pareto_k_max"])))
    high = np.flatnonzero(_above(merged["pareto_k"], threshold, ~np.isnan(merged["pareto_k"])))
    if high.size:
        util.print_("    WARNING: after moment matching the Pareto k-hat is still above {} for {} of the {}: {} -- their "
                    "estimates remain unreliable (which: <base>_{}_mm.npz)".format(
                        _fmt(_finite_or_none(threshold)), high.size, what, _shown([label(t) for t in high], MM_SHOWN), prefix))
    keys[prefix + "_mm_time_sec"] = time.time() - clock
    return keys, merged


class _TableLoglik(object):
    """loglik_fn of _mm_run over a DeviceTable: observation n (pointwise_loglik over [n, n + 1)) or, with `groups`, group g
    in its conditional form (group_loglik over [g, g + 1) without a site table)."""

    def __init__(self, table, groups=None):
        self.table, self.groups = table, groups

    def __call__(self, t, rows):
        if self.groups is None:
            return diagnostics.pointwise_loglik(rows, self.table, t, t + 1)[0][0]
        return diagnostics.group_loglik(rows, self.table, self.groups, None, t, t + 1)[0][0]


def _loo_report(kernel_results, trace, k, spec, flags, side=None):
    """--predictive_diagnostics: how well does this MODEL predict an observation it has not seen?  Over the leading `k`
    chains of the device trace -- the chains split R-hat covers -- and clamp(--loo_draws // k, 1, S) evenly spaced recorded
    steps (loo_steps): the pointwise log-likelihood of every observation at every draw (diagnostics.pointwise_loglik, from
    the model's observation table; the trace is centred, so one table serves every method), then PSIS-LOO and WAIC per
    observation (diagnostics.psis_loo), in tiles of observations whose log-likelihoods stay within LOO_CHUNK_BYTES; the
    per-observation columns are folded on the host (loo_keys).  A tail fit needs all draws of an observation in one place:
    a sharded job (world size > 1) writes null, says so once, and enters no collective -- the rule of the rank reports.
    No r_eff correction of the Monte-Carlo error, no moment matching or refits for high k-hat, no K-fold.
    --loo_predictive: the leave-one-out predictive report on the same draws.  A tile then holds the float64 log weights
    next to its log-likelihoods (a third of the rows, the two together within LOO_CHUNK_BYTES); diagnostics.psis_weights
    takes psis_loo's place -- the same columns bit for bit, and no column depends on the tiling, so every LOO_KEYS value
    and every array of <base>_loo.npz is the unflagged run's -- and diagnostics.loo_predictive folds mu, mu^2 + var and the
    PIT of every (observation, draw) with those weights; the per-observation sums are turned into the report on the host
    (diagnostics.loo_predictive_summary -> LOO_PRED_KEYS; no threshold can be derived for them, so no warning) and the
    arrays of <base>_loopred.npz are left in `side` under LOO_PRED_ARRAYS.  The keys are null whenever the report is.
    --loo_groups=PART: PSIS leave-one-group-out on the same draws (_logo_report -> LOGO_KEYS; the arrays of <base>_logo.npz
    wait under LOGO_ARRAYS for save_loo); it runs behind everything above and touches none of it.
    --loo_moment_match: moment matching for the observations (and, in _logo_report, the groups' conditional form) with a
    k-hat above the threshold (_mm_run -> LOO_MM_KEYS, LOGO_MM_KEYS; the arrays of <base>_loo_mm.npz and _logo_mm.npz wait
    under LOO_MM_ARRAYS and LOGO_MM_ARRAYS for save_loo); it runs last, adds keys and files, and changes none that exist.
    Returns (JSON keys, arrays of <base>_loo.npz or None)."""
    import torch
    pred = bool(getattr(flags, "loo_predictive", False))
    if parallel.world()[1] > 1:
        return _loo_null("the chains of a sharded job are on several devices (a tail fit needs all draws of an "
                         "observation on one)", flags), None
    clock = time.time()
    why, steps, draws = select_draws(trace, k, k, flags)
    if why:
        return _loo_null(why, flags), None
    table = diagnostics.upload_table(spec.observation_table(), int(trace.shape[2]), trace.device)
    R, N = len(steps) * k, table.N
    rows = loo_tile_rows(N, R, LOO_CHUNK_BYTES // 3) if pred else loo_tile_rows(N, R)
    ll_buffer = torch.empty(rows, R, dtype=torch.float32, device=trace.device)
    columns, sums, left_out, pred_time = [], [], 0, 0.0
    for n0 in range(0, N, rows):
        n1 = min(N, n0 + rows)
        ll, mask, n_masked = diagnostics.pointwise_loglik(draws, table, n0, n1, out=ll_buffer)
        if pred:
            out8, lw = diagnostics.psis_weights(ll, mask)
            columns.append(out8.cpu().numpy())
            pred_clock = time.time()                                      # (the copy above waited for the fits)
            sums.append(diagnostics.loo_predictive(draws, table, lw, n0, n1).cpu().numpy())
            pred_time += time.time() - pred_clock
            del lw
        else:
            columns.append(diagnostics.psis_loo(ll, mask).cpu().numpy())
        left_out = int(n_masked.item())                                   # (the same draws for every tile)
    del ll_buffer
    c = np.concatenate(columns, axis=0)
    keys = loo_keys(c, R, left_out, k, len(steps))
    util.print_("    PSIS-LOO over {} observations, {} draws ({} step(s) of {} chains, {} left out): elpd_loo {} +/- {}, "
                "p_loo {}; elpd_waic {} +/- {}; worst Pareto k-hat {} (observation {})".format(
                    N, keys["loo_draws"], len(steps), k, left_out, _fmt(keys["elpd_loo"]), _fmt(keys["elpd_loo_se"]),
                    _fmt(keys["p_loo"]), _fmt(keys["elpd_waic"]), _fmt(keys["elpd_waic_se"]), _fmt(keys["pareto_k_max"]),
                    keys["pareto_k_max_observation"]))
    if keys["pareto_k_above_threshold"]:
        util.print_("    WARNING: Pareto k-hat above {} for {} of {} observations (not fitted ones included): their "
                    "leave-one-out estimates are unreliable, the posterior hangs on them (which: <base>_loo.npz)".format(
                        _fmt(keys["pareto_k_threshold"]), keys["pareto_k_above_threshold"], N))
    arrays = OrderedDict([("elpd_loo_i", c[:, 0]), ("pareto_k", c[:, 1]), ("lppd_i", c[:, 2]), ("p_waic_i", c[:, 3])]
                         + data_tail(table.y_host, spec))
    if pred:
        pred_clock = time.time()
        summary = diagnostics.loo_predictive_summary(np.concatenate(sums, axis=0), table.y_host, table.kind)
        more = loo_pred_keys(summary)
        shown = (("LOO-PIT Kolmogorov distance", "loo_pit_ks"), ("90 % coverage", "loo_coverage_90"), ("RMSE", "loo_rmse"),
                 ("R^2", "loo_r2")) if table.kind == 0 else \
            (("Brier score", "loo_brier"), ("accuracy", "loo_accuracy"), ("balanced accuracy", "loo_balanced_accuracy"))
        util.print_("    LOO predictive report over {} observations ({} left out, not finite): {}; smallest importance-sampling "
                    "ESS {} (observation {})".format(
                        more["loo_pred_observations"], more["loo_pred_observations_left_out"],
                        ", ".join("{} {}".format(name, _fmt(more[key])) for name, key in shown), _fmt(more["loo_is_ess_min"]),
                        more["loo_is_ess_min_observation"]))
        if side is not None:
            side[LOO_PRED_ARRAYS] = OrderedDict([
                ("loo_mean", summary.loo_mean), ("loo_sd", summary.loo_sd), ("loo_pit", summary.loo_pit),
                ("loo_is_ess", summary.is_ess)] + data_tail(table.y_host, spec))
        keys.update(more)
        keys["loo_pred_time_sec"] = pred_time + (time.time() - pred_clock)
    if loo_groups_part(flags):
        logo, arrays[LOGO_ARRAYS] = _logo_report(draws, table, spec, loo_groups_part(flags), R, left_out, flags)    # (save_loo takes them out again)
        keys.update(logo)
    if loo_moment_match(flags):
        more, merged = _mm_run(draws, mask, left_out, spec, flags, c, _TableLoglik(table), "loo", "observation(s)", keys["elpd_loo"])
        merged.update(data_tail(table.y_host, spec))
        arrays[LOO_MM_ARRAYS] = merged                                     # (save_loo takes them out again)
        keys.update(more)
    keys["loo_time_sec"] = time.time() - clock
    return keys, arrays


def save_loo(file_path_base, arrays):
    """`<base>_loo.npz` (build-specific, --predictive_diagnostics): per observation `elpd_loo_i`, `pareto_k` (+inf where no
    tail was fitted), `lppd_i` and `p_waic_i` [N] float64; `y` [N], the observations themselves -- what
    diagnostics.loo_compare pairs two models by -- and `model`, the model's name.  With --loo_groups the arrays of
    <base>_logo.npz wait among them under LOGO_ARRAYS and are written by save_logo, with --loo_moment_match those of
    <base>_loo_mm.npz under LOO_MM_ARRAYS (save_mm): _loo.npz is the unflagged run's."""
    arrays = OrderedDict(arrays)
    grouped, matched = arrays.pop(LOGO_ARRAYS, None), arrays.pop(LOO_MM_ARRAYS, None)
    np.savez(file_path_base + "_loo.npz", **arrays)
    if grouped is not None:
        save_logo(file_path_base, grouped)
    if matched is not None:
        save_mm(file_path_base + "_loo_mm.npz", matched)


def save_logo(file_path_base, arrays):
    """`<base>_logo.npz` (build-specific, --loo_groups): `part`, the part whose elements are the groups; `groups` [G], their
    names; `group_of` [N] int32, the group of every observation (-1: none); `n_obs` [G], the groups' sizes; per group
    `elpd_logo_g`, `pareto_k`, `lppd_g`, `p_waic_g` [G] float64 of the MARGINAL form (NaN for an empty group, and
    throughout when the model has no marginal form) and the same four under `conditional_`; `y` [N] and `model` --
    what analyze --logo_compare pairs two models by."""
    arrays = OrderedDict(arrays)
    matched = arrays.pop(LOGO_MM_ARRAYS, None)
    np.savez(file_path_base + "_logo.npz", **arrays)
    if matched is not None:
        save_mm(file_path_base + "_logo_mm.npz", matched)


def save_mm(path, arrays):
    """`<base>_loo_mm.npz` and `<base>_logo_mm.npz` (build-specific, --loo_moment_match), per observation or group:
    `attempted` bool; `elpd_loo_i`, `pareto_k` (the matched figures where a map was accepted, the plain ones otherwise);
    `pareto_k_full`, `pareto_k_split`, `is_ess` (NaN where they do not exist); `iterations` and `maps` (the maps accepted,
    "112": T1, T1, T2); `shift`, `scale` [., D]: U - m0 and S of the total map theta = (x - m0) S + U in the centred
    coordinates, NaN where not attempted; `y`, `model`; for groups also `part`, `groups`, `group_of`."""
    np.savez(path, **arrays)


def save_loo_pred(file_path_base, arrays):
    """`<base>_loopred.npz` (build-specific, --loo_predictive): per observation `loo_mean`, `loo_sd`, `loo_pit` and
    `loo_is_ess` [N] float64 (NaN where the weights leave nothing to divide by); `y` [N], the observations themselves;
    `model`, the model's name.  The rows of observations with a high `pareto_k` in <base>_loo.npz are as unreliable as
    their `elpd_loo_i`."""
    np.savez(file_path_base + "_loopred.npz", **arrays)


PPC_ARRAYS = "ppc/"                  # where _convergence_report leaves the arrays of <base>_ppc.npz
PPC_SEED = 0x50504331                # the report's own seed constant (the probes have theirs)
PPC_EXTREME = (0.01, 0.99)           # the customary reading of an extreme predictive p-value, not a derived threshold
PPC_KEYS = ("ppc_draws", "ppc_draws_left_out", "ppc_chains", "ppc_steps", "ppc_observations", "ppc_p_mean", "ppc_p_sd",
            "ppc_p_min", "ppc_p_max", "ppc_p_deviance", "ppc_rep_mean", "ppc_rep_sd", "ppc_obs_mean", "ppc_obs_sd",
            "ppc_pit_ks", "ppc_coverage_90", "ppc_time_sec")


def check_predictive_checks(flags):
    """--predictive_checks against the job, before anything runs: check_predictive's rule for the other predictive
    report -- raises ValueError for a model without observations (neals_funnel), which has nothing to replicate."""
    if getattr(flags, "predictive_checks", False) and flags.model == "neals_funnel":
        raise ValueError("--predictive_checks: neals_funnel has no observations, so there is no data to replicate")


PPC_MIXED_ARRAYS = "ppc_mixed/"      # where _ppc_report leaves the arrays of <base>_ppc_mixed.npz among those of _ppc.npz
PPC_MIXED_SEED = 0x50504D58          # the mixed check's own seed constant: its redraws, and (the next seed) its replicates
PPC_MIXED_SHOWN = 8                  # observations with an extreme mixed PIT the printed line names
PPC_MIXED_KEYS = ("ppc_mixed_parts", "ppc_mixed_elements", "ppc_mixed_draws", "ppc_mixed_draws_left_out", "ppc_mixed_p_mean",
                  "ppc_mixed_p_sd", "ppc_mixed_p_min", "ppc_mixed_p_max", "ppc_mixed_p_deviance", "ppc_mixed_rep_mean",
                  "ppc_mixed_rep_sd", "ppc_mixed_pit_ks", "ppc_mixed_coverage_90", "ppc_mixed_pit_extreme_observations",
                  "ppc_mixed_pit_min_observation", "ppc_mixed_time_sec")


def redraw_parts(flags):
    """The names --predictive_checks_redraw gives, in the order given; [] without the flag."""
    text = getattr(flags, "predictive_checks_redraw", "") or ""
    return text.split(",") if text else []


def check_predictive_redraw(flags):
    """--predictive_checks_redraw against the job, before anything runs -- raises ValueError: _check_extends' two refusals
    (--predictive_checks), and whatever diagnostics.redraw_selection refuses: an empty name, a duplicate, a name that is no
    latent part, a selection that is not closed under descent."""
    names = redraw_parts(flags)
    if not names:
        return
    _check_extends(flags, "predictive_checks_redraw", "predictive_checks", "data to replicate")
    spec = models.spec_by_name(flags.model, dataset=getattr(flags, "dataset", None))
    diagnostics.redraw_selection(spec.site_table(), spec.part_names, names)


PPC_GROUP_ARRAYS = "ppc_groups/"     # where _ppc_report leaves the arrays of <base>_ppc_groups.npz among those of _ppc.npz
PPC_GROUP_SHOWN = 8                  # extreme groups the warning names
PPC_GROUP_LEVEL = 0.005              # 1 % two-sided, shared among the non-empty groups (Bonferroni): a convention
PPC_GROUP_STATISTICS = ("mean", "sd", "deviance")     # the statistics whose smallest and largest group p-value are keys
_PPC_GROUP_SUFFIXES = (("part", "groups", "groups_empty", "observations_left_out", "draws")
                       + tuple("p_%s_%s%s" % (name, end, tail) for name in PPC_GROUP_STATISTICS for end in ("min", "max")
                               for tail in ("", "_group")) + ("p_threshold", "extreme_groups", "time_sec"))
# (ppc_groups and ppc_groups_empty: the two counts read better without the second "group")
PPC_GROUP_KEYS = tuple(("ppc_" if suffix.startswith("groups") else "ppc_group_") + suffix for suffix in _PPC_GROUP_SUFFIXES)
PPC_GROUP_MIXED_KEYS = tuple("ppc_group_mixed_" + suffix for suffix in _PPC_GROUP_SUFFIXES)


def groups_part(flags):
    """The part --predictive_checks_groups names; "" without the flag."""
    return getattr(flags, "predictive_checks_groups", "") or ""


def check_predictive_groups(flags):
    """--predictive_checks_groups against the job, before anything runs -- raises ValueError: _check_extends' two refusals
    (--predictive_checks), and whatever diagnostics.group_selection refuses: a name that is no part, a part of one element,
    a part no observation reads, a part whose elements do not group the data."""
    part = groups_part(flags)
    if not part:
        return
    _check_extends(flags, "predictive_checks_groups", "predictive_checks", "data to group")
    spec = models.spec_by_name(flags.model, dataset=getattr(flags, "dataset", None))
    diagnostics.group_selection(spec.observation_table(), spec, part)


def _ppc_all_keys(flags):
    """The keys a run with these flags writes, in their order: PPC_KEYS, then PPC_MIXED_KEYS (--predictive_checks_redraw),
    then PPC_GROUP_KEYS (--predictive_checks_groups) and, with both flags, PPC_GROUP_MIXED_KEYS."""
    mixed, grouped = bool(redraw_parts(flags)), bool(groups_part(flags))
    return (PPC_KEYS + (PPC_MIXED_KEYS if mixed else ()) + (PPC_GROUP_KEYS if grouped else ())
            + (PPC_GROUP_MIXED_KEYS if grouped and mixed else ()))


def _ppc_null(why, flags=None):
    """Every key of the predictive checks, and of --predictive_checks_redraw and --predictive_checks_groups where set, as
    null; one message says why."""
    return _null_keys("posterior predictive checks", why, _ppc_all_keys(flags))


def ppc_group_keys(summary, part, names, n_ungrouped, mixed=False):
    """The JSON keys of the grouped predictive check (all but the time) from a diagnostics.PpcGroupSummary, the part, its
    groups' names and the number of observations in no group; pure Python.  mixed: under ppc_group_mixed_ (the groups
    of the data replicated at the redrawn rows).  Per statistic of PPC_GROUP_STATISTICS the smallest and the largest
    group p-value with their groups (null where no group defines it: sd of Bernoulli data).  p_threshold = PPC_GROUP_LEVEL
    / non-empty groups; extreme_groups: the groups whose p-value of the MEAN is <= the threshold or >= 1 - threshold, null
    when fewer than 1 / threshold draws were used -- a p-value is a multiple of 1 / draws and cannot resolve it then."""
    prefix = "ppc_group_mixed_" if mixed else "ppc_group_"
    filled = int(np.sum(summary.sizes > 0))
    keys = OrderedDict([(prefix + "part", part), (prefix + "groups" if mixed else "ppc_groups", int(summary.sizes.size)),
                        (prefix + "groups_empty" if mixed else "ppc_groups_empty", int(summary.sizes.size) - filled),
                        (prefix + "observations_left_out", int(n_ungrouped)), (prefix + "draws", int(summary.draws_used))])
    for name in PPC_GROUP_STATISTICS:
        p = summary.p[name]
        lo, hi = _nan_max(-p), _nan_max(p)
        keys[prefix + "p_%s_min" % name] = _finite_or_none(-lo[0])
        keys[prefix + "p_%s_min_group" % name] = names[lo[1]] if lo[1] >= 0 else None
        keys[prefix + "p_%s_max" % name] = _finite_or_none(hi[0])
        keys[prefix + "p_%s_max_group" % name] = names[hi[1]] if hi[1] >= 0 else None
    threshold = PPC_GROUP_LEVEL / filled if filled else None
    keys[prefix + "p_threshold"] = threshold
    extreme = None
    if threshold is not None and summary.draws_used * threshold >= 1.0:
        with np.errstate(invalid="ignore"):
            extreme = [names[g] for g in np.flatnonzero((summary.p["mean"] <= threshold) | (summary.p["mean"] >= 1.0 - threshold))]
    keys[prefix + "extreme_groups"] = extreme
    return keys


def _ppc_group_arrays(summary, prefix=""):
    """p_<T>, rep_<T>, obs_<T> [G] of <base>_ppc_groups.npz for the five statistics (NaN where not defined)."""
    return OrderedDict((prefix + "%s_%s" % (what, name), getattr(summary, what)[name])
                       for what in ("p", "rep", "obs") for name in diagnostics.PPC_STATISTICS)


def _ppc_group_report(grouped, spec, y, kind):
    """The second half of --predictive_checks_groups (_ppc_report): from the all-reduced per-group counts to the keys, the
    printed line, the warning and the arrays of <base>_ppc_groups.npz.  grouped: (part, group_of, names, posterior counts,
    mixed counts or None)."""
    part, group_of, names, counts, mixed_counts = grouped
    n_ungrouped = int(np.sum(group_of < 0))
    summary = diagnostics.ppc_group_summary(counts, y, group_of, kind)
    out = ppc_group_keys(summary, part, names, n_ungrouped)
    arrays = OrderedDict(grouped_head(part, names, group_of, summary.sizes))
    arrays.update(_ppc_group_arrays(summary))
    more = OrderedDict()
    if mixed_counts is not None:
        mixed_summary = diagnostics.ppc_group_summary(mixed_counts, y, group_of, kind)
        more = ppc_group_keys(mixed_summary, part, names, n_ungrouped, mixed=True)
        arrays.update(_ppc_group_arrays(mixed_summary, "mixed_"))
    arrays.update(data_tail(y, spec))
    ends = lambda k, pre: "{} ({}) ... {} ({})".format(_fmt(k[pre + "p_mean_min"]), k[pre + "p_mean_min_group"],
                                                      _fmt(k[pre + "p_mean_max"]), k[pre + "p_mean_max_group"])
    util.print_("    grouped predictive checks by {}: {} groups ({} empty, {} observations in none), {} draws; p-value of the "
                "group mean, smallest ... largest: {}{}".format(
                    part, out["ppc_groups"], out["ppc_groups_empty"], n_ungrouped, out["ppc_group_draws"], ends(out, "ppc_group_"),
                    "; mixed {}".format(ends(more, "ppc_group_mixed_")) if more else ""))
    shown = lambda groups: "{} group(s): {}".format(len(groups), _shown(groups, PPC_GROUP_SHOWN))
    extreme = [(label, k[pre + "extreme_groups"]) for label, k, pre in (("posterior", out, "ppc_group_"), ("mixed", more, "ppc_group_mixed_"))
               if k.get(pre + "extreme_groups")]
    if extreme:
        util.print_("    WARNING: predictive p-value of the group mean within {} of 0 or 1 ({} / non-empty groups: Bonferroni at "
                    "the customary 1 %, a convention, not a derived threshold) for groups of {} -- {} -- groups whose mean the "
                    "replicated data (almost) never or (almost) always exceed (the p-values: <base>_ppc_groups.npz)".format(
                        _fmt(out["ppc_group_p_threshold"]), PPC_GROUP_LEVEL, part,
                        "; ".join("{} {}".format(label, shown(groups)) for label, groups in extreme)))
    return out, more, arrays


def ppc_mixed_keys(summary, chosen, n_elements, kind):
    """The JSON keys of the mixed predictive check (all but ppc_mixed_time_sec) from the diagnostics.PpcSummary of the data
    replicated at the REDRAWN rows, the parts redrawn (in part order) and how many elements they hold; pure Python.  The
    nulls of Bernoulli data are those of ppc_keys; the two PIT keys are per observation and Normal data's alone, as
    ppc_pit_ks is."""
    num = lambda v: None if v is None else _finite_or_none(v)
    keys = OrderedDict([("ppc_mixed_parts", list(chosen)), ("ppc_mixed_elements", int(n_elements)),
                        ("ppc_mixed_draws", int(summary.draws_used)), ("ppc_mixed_draws_left_out", int(summary.draws_left_out))])
    for name in diagnostics.PPC_STATISTICS:
        keys["ppc_mixed_p_" + name] = num(summary.p[name])
    keys.update([("ppc_mixed_rep_mean", num(summary.rep["mean"])), ("ppc_mixed_rep_sd", num(summary.rep["sd"])),
                 ("ppc_mixed_pit_ks", num(summary.pit_ks)), ("ppc_mixed_coverage_90", num(summary.coverage_90))])
    pit = np.asarray(summary.pit, np.float64)
    defined = int(kind) == 0 and summary.draws_used > 0 and pit.size > 0
    with np.errstate(invalid="ignore"):
        extreme = np.flatnonzero((pit < PPC_EXTREME[0]) | (pit > PPC_EXTREME[1])) if defined else []
    at = _nan_max(-pit)[1] if defined else -1                              # (the smallest finite PIT)
    keys["ppc_mixed_pit_extreme_observations"] = [int(n) for n in extreme] if defined else None
    keys["ppc_mixed_pit_min_observation"] = at if at >= 0 else None
    return keys


def ppc_keys(summary, n_chains, n_steps):
    """The JSON keys of the predictive checks (all but ppc_time_sec) from a diagnostics.PpcSummary; pure Python."""
    num = lambda v: None if v is None else _finite_or_none(v)
    keys = OrderedDict([("ppc_draws", int(summary.draws_used)), ("ppc_draws_left_out", int(summary.draws_left_out)),
                        ("ppc_chains", int(n_chains)), ("ppc_steps", int(n_steps)),
                        ("ppc_observations", int(summary.observations))])
    for name in diagnostics.PPC_STATISTICS:
        keys["ppc_p_" + name] = num(summary.p[name])
    keys.update([("ppc_rep_mean", num(summary.rep["mean"])), ("ppc_rep_sd", num(summary.rep["sd"])),
                 ("ppc_obs_mean", num(summary.obs["mean"])), ("ppc_obs_sd", num(summary.obs["sd"])),
                 ("ppc_pit_ks", num(summary.pit_ks)), ("ppc_coverage_90", num(summary.coverage_90))])
    return keys


def _ppc_report(kernel_results, trace, k, k_total, spec, flags, dev):
    """--predictive_checks: does data simulated from the fitted MODEL look like the data?  Over the draws the predictive
    report takes (select_draws: the leading `k` chains of this rank's device trace, the chains split R-hat covers, at the
    steps that `k_total`, their number in the whole job, already all-reduced, gives) one replicated data set per draw at the
    observed covariates, folded on the device into per-draw test statistics and per-observation predictive sums
    (replicate_tiles).  The random numbers are keyed by (seed, observation, global draw number), the seed derived from
    --seed and PPC_SEED; a rank's first global draw number is its chain offset times the number of steps.  Every quantity
    is a sum over draws: the counts behind the p-values and the per-observation sums go through ONE all-reduce, and a
    sharded job reports real numbers (rank 0 writes them; <base>_ppc.npz then holds the draw statistics of rank 0's draws).
    The posterior PIT (the LOO-PIT: --loo_predictive); group-level statistics: --predictive_checks_groups, below; no
    user-defined statistic.
    --predictive_checks_redraw=PART[,PART...]: the MIXED predictive check (Gelman, Meng, Stern 1996; Marshall,
    Spiegelhalter 2007) on the same draws, the same tiles and the same global draw numbers.  The posterior check replicates
    y at group effects that were fitted to that very y, so it cannot say whether the effects look like draws from their own
    prior layer; here every draw keeps its hyperparameters, the named parts are drawn anew from their conditional prior
    given them (diagnostics.site_redraw over ModelSpec.site_table, the selection diagnostics.redraw_selection's, seeded by
    --seed and PPC_MIXED_SEED) and the data are replicated from the redrawn rows as a one-step trace [1, R, D]
    (replicate_tiles under the next seed -- the redraws' own would hand element d and observation d the same Philox
    words).  ppc_counts and ppc_from_counts as above, the counts and sums in the SAME all-reduce: no new statistic, no
    second definition, and real numbers from a sharded job.  The mixed PIT of an observation asks whether a NEW group under
    these hyperparameters would have produced it -- leave-group-out cross-validation without a refit.  Every PPC_KEYS value
    and every array of <base>_ppc.npz is the unflagged run's; the keys are null whenever the posterior check's are; the
    arrays of <base>_ppc_mixed.npz wait among the returned ones under PPC_MIXED_ARRAYS, where save_ppc finds them.
    Selection by part, not by element or group; the data are still replicated at the observed covariates.
    --predictive_checks_groups=PART: the same check per GROUP of observations -- the observations that read one element of
    the latent part (diagnostics.group_selection: radon's counties for m, election's states for a) -- on the same draws,
    seed and draw offset, so the replicated values are the posterior check's own, bit for bit: one more kernel pass
    (replicate_groups over arp_group_predictive_check) folds them per (group, draw), diagnostics.ppc_group_counts turns
    every group's rows into the counts ppc_counts defines -- no second definition of a statistic -- and the [G, PPC_COUNTS]
    counts join the SAME all-reduce.  With --predictive_checks_redraw too, a second pass over the redrawn rows the mixed
    check has on the device already (they are handed to both, not drawn twice) under the mixed check's seeds gives the
    figure the mixed replication exists for: which county is not a draw from its prior layer (Marshall, Spiegelhalter
    2007).  PPC_GROUP_KEYS (and PPC_GROUP_MIXED_KEYS), null whenever the posterior check's are; the arrays of
    <base>_ppc_groups.npz wait under PPC_GROUP_ARRAYS for save_ppc.  One part per run; groups by latent element, not by a
    covariate; the posterior p-values are conservative (the group effect was fitted to the group's own data), the mixed
    ones are the sharper check.  Without the flag every output is bit for bit unchanged.
    Returns (JSON keys, arrays of <base>_ppc.npz or None).  (A collective when ws > 1: every rank calls it.)"""
    clock = time.time()
    why, steps, draws = select_draws(trace, k, k_total, flags)
    if why:
        return _ppc_null(why, flags), None
    names = redraw_parts(flags)
    host_table = spec.observation_table()
    N, kind = int(np.asarray(host_table.y).size), int(host_table.kind)
    y = np.asarray(host_table.y, np.float32).reshape(-1)
    draw_offset = int(getattr(getattr(kernel_results, "probe", None), "chain_offset", 0)) * len(steps)
    counts, obs_sums, stats_host = np.zeros(diagnostics.PPC_COUNTS), np.zeros((N, len(diagnostics.PPC_OBS_COLUMNS))), None
    part, group_time, group_mixed_time = groups_part(flags), 0.0, 0.0
    if part:
        group_clock = time.time()
        group_of, group_names = diagnostics.group_selection(host_table, spec, part)
        group_counts = np.zeros((len(group_names), diagnostics.PPC_COUNTS))
        group_mixed_counts = np.zeros_like(group_counts) if names else None
        group_time = time.time() - group_clock
    if draws is not None:                                                    # (None: an idle rank, zeros into the all-reduce)
        table = diagnostics.upload_table(host_table, int(trace.shape[2]), trace.device)
        stats, sums, mask = replicate_tiles(draws, table, derived_seed(flags.seed, PPC_SEED), draw_offset, budget=LOO_CHUNK_BYTES)
        stats_host, obs_sums = _lib.host64(stats), _lib.host64(sums)
        counts = diagnostics.ppc_counts(stats_host, y, mask)
        if part:
            group_clock = time.time()
            groups = diagnostics.upload_groups(*diagnostics.group_order(group_of, len(group_names)), N, trace.device)
            group_counts, _ = replicate_groups(draws, table, groups, y, group_of, derived_seed(flags.seed, PPC_SEED), draw_offset,
                                               budget=LOO_CHUNK_BYTES)
            group_time += time.time() - group_clock
    mixed, mixed_time = None, 0.0
    if names:
        mixed_clock = time.time()
        redrawn = diagnostics.redraw_selection(spec.site_table(), spec.part_names, names)
        mixed_counts, mixed_sums, mixed_stats = np.zeros_like(counts), np.zeros_like(obs_sums), None
        if draws is not None:
            seed = derived_seed(flags.seed, PPC_MIXED_SEED)
            site = diagnostics.upload_site_table(spec.site_table(), int(trace.shape[2]), trace.device)
            rows, undrawn = diagnostics.site_redraw(draws, site, redrawn, seed=seed, draw_offset=draw_offset)
            stats, sums, mask = replicate_tiles(rows[None], table, next_seed(seed), draw_offset, budget=LOO_CHUNK_BYTES)
            left = (mask != 0) | (undrawn != 0)                              # (an undrawn element is NaN: masked too)
            mixed_stats, mixed_sums = _lib.host64(stats), _lib.host64(sums)
            mixed_counts = diagnostics.ppc_counts(mixed_stats, y, left)
            mixed_time = time.time() - mixed_clock
            if part:                                                         # (the redrawn rows serve both: not drawn twice)
                group_clock = time.time()
                group_mixed_counts, _ = replicate_groups(rows[None], table, groups, y, group_of, next_seed(seed), draw_offset,
                                                         left_out=undrawn != 0, budget=LOO_CHUNK_BYTES)
                group_mixed_time = time.time() - group_clock
            del rows
        else:
            mixed_time = time.time() - mixed_clock
    blocks = [counts, obs_sums] + ([mixed_counts, mixed_sums] if names else []) + ([group_counts] if part else []) \
        + ([group_mixed_counts] if part and names else [])
    blocks = _reduced(blocks, dev)                                           # (ONE all-reduce for everything the flags ask)
    counts, obs_sums = blocks[:2]
    if names:
        mixed = (redrawn, blocks[2], blocks[3], mixed_stats)
    if part:
        group_counts, group_mixed_counts = blocks[2 + 2 * bool(names)], (blocks[-1] if names else None)
    summary = diagnostics.ppc_from_counts(counts, obs_sums, y, kind)
    keys = ppc_keys(summary, k_total, len(steps))
    p = OrderedDict((name, keys["ppc_p_" + name]) for name in diagnostics.PPC_STATISTICS)
    util.print_("    posterior predictive checks over {} observations, {} draws ({} step(s) of {} chains, {} left out): "
                "p-values mean {}, sd {}, min {}, max {}, deviance {}; replicated mean {} against {} observed; PIT "
                "Kolmogorov distance {}, 90 % coverage {}".format(
                    N, keys["ppc_draws"], len(steps), int(k_total), keys["ppc_draws_left_out"], _fmt(p["mean"]), _fmt(p["sd"]),
                    _fmt(p["min"]), _fmt(p["max"]), _fmt(p["deviance"]), _fmt(keys["ppc_rep_mean"]), _fmt(keys["ppc_obs_mean"]),
                    _fmt(keys["ppc_pit_ks"]), _fmt(keys["ppc_coverage_90"])))
    extreme = [name for name, v in p.items() if v is not None and not PPC_EXTREME[0] <= v <= PPC_EXTREME[1]]
    if extreme:
        util.print_("    WARNING: posterior predictive p-value outside [{}, {}] for: {} -- replicated data sets (almost) never "
                    "or (almost) always exceed the observed statistic; customarily read as a misfit of the model in that "
                    "respect (a convention, not a derived threshold)".format(PPC_EXTREME[0], PPC_EXTREME[1], ", ".join(extreme)))
    arrays = OrderedDict([("predictive_mean", summary.predictive_mean), ("predictive_sd", summary.predictive_sd),
                          ("pit", summary.pit), ("y", y),
                          ("draw_stats", stats_host if stats_host is not None else np.zeros((0, len(diagnostics.PPC_DRAW_COLUMNS)))),
                          ("model", np.asarray(spec.name))])
    more = OrderedDict()
    if mixed is not None:
        mixed_clock = time.time()
        more, mixed_arrays = _ppc_mixed_report(mixed, names, keys, spec, y, kind)
        arrays[PPC_MIXED_ARRAYS] = mixed_arrays                               # (save_ppc takes them out again: a file of their own)
        more["ppc_mixed_time_sec"] = mixed_time + (time.time() - mixed_clock)
    if part:
        group_clock = time.time()
        group_keys, group_more, group_arrays = _ppc_group_report((part, group_of, group_names, group_counts, group_mixed_counts),
                                                                 spec, y, kind)
        arrays[PPC_GROUP_ARRAYS] = group_arrays                               # (save_ppc takes them out again, as the mixed ones)
        group_keys["ppc_group_time_sec"] = group_time + group_mixed_time + (time.time() - group_clock)
        if group_more:
            group_more["ppc_group_mixed_time_sec"] = group_mixed_time         # (the pass over the redrawn rows: a part of the above)
        more.update(group_keys)
        more.update(group_more)
    keys["ppc_time_sec"] = time.time() - clock
    keys.update(more)                     # (PPC_KEYS in their order, then PPC_MIXED_KEYS, PPC_GROUP_KEYS, PPC_GROUP_MIXED_KEYS)
    return keys, arrays


def _ppc_mixed_report(mixed, names, posterior_keys, spec, y, kind):
    """The second half of --predictive_checks_redraw (_ppc_report): from the all-reduced counts and sums of the data
    replicated at the redrawn rows to the keys, the printed comparison and the arrays of <base>_ppc_mixed.npz.
    mixed: (redrawn [D] uint8, counts, obs_sums, this rank's draw statistics or None); posterior_keys: the posterior
    check's keys, which the line sets the mixed figures next to -- that comparison is the report."""
    redrawn, counts, obs_sums, stats_host = mixed
    summary = diagnostics.ppc_from_counts(counts, obs_sums, y, kind)
    chosen = [name for name in spec.part_names if name in names]
    keys = ppc_mixed_keys(summary, chosen, int(np.sum(redrawn != 0)), kind)
    pair = lambda key: "{} ({})".format(_fmt(keys["ppc_mixed_" + key]), _fmt(posterior_keys["ppc_" + key]))
    util.print_("    mixed predictive checks, {} redrawn from the conditional prior ({} elements), {} draws ({} left out) -- "
                "mixed (posterior): p-values mean {}, sd {}, min {}, max {}, deviance {}; replicated sd {}; PIT Kolmogorov "
                "distance {}, 90 % coverage {}".format(
                    ", ".join(chosen), keys["ppc_mixed_elements"], keys["ppc_mixed_draws"], keys["ppc_mixed_draws_left_out"],
                    pair("p_mean"), pair("p_sd"), pair("p_min"), pair("p_max"), pair("p_deviance"), pair("rep_sd"),
                    pair("pit_ks"), pair("coverage_90")))
    extreme = [name for name in diagnostics.PPC_STATISTICS if keys["ppc_mixed_p_" + name] is not None
               and not PPC_EXTREME[0] <= keys["ppc_mixed_p_" + name] <= PPC_EXTREME[1]]
    if extreme:
        util.print_("    WARNING: mixed predictive p-value outside [{}, {}] for: {} -- data sets replicated from NEW draws of {} "
                    "under the fitted hyperparameters (almost) never or (almost) always exceed the observed statistic; "
                    "customarily read as a misfit of that layer of the model, which the posterior check, at effects fitted "
                    "to the data, cannot see (a convention, not a derived threshold)".format(
                        PPC_EXTREME[0], PPC_EXTREME[1], ", ".join(extreme), ", ".join(chosen)))
    out = keys["ppc_mixed_pit_extreme_observations"]
    if out:
        util.print_("    {} of {} observations have a mixed PIT outside [{}, {}] -- outliers against a new draw of {}: {} "
                    "(the PIT values: <base>_ppc_mixed.npz)".format(
                        len(out), int(y.size), PPC_EXTREME[0], PPC_EXTREME[1], ", ".join(chosen), _shown(out, PPC_MIXED_SHOWN)))
    arrays = OrderedDict([("parts", np.asarray(chosen)), ("redrawn", np.asarray(redrawn, np.uint8)),
                          ("predictive_mean", summary.predictive_mean), ("predictive_sd", summary.predictive_sd),
                          ("pit", summary.pit), ("y", y),
                          ("draw_stats", stats_host if stats_host is not None else np.zeros((0, len(diagnostics.PPC_DRAW_COLUMNS)))),
                          ("model", np.asarray(spec.name))])
    return keys, arrays


def save_ppc_mixed(file_path_base, arrays):
    """`<base>_ppc_mixed.npz` (build-specific, --predictive_checks_redraw): `parts`, the parts redrawn, in part order, and
    `redrawn` [D] uint8, their elements; per observation `predictive_mean`, `predictive_sd` and `pit` [N] float64 of the
    MIXED predictive distribution and `y` [N]; `draw_stats` [R, 8] float64 as in <base>_ppc.npz, of the data sets replicated
    at the redrawn rows (zeros for a draw left out); `model`."""
    np.savez(file_path_base + "_ppc_mixed.npz", **arrays)


def save_ppc_groups(file_path_base, arrays):
    """`<base>_ppc_groups.npz` (build-specific, --predictive_checks_groups): `part`, the part whose elements are the groups;
    `groups` [G], their names; `group_of` [N] int32, every observation's group (-1: none); `n_obs` [G], the groups' sizes;
    per group `p_<T>`, `rep_<T>`, `obs_<T>` [G] float64 for T in diagnostics.PPC_STATISTICS as the whole-data keys define
    them, over the group's observations (NaN where not defined: an empty group, sd of a group of one or of Bernoulli data);
    the same arrays under `mixed_` with --predictive_checks_redraw; `y` [N]; `model`."""
    np.savez(file_path_base + "_ppc_groups.npz", **arrays)


def save_ppc(file_path_base, arrays):
    """`<base>_ppc.npz` (build-specific, --predictive_checks): per observation `predictive_mean`, `predictive_sd` and `pit`
    [N] float64 and `y` [N], the observations themselves; `draw_stats` [R, 8] float64, the per-draw sums of
    diagnostics.PPC_DRAW_COLUMNS (zeros for a draw left out); `model`, the model's name.  With --predictive_checks_redraw
    the mixed check's arrays wait under PPC_MIXED_ARRAYS and go to a file of their own (save_ppc_mixed): <base>_ppc.npz
    holds what it holds without the flag."""
    arrays = OrderedDict(arrays)
    mixed, grouped = arrays.pop(PPC_MIXED_ARRAYS, None), arrays.pop(PPC_GROUP_ARRAYS, None)
    np.savez(file_path_base + "_ppc.npz", **arrays)
    if mixed is not None:
        save_ppc_mixed(file_path_base, mixed)
    if grouped is not None:
        save_ppc_groups(file_path_base, grouped)


PSENS_ARRAYS = "psens/"              # where _convergence_report leaves the arrays of <base>_psens.npz
PSENS_SHOWN = 8                      # conflict elements the warning names
PSENS_KEYS = ("psens_draws", "psens_draws_left_out", "psens_chains", "psens_steps", "psens_elements_left_out",
              "psens_prior_max", "psens_prior_max_element", "psens_likelihood_max", "psens_likelihood_max_element",
              "psens_conflict_elements", "psens_weak_likelihood_elements", "psens_pareto_k_max", "psens_pareto_k_threshold",
              "psens_time_sec")


def check_sensitivity(flags):
    """--sensitivity_diagnostics against the job, before anything runs: check_predictive_checks' rule -- raises ValueError
    for a model without observations (neals_funnel), which has no likelihood to tell from its prior."""
    if getattr(flags, "sensitivity_diagnostics", False) and flags.model == "neals_funnel":
        raise ValueError("--sensitivity_diagnostics: neals_funnel has no observations, so there is no likelihood to "
                         "power-scale against the prior")


PSENS_SITES_ARRAYS = "psens_sites/"  # where _psens_report leaves the arrays of <base>_psens_sites.npz (--sensitivity_prior_parts)
PSENS_SITE_KEYS = ("psens_sites", "psens_sites_draws_left_out", "psens_sites_prior_max", "psens_sites_prior_max_element",
                   "psens_sites_conflict_elements", "psens_sites_weak_likelihood_elements", "psens_sites_pareto_k_max",
                   "psens_sites_joint_gap_max", "psens_sites_time_sec")


def prior_parts(flags):
    """The names --sensitivity_prior_parts gives, in the order given; [] without the flag."""
    text = getattr(flags, "sensitivity_prior_parts", "") or ""
    return text.split(",") if text else []


def check_sensitivity_sites(flags):
    """--sensitivity_prior_parts against the job, before anything runs -- raises ValueError for the flag without
    --sensitivity_diagnostics, an empty name, a duplicate and a name that is not a latent part of the model."""
    names = prior_parts(flags)
    if not names:
        return
    if not getattr(flags, "sensitivity_diagnostics", False):
        raise ValueError("--sensitivity_prior_parts is read with --sensitivity_diagnostics only")
    if "" in names:
        raise ValueError("--sensitivity_prior_parts: an empty name in {!r}".format(flags.sensitivity_prior_parts))
    if len(set(names)) != len(names):
        raise ValueError("--sensitivity_prior_parts: {} is named twice".format(
            ", ".join(sorted({n for n in names if names.count(n) > 1}))))
    parts = models.spec_by_name(flags.model, dataset=getattr(flags, "dataset", None)).part_names
    unknown = [n for n in names if n not in parts]
    if unknown:
        raise ValueError("--sensitivity_prior_parts: {} is no latent part of {}; its parts: {}".format(
            ", ".join(unknown), flags.model, ", ".join(parts)))


def _psens_null(why, flags=None):
    """Every key of the sensitivity report, and of --sensitivity_prior_parts where set, as null; one message says why."""
    return _null_keys("power-scaling sensitivity", why, PSENS_KEYS + (PSENS_SITE_KEYS if prior_parts(flags) else ()))


def psens_keys(summary, names, pareto_k, R, left_out, n_chains, n_steps):
    """The JSON keys of the sensitivity report (all but psens_time_sec) from a diagnostics.PsensSummary, the elements'
    names, the four k-hat of the power-scaled ratios, the draws taken `R` and how many of them were left out; pure numpy."""
    used = int(R) - int(left_out)
    p_max, p_at = _nan_max(summary.prior)
    l_max, l_at = _nan_max(summary.likelihood)
    k_max, _ = _nan_max(pareto_k)
    return OrderedDict([
        ("psens_draws", used), ("psens_draws_left_out", int(left_out)), ("psens_chains", int(n_chains)),
        ("psens_steps", int(n_steps)), ("psens_elements_left_out", int(summary.constant)),
        ("psens_prior_max", _finite_or_none(p_max)), ("psens_prior_max_element", names[p_at] if p_at >= 0 else None),
        ("psens_likelihood_max", _finite_or_none(l_max)), ("psens_likelihood_max_element", names[l_at] if l_at >= 0 else None),
        ("psens_conflict_elements", [names[i] for i in summary.conflict]),
        ("psens_weak_likelihood_elements", [names[i] for i in summary.weak_likelihood]),
        ("psens_pareto_k_max", _finite_or_none(k_max)),
        ("psens_pareto_k_threshold", _finite_or_none(diagnostics.pareto_k_threshold(used)))])


def site_prior_split(draws, site_table, selected):
    """(log_prior_selected, log_prior_rest) [R] float64 device tensors for centred draws [steps, chains, D] on the GPU, a
    diagnostics.DeviceSiteTable and `selected` [P] bool: diagnostics.site_logprior with groups = parts, the steps walked
    in blocks whose [rows, P] float64 output stays within LOO_CHUNK_BYTES, and the chosen parts' columns added in
    ascending part order (the others' likewise): sequential float64 additions on the device, row by row -- the blocks
    compose bit for bit."""
    import torch
    n_steps, k, _ = (int(v) for v in draws.shape)
    P = site_table.P
    per_block = max(1, LOO_CHUNK_BYTES // (8 * P * k))
    sel, rest = (torch.zeros(n_steps * k, dtype=torch.float64, device=draws.device) for _ in range(2))
    for s0 in range(0, n_steps, per_block):
        s1 = min(n_steps, s0 + per_block)
        by_part = diagnostics.site_logprior(draws[s0:s1], site_table)[0]
        for p in range(P):
            (sel if selected[p] else rest)[s0 * k:s1 * k] += by_part[:, p]
    return sel, rest


def _psens_sites_report(names, draws, spec, log_prior, logp_const, log_lik, left, order, values, centre):
    """--sensitivity_prior_parts: the second report of _psens_report, on its draws, its left-out mask, its log-likelihood
    and its element order -- the prior that is power-scaled is the sum of the named parts' site densities
    (site_prior_split) instead of the joint one.  A draw whose selected prior is not finite joins the left-out draws of
    this report only.  diagnostics.powerscale_lw, cjs_sums and psens_summary as there: no second definition.
    psens_sites_joint_gap_max: the largest |sum of ALL parts - (log_prior + logp_const)| over the draws kept -- how far the
    two routes to the prior are apart (the float32 rounding of the engine's log joint); written, never warned about.
    Returns (JSON keys, arrays of <base>_psens_sites.npz)."""
    import torch
    clock = time.time()
    dev = draws.device
    selected = np.asarray([name in names for name in spec.part_names])
    site_table = diagnostics.upload_site_table(spec.site_table(), spec.D, dev)
    sel, rest = site_prior_split(draws, site_table, selected)
    left = left | ~torch.isfinite(sel)
    kept = ~left
    gap = torch.where(kept, ((sel + rest) - (log_prior + logp_const)).abs(), torch.zeros_like(sel))
    gap = float(gap.max().item()) if bool(kept.any().item()) else float("nan")
    out8, lw = diagnostics.powerscale_lw(sel, log_lik, left)
    summary = diagnostics.psens_summary(diagnostics.cjs_sums(values, order, lw, centre).cpu().numpy())
    del lw
    elements = element_names(spec)
    pareto_k = out8.cpu().numpy()[:2, 1]                       # (the prior rows: the likelihood's are the first report's)
    p_max, p_at = _nan_max(summary.prior)
    chosen = [name for name in spec.part_names if name in names]
    keys = OrderedDict([
        ("psens_sites", chosen), ("psens_sites_draws_left_out", int(left.sum().item())),
        ("psens_sites_prior_max", _finite_or_none(p_max)), ("psens_sites_prior_max_element", elements[p_at] if p_at >= 0 else None),
        ("psens_sites_conflict_elements", [elements[i] for i in summary.conflict]),
        ("psens_sites_weak_likelihood_elements", [elements[i] for i in summary.weak_likelihood]),
        ("psens_sites_pareto_k_max", _finite_or_none(_nan_max(pareto_k)[0])),
        ("psens_sites_joint_gap_max", _finite_or_none(gap))])
    util.print_("    power-scaling sensitivity to the priors of {} alone: prior max {} ({}); {} prior-data conflict(s), {} "
                "element(s) with a weak likelihood or a strong prior".format(
                    ", ".join(chosen), _fmt(keys["psens_sites_prior_max"]), keys["psens_sites_prior_max_element"],
                    len(keys["psens_sites_conflict_elements"]), len(keys["psens_sites_weak_likelihood_elements"])))
    if keys["psens_sites_conflict_elements"]:
        shown = keys["psens_sites_conflict_elements"][:PSENS_SHOWN]
        util.print_("    WARNING: prior-data conflict (prior and likelihood sensitivity above {}) with the priors of {} for: {}{} "
                    "-- these priors and the data pull these marginals apart; no reparameterisation repairs that (all of "
                    "them: <base>_psens_sites.npz)".format(
                        diagnostics.PSENS_THRESHOLD, ", ".join(chosen), ", ".join(shown),
                        " and {} more".format(len(keys["psens_sites_conflict_elements"]) - len(shown))
                        if len(keys["psens_sites_conflict_elements"]) > len(shown) else ""))
    arrays = OrderedDict([("parts", np.asarray(spec.part_names)), ("selected", selected),
                          ("log_prior_selected", sel.cpu().numpy()), ("log_prior_rest", rest.cpu().numpy()),
                          ("left_out", left.cpu().numpy()), ("pareto_k", pareto_k)])
    _by_part(spec, arrays, (("prior", summary.prior), ("mean_shift_prior", summary.mean_shift_prior),
                            ("sd_ratio_prior", summary.sd_ratio_prior)))
    keys["psens_sites_time_sec"] = time.time() - clock
    return keys, arrays


def _psens_report(trace, k, spec, flags, pooled_mean=None, side=None):
    """--sensitivity_diagnostics: how much of each posterior marginal comes from the prior, how much from the data?
    Power-scaling sensitivity (Kallioinen, Paananen, Buerkner, Vehtari 2023; priorsense, ArviZ psens) over the draws the
    predictive report takes (select_draws: the leading `k` chains of the device trace, the chains split R-hat covers),
    centred.  The likelihood of a draw is joint_loglik's, in the observation tiles of the predictive report; the prior is
    the centred log joint at the same draws minus that -- the joint density of ALL latent sites, the hierarchical layers
    included -- from an engine of the report's own set to CP, so that nothing of the run's state is touched.  A draw the
    log-likelihood masks or whose log joint is not finite is left out and counted.  The prior and the likelihood are raised
    to 1 / (1 + delta) and 1 + delta (diagnostics.powerscale_lw: Pareto-smoothed weights), every element's pooled draws are
    ordered (diagnostics.element_order) and the weighted ECDFs folded (diagnostics.cjs_sums, about `pooled_mean`); the
    statistics are diagnostics.psens_summary's.  The order of an element's draws needs them on one device: a sharded job
    (world size > 1) writes null, says so once, and enters no collective -- the rule of the rank reports.  delta is fixed;
    no power-scaling sequence.  The choice of prior sites is --sensitivity_prior_parts: a second report on the same draws,
    mask, likelihood and order whose prior is the named parts' own (_psens_sites_report); its keys join these, its arrays
    are left in `side` under PSENS_SITES_ARRAYS, and it changes nothing of the first report.  Its keys are null whenever
    these are.  Returns (JSON keys, arrays of <base>_psens.npz or None)."""
    import torch
    if parallel.world()[1] > 1:
        return _psens_null("the chains of a sharded job are on several devices (the order of an element's pooled draws "
                           "needs them on one)", flags), None
    clock = time.time()
    why, steps, draws = select_draws(trace, k, k, flags)
    if why:
        return _psens_null(why, flags), None
    k, D, dev, R = int(k), int(trace.shape[2]), trace.device, len(steps) * int(k)
    table = diagnostics.upload_table(spec.observation_table(), D, dev)
    rows = loo_tile_rows(table.N, R)
    ll_buffer = torch.empty(rows, R, dtype=torch.float32, device=dev)
    log_lik, mask = joint_loglik(draws, table, ll_buffer, rows)
    del ll_buffer
    eng = _centred_engine(spec, dev)
    log_joint = eng.logp_grad(draws.reshape(R, D), which=0)[0].to(torch.float64)
    logp_const = float(eng.logp_const(0))
    del eng
    log_prior = log_joint - log_lik
    left = (mask != 0) | ~torch.isfinite(log_prior)
    left_out = int(left.sum().item())
    out8, lw = diagnostics.powerscale_lw(log_prior, log_lik, left)
    order, values = diagnostics.element_order(draws)
    centre = np.zeros(D) if pooled_mean is None else np.asarray(pooled_mean, np.float64).reshape(D)
    centre = np.nan_to_num(centre, nan=0.0, posinf=0.0, neginf=0.0).astype(np.float32)
    centre = torch.as_tensor(centre, device=dev)
    sums = diagnostics.cjs_sums(values, order, lw, centre).cpu().numpy()
    del lw
    summary = diagnostics.psens_summary(sums)
    names = element_names(spec)
    pareto_k = out8.cpu().numpy()[:, 1]
    keys = psens_keys(summary, names, pareto_k, R, left_out, k, len(steps))
    util.print_("    power-scaling sensitivity over {} draws ({} step(s) of {} chains, {} left out), {} elements ({} constant): "
                "prior max {} ({}), likelihood max {} ({}); {} prior-data conflict(s), {} element(s) with a weak likelihood "
                "or a strong prior".format(
                    keys["psens_draws"], len(steps), k, left_out, D, keys["psens_elements_left_out"],
                    _fmt(keys["psens_prior_max"]), keys["psens_prior_max_element"], _fmt(keys["psens_likelihood_max"]),
                    keys["psens_likelihood_max_element"], len(keys["psens_conflict_elements"]),
                    len(keys["psens_weak_likelihood_elements"])))
    if keys["psens_conflict_elements"]:
        shown = keys["psens_conflict_elements"][:PSENS_SHOWN]
        util.print_("    WARNING: prior-data conflict (prior and likelihood sensitivity above {}) for: {}{} -- prior and data "
                    "pull these marginals apart; no reparameterisation repairs that (all of them: <base>_psens.npz)".format(
                        diagnostics.PSENS_THRESHOLD, ", ".join(shown),
                        " and {} more".format(len(keys["psens_conflict_elements"]) - len(shown))
                        if len(keys["psens_conflict_elements"]) > len(shown) else ""))
    threshold = keys["psens_pareto_k_threshold"]
    with np.errstate(invalid="ignore"):
        high = int(np.sum(~(pareto_k <= threshold))) if threshold is not None else int(np.sum(~np.isfinite(pareto_k)))
    if high:
        util.print_("    WARNING: Pareto k-hat above {} for {} of the 4 power-scaled weight rows (not fitted ones included): "
                    "their sensitivities are unreliable".format(_fmt(threshold), high))
    arrays = OrderedDict([("elements", np.asarray(names))] + data_tail(table.y_host, spec)
                         + [("pareto_k", pareto_k), ("log_prior", log_prior.cpu().numpy()),
                            ("log_likelihood", log_lik.cpu().numpy()), ("left_out", left.cpu().numpy())])
    _by_part(spec, arrays, (("prior", summary.prior), ("likelihood", summary.likelihood),
                            ("mean_shift_prior", summary.mean_shift_prior),
                            ("mean_shift_likelihood", summary.mean_shift_likelihood),
                            ("sd_ratio_prior", summary.sd_ratio_prior), ("sd_ratio_likelihood", summary.sd_ratio_likelihood)))
    names_chosen = prior_parts(flags)
    if names_chosen:
        site_keys, site_arrays = _psens_sites_report(names_chosen, draws, spec, log_prior, logp_const, log_lik, left, order,
                                                     values, centre)
        keys.update(site_keys)
        if side is not None:
            side[PSENS_SITES_ARRAYS] = site_arrays
    del order, values
    keys["psens_time_sec"] = time.time() - clock
    return keys, arrays


def save_psens(file_path_base, arrays):
    """`<base>_psens.npz` (build-specific, --sensitivity_diagnostics): `elements`, the elements' names in trace order; `y`,
    the observations; `model`; `pareto_k` [4], the k-hat of the power-scaled ratios (prior lower, prior upper, likelihood
    lower, likelihood upper); `log_prior`, `log_likelihood` [R] float64 of the draws taken (without the constants the
    density omits) and `left_out` [R]; per latent part `prior/<part>`, `likelihood/<part>` (the sensitivities, NaN for a
    constant element), `mean_shift_prior/<part>`, `mean_shift_likelihood/<part>`, `sd_ratio_prior/<part>` and
    `sd_ratio_likelihood/<part>` (the upper row's weighted mean shift in pooled sd and its sd ratio)."""
    np.savez(file_path_base + "_psens.npz", **arrays)


def save_psens_sites(file_path_base, arrays):
    """`<base>_psens_sites.npz` (build-specific, --sensitivity_prior_parts): `parts`, the model's latent parts in trace order,
    and `selected` [P] bool, the ones whose priors were power-scaled; `log_prior_selected`, `log_prior_rest` [R] float64 of
    the draws _psens.npz holds: the sums of the chosen parts' site log densities and of the others' (normalisers included);
    `left_out` [R] (the first report's and the draws whose selected prior is not finite); `pareto_k` [2], the k-hat of the
    prior's power-scaled ratios (lower, upper); per latent part `prior/<part>`, `mean_shift_prior/<part>` and
    `sd_ratio_prior/<part>` as in _psens.npz, for the chosen priors."""
    np.savez(file_path_base + "_psens_sites.npz", **arrays)


PRIOR_ARRAYS = "prior/"              # where _convergence_report leaves the arrays of <base>_prior.npz
PRIOR_SEED = 0x5052494F              # the report's own seed constant, as PPC_SEED is the posterior checks'
PRIOR_KEYS = ("prior_draws", "prior_draws_left_out", "prior_observations", "prior_p_mean", "prior_p_sd", "prior_p_min",
              "prior_p_max", "prior_p_deviance", "prior_rep_mean_q05", "prior_rep_mean_q50", "prior_rep_mean_q95",
              "prior_rep_sd_q05", "prior_rep_sd_q50", "prior_rep_sd_q95", "prior_rep_min_q05", "prior_rep_max_q95",
              "prior_obs_mean", "prior_obs_sd", "prior_contraction_min", "prior_contraction_min_element",
              "prior_z_score_max_abs", "prior_z_score_max_element", "prior_elements_left_out", "prior_time_sec")


def check_prior_predictive(flags):
    """--prior_predictive_checks against the job, before anything runs: check_predictive_checks' rule -- raises ValueError
    for a model without observations (neals_funnel), whose prior predicts no data."""
    if getattr(flags, "prior_predictive_checks", False) and flags.model == "neals_funnel":
        raise ValueError("--prior_predictive_checks: neals_funnel has no observations, so there is no data for its prior to "
                         "predict")


def _prior_null(why):
    """Every key of the prior predictive checks as null, with the one message that says why."""
    return _null_keys("prior predictive checks", why, PRIOR_KEYS)


def prior_keys(summary, predictive, contraction, names):
    """The JSON keys of the prior predictive checks (all but prior_time_sec) from a diagnostics.PpcSummary of replicated
    data at PRIOR draws, the PriorPredictiveSummary of the same draw statistics and a PriorContractionSummary; `names`:
    element_names.  Pure Python."""
    num = lambda v: None if v is None else _finite_or_none(v)
    keys = OrderedDict([("prior_draws", int(summary.draws_used)), ("prior_draws_left_out", int(summary.draws_left_out)),
                        ("prior_observations", int(summary.observations))])
    for name in diagnostics.PPC_STATISTICS:
        keys["prior_p_" + name] = num(summary.p[name])
    q = {name: v if v is not None else (None, None, None) for name, v in predictive.quantiles.items()}
    keys.update([("prior_rep_mean_q05", num(q["mean"][0])), ("prior_rep_mean_q50", num(q["mean"][1])),
                 ("prior_rep_mean_q95", num(q["mean"][2])), ("prior_rep_sd_q05", num(q["sd"][0])),
                 ("prior_rep_sd_q50", num(q["sd"][1])), ("prior_rep_sd_q95", num(q["sd"][2])),
                 ("prior_rep_min_q05", num(q["min"][0])), ("prior_rep_max_q95", num(q["max"][2])),
                 ("prior_obs_mean", num(summary.obs["mean"])), ("prior_obs_sd", num(summary.obs["sd"]))])
    least, at = _nan_max(-np.asarray(contraction.contraction, np.float64))
    far, at_z = _nan_max(np.abs(np.asarray(contraction.z_score, np.float64)))
    keys.update([("prior_contraction_min", _finite_or_none(-least)), ("prior_contraction_min_element", names[at] if at >= 0 else None),
                 ("prior_z_score_max_abs", _finite_or_none(far)), ("prior_z_score_max_element", names[at_z] if at_z >= 0 else None),
                 ("prior_elements_left_out", int(contraction.left_out))])
    return keys


def _prior_report(spec, flags, dev, post_mean, post_sd):
    """--prior_predictive_checks: what does the model say BEFORE it has seen data, and how far did the data move it?  The
    first step of the Bayesian workflow (Gabry, Simpson, Vehtari, Betancourt, Gelman 2019; Gelman et al. 2020).
    R = --loo_draws ancestral draws from the model's latent site table (diagnostics.site_prior_draws), keyed by a seed
    derived from --seed and PRIOR_SEED; they need no device trace.  A draw one of whose elements is not finite (which
    predictive_check masks) or could not be drawn is left out and counted.
      * The predictive side: one replicated data set per draw at the observed covariates (diagnostics.predictive_check on
        the draws as a [1, R, D] trace, under the next seed -- the draws' own would hand element d and observation d the
        same Philox words), in _ppc_report's tiles of observations; diagnostics.ppc_summary says where the observed mean,
        sd, min, max and deviance sit among the prior-predicted ones, diagnostics.prior_predictive_summary gives the 5 %,
        50 % and 95 % points of the replicated statistics.
      * The contraction side: every element's kept draws are ordered (diagnostics.element_order), its 5 %, 50 % and 95 %
        points gathered on the device and set against `post_mean` and `post_sd`, the pooled posterior moments split R-hat
        has already all-reduced (diagnostics.prior_contraction_summary: contraction and z-score on a QUANTILE scale of the
        prior against a MOMENT scale of the posterior).
    No warning and no threshold: none can be derived for a prior predictive p-value -- a weakly informative prior is MEANT
    to be wider than the data, so p-values near 0 or 1 for min and max are the expected reading, not a finding.  No prior
    draws at new covariates, no simulation-based calibration, no user-defined statistic.  Rank 0 of a sharded job runs it
    alone and enters no collective (the other ranks return nothing).  Returns (JSON keys, arrays of <base>_prior.npz or None)."""
    if parallel.world()[0] != 0:
        return {}, None
    clock = time.time()
    D = int(spec.D)
    if D > diagnostics.LOGLIK_MAX_D:
        return _prior_null("the model has more than {} elements".format(diagnostics.LOGLIK_MAX_D)), None
    R = int(min(max(int(getattr(flags, "loo_draws", 65536)), 1), diagnostics.SITE_MAX_DRAWS))
    seed = derived_seed(flags.seed, PRIOR_SEED)
    site = diagnostics.upload_site_table(spec.site_table(), D, dev)
    x, undrawn = diagnostics.site_prior_draws(site, R, seed=seed)
    table = diagnostics.upload_table(spec.observation_table(), D, dev)
    N, kind, y = table.N, table.kind, table.y_host
    stats, sums, mask = replicate_tiles(x[None], table, next_seed(seed), budget=LOO_CHUNK_BYTES)      # [1, R, D]: one step, R chains
    left = (mask != 0) | (undrawn != 0)                                                  # (an undrawn element is NaN: masked too)
    stats_host, obs_sums, left_host = _lib.host64(stats), _lib.host64(sums), left.cpu().numpy()
    summary = diagnostics.ppc_summary(stats_host, obs_sums, y, kind, left_host)
    predictive = diagnostics.prior_predictive_summary(stats_host, y, kind, left_host)
    kept = int(summary.draws_used)
    quantiles = np.full((D, len(diagnostics.PRIOR_QUANTILES)), np.nan)
    if kept > 0:
        _, values = diagnostics.element_order(x[~left][None].contiguous(), want_sorted=True)
        at = [diagnostics.order_statistic_index(p, kept) for p in diagnostics.PRIOR_QUANTILES]
        quantiles = _lib.host64(values[:, at])
        del values
    nan = np.full(D, np.nan)
    contraction = diagnostics.prior_contraction_summary(
        quantiles[:, 0], quantiles[:, 1], quantiles[:, 2], nan if post_mean is None else np.asarray(post_mean, np.float64).reshape(D),
        nan if post_sd is None else np.asarray(post_sd, np.float64).reshape(D))
    names = element_names(spec)
    keys = prior_keys(summary, predictive, contraction, names)
    util.print_("    prior predictive checks over {} observations, {} prior draws ({} left out): the observed mean sits at "
                "p = {} and the observed sd at p = {} among the prior-predicted ones (min {}, max {}, deviance {}); prior "
                "90 % band of the replicated mean {} ... {} against {} observed, of the replicated sd {} ... {} against {} "
                "observed (no threshold: a weak prior is meant to be wider than the data)".format(
                    N, keys["prior_draws"], keys["prior_draws_left_out"], _fmt(keys["prior_p_mean"]), _fmt(keys["prior_p_sd"]),
                    _fmt(keys["prior_p_min"]), _fmt(keys["prior_p_max"]), _fmt(keys["prior_p_deviance"]),
                    _fmt(keys["prior_rep_mean_q05"]), _fmt(keys["prior_rep_mean_q95"]), _fmt(keys["prior_obs_mean"]),
                    _fmt(keys["prior_rep_sd_q05"]), _fmt(keys["prior_rep_sd_q95"]), _fmt(keys["prior_obs_sd"])))
    util.print_("    prior to posterior over {} elements ({} left out): least contraction {} ({}), largest |z-score| {} ({}) "
                "-- quantile scale of the prior, moment scale of the posterior".format(
                    D, keys["prior_elements_left_out"], _fmt(keys["prior_contraction_min"]), keys["prior_contraction_min_element"],
                    _fmt(keys["prior_z_score_max_abs"]), keys["prior_z_score_max_element"]))
    arrays = OrderedDict([("elements", np.asarray(names))] + data_tail(y, spec)
                         + [("draw_stats", stats_host), ("left_out", left_host),
                            ("predictive_mean", summary.predictive_mean), ("predictive_sd", summary.predictive_sd)])
    _by_part(spec, arrays, (("prior_q05", quantiles[:, 0]), ("prior_median", quantiles[:, 1]), ("prior_q95", quantiles[:, 2]),
                            ("contraction", contraction.contraction), ("z_score", contraction.z_score)))
    keys["prior_time_sec"] = time.time() - clock
    return keys, arrays


def save_prior(file_path_base, arrays):
    """`<base>_prior.npz` (build-specific, --prior_predictive_checks): `elements`, the elements' names in trace order; `y`
    [N], the observations; `model`; `draw_stats` [R, 8] float64, the per-draw sums of diagnostics.PPC_DRAW_COLUMNS of the data
    sets replicated at the PRIOR draws (zeros for a draw left out) and `left_out` [R]; `predictive_mean`, `predictive_sd`
    [N], the prior predictive mean and sd of every observation; per latent part `prior_q05/<part>`, `prior_median/<part>`,
    `prior_q95/<part>` (order statistics of the kept draws), `contraction/<part>` and `z_score/<part>` (NaN for an element
    left out)."""
    np.savez(file_path_base + "_prior.npz", **arrays)


def _fit_chains(trace, k, workspace_bytes):
    """The largest of k, k/2, k/4, ... leading chains whose z-score trace and the `workspace_bytes(S, k, D)` next to it
    fit the free device memory."""
    import torch
    S, _, D = (int(v) for v in trace.shape)
    free = torch.cuda.mem_get_info(trace.device)[0]
    while k > 0 and S * k * D * 4 + workspace_bytes(S, k, D) > free:
        k //= 2
    return k


def _rank_fit_chains(trace, k):
    """_fit_chains for the rank report: the z-score trace and the rank workspace."""
    return _fit_chains(trace, k, lambda S, k, D: diagnostics.rank_workspace_bytes(S, k, D, True))


def _rank_report(trace, k, spec, arrays, by_part):
    """--rank_normalized_rhat: the rank-normalised, folded split R-hat over the leading k chains of the device trace (fewer
    where z and the workspace do not fit: the count is reported) and the pooled median / 5 % / 95 % quantiles, into
    `arrays`; returns the five rank_rhat_* JSON keys.  The pooled ranks need every draw on one device: a sharded job
    (world size > 1) writes null, says so once, and enters no collective."""
    keys = {"rank_rhat_max": None, "rank_rhat_bulk_max": None, "rank_rhat_tail_max": None, "rank_rhat_chains": 0,
            "rank_rhat_time_sec": None}
    if parallel.world()[1] > 1:
        util.print_("    rank-normalised R-hat: skipped, the chains of a sharded job are on several devices "
                    "(the pooled ranks need all draws on one)")
        return keys
    clock = time.time()
    k = _rank_fit_chains(trace, k) if k > 0 else 0
    if k <= 0:
        util.print_("    rank-normalised R-hat: no chains to rank")
        return keys
    r = diagnostics.rank_rhat(trace[:, :k])
    by_part(arrays, (("rank_rhat_bulk", r.bulk), ("rank_rhat_tail", r.tail), ("posterior_median", r.median),
                     ("posterior_q05", r.q05), ("posterior_q95", r.q95)))
    top, at = _nan_max(r.rhat)
    bulk_max, tail_max = _nan_max(r.bulk)[0], _nan_max(r.tail)[0]
    util.print_("    rank-normalised split R-hat over {} chains: max {:.4f} (element {}; bulk {:.4f}, tail {:.4f})".format(
        k, top, at, bulk_max, tail_max))
    if np.nan_to_num(top) > RHAT_WARN:
        util.print_("    WARNING: rank-normalised R-hat above {}: the chains have not converged to one distribution "
                    "(the elements: <base>_rhat.npz)".format(RHAT_WARN))
    keys.update(rank_rhat_max=_finite_or_none(top), rank_rhat_bulk_max=_finite_or_none(bulk_max),
                rank_rhat_tail_max=_finite_or_none(tail_max), rank_rhat_chains=k, rank_rhat_time_sec=time.time() - clock)
    return keys


def nested_warn_level(K, M):
    """The B / W above which nested R-hat over K superchains of M chains is reported as not converged: the stationary
    floor 1 / M with three standard deviations of B's sampling noise over K superchains, sqrt(2 / (K - 1)) of itself, plus
    the share of non-stationary variance RHAT_WARN stands for.  K may be an array; NaN where K < 2."""
    K = np.asarray(K, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(K >= 2, (1.0 + 3.0 * np.sqrt(2.0 / (K - 1.0))) / M + (RHAT_WARN ** 2 - 1.0), np.nan)


def _nested_report(trace, moments, M, dev, arrays, by_part):
    """--superchain_size M >= 2: nested R-hat (diagnostics.nested_fold -> nested_rhat_from_sums) over ALL chains of the job,
    from the per-chain moments of the whole trace or, in a streaming run, from the in-kernel statistics (`moments`); and
    its profile over the recorded steps, one draw per chain (diagnostics.nested_step_sums), over the whole superchains
    among the chains whose trace is on the device.  Both sets of sums are additive over superchains and every rank holds
    whole superchains: a sharded job reports real numbers.  Fills `arrays`, returns the nine JSON keys.
    (A collective when ws > 1: every rank calls it.)"""
    clock = time.time()
    S, C_local, D = (int(v) for v in trace.shape)
    if moments is not None:
        mean, var = moments
    else:
        mean, var = (m[0] for m in diagnostics.split_moments(trace, split=False))
    n_local = int(mean.shape[0])
    local = diagnostics.nested_fold(mean, None if S == 1 else var, M)
    sums, n_chains = _reduced([local, float(n_local)], dev)
    whole, n_chains = diagnostics.nested_rhat_from_sums(sums), int(round(float(n_chains)))
    top, at = _nan_max(whole.rhat)
    by_part(arrays, (("nested_rhat", whole.rhat),))
    counted = int(whole.superchains.min()) if D else 0
    left_out = int(whole.left_out.max()) if D else 0
    floor = float(np.sqrt(1.0 + 1.0 / M))
    util.print_("    nested R-hat over {} superchains of {} chains: max {:.4f} (element {}; stationary floor {:.4f}{})".format(
        counted, M, top, at, floor, "; {} superchain(s) left out, not finite".format(left_out) if left_out else ""))
    with np.errstate(invalid="ignore"):
        alarm = bool(np.any(whole.excess > nested_warn_level(whole.superchains, M)))

    # the profile: one draw per chain at every recorded step, over the leading whole superchains of the device trace
    kk = (C_local // M) * M
    sums4, n_super = _reduced([diagnostics.nested_step_sums(trace[:, :kk], M) if kk > 0 else np.zeros((4, S, D)),
                               float(kk // M)], dev)
    n_super = int(round(float(n_super)))
    first = last = float("nan")
    if n_super >= 2 and S > 0:
        by_step = diagnostics.nested_rhat_by_step(sums4)                       # [S, D]: not saved (tens of MB for a kept trace)
        ok = np.isfinite(by_step)
        arrays["nested_rhat_by_step_element"] = np.where(ok.any(axis=1), np.where(ok, by_step, -np.inf).argmax(axis=1), -1)
        arrays["nested_rhat_by_step"] = np.where(ok.any(axis=1), np.where(ok, by_step, -np.inf).max(axis=1), np.nan)
        first, last = float(arrays["nested_rhat_by_step"][0]), float(arrays["nested_rhat_by_step"][-1])
        util.print_("    nested R-hat by step over {} superchains (one draw per chain): first {:.4f}, last {:.4f}".format(
            n_super, first, last))
        with np.errstate(invalid="ignore"):
            alarm = alarm or bool(np.any(by_step[0] ** 2 - 1.0 > nested_warn_level(sums4[0, 0], M)))
    else:
        util.print_("    nested R-hat by step: fewer than two whole superchains have their trace on the device")
    if alarm:
        util.print_("    WARNING: nested R-hat above its stationary level (B / W > (1 + 3 sqrt(2 / (K - 1))) / M + {:.4f}): the "
                    "superchains have not forgotten their starting points (the elements: <base>_rhat.npz)".format(
                        RHAT_WARN ** 2 - 1.0))
    return {"nested_rhat_max": _finite_or_none(top), "nested_rhat_superchains": counted, "nested_rhat_superchain_size": M,
            "nested_rhat_chains": n_chains, "nested_rhat_floor": floor, "nested_rhat_left_out": left_out,
            "nested_rhat_first_step_max": _finite_or_none(first), "nested_rhat_last_step_max": _finite_or_none(last),
            "nested_rhat_time_sec": time.time() - clock}


ESS_PER_CHAIN_WARN = 100    # Stan's rule: bulk- and tail-ESS of at least 100 per chain


def _bulk_tail_fit_chains(trace, k):
    """_fit_chains for the bulk / tail report: the z-score trace and the larger of the rank workspace and the ESS
    workspace (they are not alive together)."""
    return _fit_chains(trace, k, lambda S, k, D: max(diagnostics.rank_workspace_bytes(S, k, D, False),
                                                     diagnostics.ess_multichain_workspace_bytes(S, k, D, True)))


def _bulk_tail_report(trace, k, spec, arrays, by_part):
    """--bulk_tail_ess: the multi-chain bulk-ESS, tail-ESS, ESS of the mean and its Monte-Carlo standard error over the
    leading k chains of the device trace (fewer where the z trace and the workspaces do not fit: the count is reported),
    into `arrays`; returns the six JSON keys.  Like the pooled ranks, the pooled autocovariances need every draw on one
    device: a sharded job (world size > 1) writes null, says so once, and enters no collective.  The reference's ess_min
    (per chain) is not touched."""
    keys = {"ess_bulk_min": None, "ess_tail_min": None, "ess_mean_min": None, "mcse_mean_over_sd_max": None,
            "bulk_tail_ess_chains": 0, "bulk_tail_ess_time_sec": None}
    if parallel.world()[1] > 1:
        util.print_("    bulk / tail ESS: skipped, the chains of a sharded job are on several devices "
                    "(the pooled ranks and autocovariances need all draws on one)")
        return keys
    clock = time.time()
    k = _bulk_tail_fit_chains(trace, k) if k > 0 else 0
    if k <= 0:
        util.print_("    bulk / tail ESS: no chains to pool")
        return keys
    r = diagnostics.bulk_tail_ess(trace[:, :k])
    by_part(arrays, (("ess_bulk", r.bulk), ("ess_tail", r.tail), ("ess_mean", r.mean), ("mcse_mean", r.mcse_mean)))

    def nan_min(x):
        return -_nan_max(-np.asarray(x, np.float64))[0]
    bulk_min, tail_min, mean_min = nan_min(r.bulk), nan_min(r.tail), nan_min(r.mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_max = _nan_max(r.mcse_mean / r.sd)[0]
    util.print_("    multi-chain ESS over {} chains: bulk min {:.1f}, tail min {:.1f}, mean min {:.1f}; "
                "largest MCSE of a mean {:.4f} posterior sd".format(k, bulk_min, tail_min, mean_min, rel_max))
    low = [v for v in (bulk_min, tail_min) if np.isfinite(v)]
    if low and min(low) < ESS_PER_CHAIN_WARN * k:
        util.print_("    WARNING: bulk- or tail-ESS below {} per chain: the posterior summaries of these elements are not "
                    "reliable yet (the elements: <base>_rhat.npz)".format(ESS_PER_CHAIN_WARN))
    keys.update(ess_bulk_min=_finite_or_none(bulk_min), ess_tail_min=_finite_or_none(tail_min),
                ess_mean_min=_finite_or_none(mean_min), mcse_mean_over_sd_max=_finite_or_none(rel_max),
                bulk_tail_ess_chains=k, bulk_tail_ess_time_sec=time.time() - clock)
    return keys


def save_energy(file_path_base, arrays):
    """`<base>_energy.npz` (build-specific, --energy_diagnostics): `steps`, the probed recorded steps with -1 for the final
    state; `energy_error` [len(steps), C] float32, the energy error of every probed trajectory (NaN where a chain has no
    trace on the device; `energy_error_1`: the second inner kernel of --method=i); and of up to ENERGY_WHERE_MAX divergent
    trajectories the centred state they started from, per latent part (`divergent_where/<part>`), with `divergent_chain`,
    `divergent_step` and `divergent_kernel`."""
    np.savez(file_path_base + "_energy.npz", **arrays)


def save_trajectory(file_path_base, arrays):
    """`<base>_trajectory.npz` (build-specific, --trajectory_profile): `leapfrogs` = 1 ... LMAX; per latent part
    `esjd/<part>` [LMAX, *event], the Metropolis-weighted expected squared jump distance of every element in units of its
    pooled posterior variance for a trajectory of that many leapfrog steps; `accept_prob` and `divergence_rate` [LMAX].  The
    second inner kernel of --method=i: `esjd_1/<part>`, `accept_prob_1`, `divergence_rate_1`."""
    np.savez(file_path_base + "_trajectory.npz", **arrays)


def save_geometry(file_path_base, arrays):
    """`<base>_geometry.npz` (build-specific, --geometry_diagnostics): `elements`, one name per element; in the sampler's
    coordinates `mean`, `sd` [D], `correlation` [D, D] (NaN at the elements left out), `eigenvalues` (ascending, of the
    correlation matrix over the elements kept), `step_scaled_eigenvalues` (of the covariance scaled by the run's base steps),
    `scale_coupling` [D, D] (K[i][j]: how strongly element i drives the scale of element j) and per latent part
    `stiffest_direction/<part>`, `softest_direction/<part>`; centred, `correlation_centred` and `eigenvalues_centred`.  The
    second inner kernel of --method=i: the same names with the suffix `_1` (`correlation_1`, `stiffest_direction_1/<part>`)."""
    np.savez(file_path_base + "_geometry.npz", **arrays)


# what _convergence_report hands a side report (k: the leading chains split R-hat covers; the moments: already all-reduced)
_Run = collections.namedtuple("_Run", "kernel_results trace k n_split spec flags dev arrays split_mean pooled_mean pooled_sd")
# A report with a side file, in run order: its flag; the tag its arrays wait under among those of _rhat.npz; null(flags) -> its
# keys as null without a device trace; its writer; report(run) -> (JSON keys, arrays or None), or None: the row above leaves them.
SideReport = collections.namedtuple("SideReport", "flag tag null save report")
_NO_TRACE = "no chain has its trace on the device"
SIDE_REPORTS = (
    SideReport("energy_diagnostics", ENERGY_ARRAYS, None, save_energy,
               lambda r: _energy_report(r.kernel_results, r.trace, r.spec, r.flags, r.dev)),
    SideReport("trajectory_profile", TRAJECTORY_ARRAYS, None, save_trajectory,             # (LMAX: 0 is off)
               lambda r: _trajectory_report(r.kernel_results, r.trace, r.spec, r.flags, r.dev, r.pooled_sd)),
    SideReport("geometry_diagnostics", GEOMETRY_ARRAYS, None, save_geometry,
               lambda r: _geometry_report(r.kernel_results, r.trace, r.k, r.spec, r.flags, r.dev, r.split_mean)),
    SideReport("predictive_diagnostics", LOO_ARRAYS, lambda flags: _loo_null(_NO_TRACE, flags), save_loo,
               lambda r: _loo_report(r.kernel_results, r.trace, r.k, r.spec, r.flags, r.arrays)),
    SideReport(None, LOO_PRED_ARRAYS, None, save_loo_pred, None),
    SideReport("predictive_checks", PPC_ARRAYS, lambda flags: _ppc_null(_NO_TRACE, flags), save_ppc,
               lambda r: _ppc_report(r.kernel_results, r.trace, r.k, r.n_split, r.spec, r.flags, r.dev)),
    SideReport("sensitivity_diagnostics", PSENS_ARRAYS, lambda flags: _psens_null(_NO_TRACE, flags), save_psens,
               lambda r: _psens_report(r.trace, r.k, r.spec, r.flags, r.split_mean, r.arrays)),
    SideReport(None, PSENS_SITES_ARRAYS, None, save_psens_sites, None),
    SideReport("prior_predictive_checks", PRIOR_ARRAYS,
               lambda flags: _prior_null(_NO_TRACE + ", so there is no pooled posterior to set the prior against"), save_prior,
               lambda r: _prior_report(r.spec, r.flags, r.trace.device, r.pooled_mean, r.pooled_sd)))


def _save_diagnostics(file_path_base, arrays):
    """<base>_rhat.npz, then the side file of every row of SIDE_REPORTS whose arrays _convergence_report left under its tag."""
    if arrays is None:
        return
    side = [(row.save, arrays.pop(row.tag)) for row in SIDE_REPORTS if row.tag in arrays]
    save_rhat(file_path_base, arrays)
    for save, side_arrays in side:
        save(file_path_base, side_arrays)


def save_rhat(file_path_base, arrays):
    """`<base>_rhat.npz` (build-specific): per latent part `split_rhat/<part>` and the pooled `posterior_mean/<part>`,
    `posterior_sd/<part>` over the chains the split statistic covers, [*event] each; a streaming run adds the same three
    over ALL chains from the in-kernel statistics (`rhat_all_chains/`, `posterior_mean_all_chains/`, `posterior_sd_all_chains/`);
    --superchain_size adds `nested_rhat/<part>` over all chains and the profile `nested_rhat_by_step` [S] (the largest
    element of every recorded step) with `nested_rhat_by_step_element` [S] (which element that is)."""
    np.savez(file_path_base + "_rhat.npz", **arrays)


def _read_vi_fit(file_path):
    """The JSON a VI run of the same method left behind (step sizes, variational parameters, tuning runs so far)."""
    if not os.path.exists(file_path):
        raise Exception("Run VI first to find initial step sizes")
    with open(file_path, "r") as f:
        return json.load(f)


def check_superchains(M, num_chains, world_size=1):
    """--superchain_size M against the job: raises ValueError unless M = 0 (off) or M >= 2 divides num_chains into at
    least two superchains, and every rank's shard (parallel.shard_bounds) holds whole superchains."""
    M, num_chains, world_size = int(M), int(num_chains), int(world_size)
    if M == 0:
        return
    if M < 2:
        raise ValueError("--superchain_size must be 0 (off) or at least 2, not %d" % M)
    if num_chains % M != 0:
        raise ValueError("--superchain_size=%d does not divide --num_chains=%d" % (M, num_chains))
    if num_chains // M < 2:
        raise ValueError("--superchain_size=%d leaves %d superchain(s) of --num_chains=%d: nested R-hat needs at least two"
                         % (M, num_chains // M, num_chains))
    if world_size > 1 and num_chains % (M * world_size) != 0:
        raise ValueError("--superchain_size=%d: the %d ranks of this job must hold whole superchains (--num_chains=%d is "
                         "not a multiple of %d)" % (M, world_size, num_chains, M * world_size))


def tie_superchains(parts, M, world_size=1):
    """The initial population tied into superchains of M adjacent chains (Margossian et al. 2024): chain c takes the state
    of chain (c // M) * M, for every latent part ([C, *event] arrays).  The chains' random streams are keyed by their
    global id and stay their own, which is what makes tied chains part ways.  M = 0: `parts` itself, untouched."""
    if int(M) == 0:
        return parts
    n = int(np.asarray(parts[0]).shape[0])
    check_superchains(M, n, world_size)
    leader = (np.arange(n) // int(M)) * int(M)
    return [np.ascontiguousarray(np.asarray(p)[leader]) for p in parts]


def _initial_population(fit, model_config, flags):
    """num_chains draws from the fitted mean-field Normal (reference util.py:394-410), one array per latent part; with
    --superchain_size M tied into superchains (tie_superchains)."""
    M = int(getattr(flags, "superchain_size", 0) or 0)
    check_superchains(M, flags.num_chains, parallel.world()[1])               # (before anything is drawn or launched)
    names = _param_names(model_config)
    population = list(util.variational_inits_from_params(fit["learned_variational_params"], param_names=names,
                                                         num_inits=flags.num_chains, seed=flags.seed).values())
    return tie_superchains(population, M, parallel.world()[1])


def _settle_leapfrog_count(fit, tuning, flags):
    """--num_leapfrog_steps as given; a tuning run insists on it (and is skipped when the file already has that count),
    a sampling run without it takes the best tuning run's.  Returns False when there is nothing to do."""
    if tuning:
        if not flags.num_leapfrog_steps:
            raise ValueError("You must specify the number of leapfrog steps for a tuning run.")
        done = [t for t in fit.get("tuning_runs", []) if t["num_leapfrog_steps"] == flags.num_leapfrog_steps]
        if done:
            util.print_("tuning run with {} leapfrog steps is already recorded ({}): skipped".format(
                flags.num_leapfrog_steps, done[0]))
            return False
    elif not flags.num_leapfrog_steps:
        flags.num_leapfrog_steps = get_best_num_leapfrog_steps_from_tuning_runs(fit["tuning_runs"])
    util.print_("\nsampling with {} leapfrog steps per transition\n".format(flags.num_leapfrog_steps))
    if flags.count_in_leapfrog_steps:
        # schedule lengths given in gradient evaluations (reference main.py:331-336)
        for name in ("num_samples", "num_burnin_steps", "num_adaptation_steps"):
            setattr(flags, name, int(getattr(flags, name) / float(flags.num_leapfrog_steps)))
    return True


def run_hmc(model_config, results_dir, file_path, tuning=False, flags=FLAGS, out=None):
    """One HMC run (or one HMCtuning run) of a fitted method: the reference's run_hmc (main.py:296-398) -- same inputs,
    files and keys; chains sharded over the ranks of the job, statistics combined at the end."""
    fit = _read_vi_fit(file_path)
    if not _settle_leapfrog_count(fit, tuning, flags):
        return
    initial_states = _initial_population(fit, model_config, flags)
    target, _, _, _, _, reparam = create_target_graph(model_config, results_dir, flags)
    # one process per GPU: every rank draws the same initial population and keeps its block of chains
    rank, ws = parallel.world()
    initial_states, chain_offset = parallel.shard_states(initial_states, rank, ws)
    clock = time.time()
    _, kernel_results, samples, ess_final = inference.hmc(
        target, model_config, fit["initial_step_size"], initial_states=initial_states, reparam=reparam, flags=flags,
        chain_offset=chain_offset)
    mcmc_time = time.time() - clock
    if out is not None:
        out["kernel_results"] = kernel_results      # .ess_info, .moments: what the run knows beyond the reference's tuple
    per_1000_gradients = 1000.0 / (flags.num_samples * flags.num_leapfrog_steps)
    normalized_ess_final = [e * per_1000_gradients for e in ess_final]
    info = kernel_results.ess_info
    dev = flags.device if ws > 1 else None
    n_ess = _ess_chain_count(info, model_config, flags)          # None: a chain subset (streaming run)
    ess_min, sem_min, acceptance_rate, _ = parallel.summarize(
        normalized_ess_final, kernel_results.inner_results.is_accepted, flags.num_samples, flags.num_chains, device=dev,
        ess_chains_total=n_ess)
    util.print_("ESS per 1000 gradients: {} +/- {}".format(ess_min, sem_min))
    extra = _ess_report(info, model_config, flags, dev, normalized_ess_final)
    rhat_arrays = None
    if not tuning:
        convergence, rhat_arrays = _convergence_report(kernel_results, model_config, flags, dev)
        extra.update(convergence)
    if ws > 1 and not tuning:
        # _ess.npz / _ess.txt hold every chain's per-element ESS: collect the other ranks' blocks (a collective: all ranks)
        normalized_ess_final = parallel.gather_parts(normalized_ess_final, n_ess, flags.device)
        if flags.num_chains_to_save > 0:
            # _traces.npz holds the JOB's first chains, whichever ranks own them (rank 0's block may be shorter)
            samples = parallel.gather_leading_chains(samples, flags.num_chains_to_save, chain_offset, flags.device)
    summary = (ess_min, sem_min, acceptance_rate, mcmc_time)
    if rank != 0:
        return summary
    if tuning:
        # the reference's keys of a tuning_runs entry, no more
        save_hmc_results(file_path=file_path, tuning_runs=dict(
            num_leapfrog_steps=flags.num_leapfrog_steps, ess_min=float(ess_min), sem_min=float(sem_min),
            acceptance_rate=float(acceptance_rate), mcmc_time=mcmc_time, num_samples=flags.num_samples,
            num_burnin_steps=flags.num_burnin_steps))
        return summary
    save_hmc_results(file_path=file_path, ess_min=float(ess_min), sem_min=float(sem_min),
                     acceptance_rate=float(acceptance_rate), mcmc_time_sec=mcmc_time, **extra)
    save_ess(file_path_base=file_path[:-5], samples=samples, param_names=_param_names(model_config),
             normalized_ess_final=normalized_ess_final, num_chains_to_save=flags.num_chains_to_save)
    _save_diagnostics(file_path[:-5], rhat_arrays)
    return summary


def run_interleaved_hmc_with_leapfrog_steps(model_config, results_dir, num_leapfrog_steps_cp,
                                            num_leapfrog_steps_ncp, initial_step_size_cp, initial_step_size_ncp,
                                            initial_states_cp, flags=FLAGS):
    """reference main.py:401-449"""
    target, model, elbo, vp, lp, actual_reparam = create_target_graph(model_config, results_dir, flags)
    target_cp, target_ncp = target
    rank, ws = parallel.world()
    initial_states_cp, chain_offset = parallel.shard_states(list(initial_states_cp), rank, ws)
    start_time = time.time()
    states, kernel_results, ess_final = inference.hmc_interleaved(
        model_config, target_cp, target_ncp, num_leapfrog_steps_cp=num_leapfrog_steps_cp,
        num_leapfrog_steps_ncp=num_leapfrog_steps_ncp, step_size_cp=initial_step_size_cp,
        step_size_ncp=initial_step_size_ncp, initial_states_cp=initial_states_cp, flags=flags,
        chain_offset=chain_offset)
    mcmc_time = time.time() - start_time
    is_accepted_cp = kernel_results.cp_results.inner_results.is_accepted
    is_accepted_ncp = kernel_results.ncp_results.inner_results.is_accepted
    normalized_ess_final = [1000 * e / (flags.num_samples * flags.num_leapfrog_steps) for e in ess_final]
    dev = flags.device if ws > 1 else None
    info = kernel_results.ess_info
    n_ess = _ess_chain_count(info, model_config, flags)
    ess_min, sem_min, acc_cp, _ = parallel.summarize(normalized_ess_final, is_accepted_cp, flags.num_samples,
                                                     flags.num_chains, device=dev, ess_chains_total=n_ess)
    extra = _ess_report(info, model_config, flags, dev, normalized_ess_final)
    # (before the trace is released below)
    convergence, rhat_arrays = _convergence_report(kernel_results, model_config, flags, dev)
    extra.update(convergence)
    acc_ncp = float(parallel.all_reduce_sum(float(np.sum(is_accepted_ncp)), dev).item()) * 100.0 / float(
        flags.num_samples * flags.num_chains)
    util.print_("ESS: {} +/- {}".format(ess_min, sem_min))
    if ws > 1:
        normalized_ess_final = parallel.gather_parts(normalized_ess_final, n_ess, flags.device)
    # Only `[:, :num_chains_to_save]` of the samples is ever read again (save_ess).  Taking that slice to the host now
    # releases the [S, C, D] device trace before the next candidate leapfrog count allocates its own (two 18.6 GB traces
    # alive at once at the headline size, and a fresh device allocation of that size can cost half a second).
    k = max(0, int(flags.num_chains_to_save))
    if k > 0:
        states = parallel.gather_leading_chains(states, k, chain_offset, flags.device if ws > 1 else None)
    else:
        states = [np.zeros((flags.num_samples, 0), np.float32) for _ in states]
    del kernel_results, is_accepted_cp, is_accepted_ncp
    return (ess_min, sem_min, acc_cp, acc_ncp, mcmc_time, states, normalized_ess_final, extra, rhat_arrays)


def _first_existing(results_dir, names):
    for n in names:
        p = os.path.join(results_dir, n)
        if os.path.exists(p):
            return p
    return None


def _tuned_fit(results_dir, names, what):
    """(step sizes, best tuned leapfrog count, variational parameters) of a CP / NCP fit this directory holds; the
    reference writes `CP_tied.json` and looks for `CP.json`: both spellings are accepted."""
    path = _first_existing(results_dir, names)
    if path is None:
        raise Exception("Run VI first to find initial step sizes, and HMC first to find num_leapfrog_steps.")
    with open(path, "r") as f:
        fit = json.load(f)
    if not fit.get("tuning_runs"):
        raise Exception("no HMCtuning run recorded for {}: run --inference=HMCtuning --method={} first".format(path, what))
    return fit["initial_step_size"], get_best_num_leapfrog_steps_from_tuning_runs(fit["tuning_runs"]), \
        fit["learned_variational_params"]


def run_interleaved_hmc(model_config, results_dir, file_path, flags=FLAGS):
    """--method=i: the interleaved CP / NCP sampler started from the centred fit, once per tuned leapfrog count of the two
    fits, keeping the run with the larger ESS (reference main.py:452-528, intended behaviour: module docstring)."""
    tied = "_tied" if flags.tied_pparams else ""
    step_cp, ls_cp, vparams_cp = _tuned_fit(results_dir, ["CP.json", "CP%s.json" % tied], "CP")
    step_ncp, ls_ncp, _ = _tuned_fit(results_dir, ["NCP.json", "NCP%s.json" % tied], "NCP")
    initial_states_cp = _initial_population({"learned_variational_params": vparams_cp}, model_config, flags)
    kept, kept_ls = None, None
    for num_ls in sorted({ls_ncp, ls_cp}):
        flags.num_leapfrog_steps = 2 * num_ls          # what the ESS normalisation counts (reference main.py:493)
        util.print_("\ninterleaved sampling with {0} + {0} leapfrog steps per step\n".format(num_ls))
        run = run_interleaved_hmc_with_leapfrog_steps(
            model_config=model_config, results_dir=results_dir, num_leapfrog_steps_cp=num_ls,
            num_leapfrog_steps_ncp=num_ls, initial_step_size_cp=step_cp, initial_step_size_ncp=step_ncp,
            initial_states_cp=initial_states_cp, flags=flags)
        if kept is None or float(run[0]) > float(kept[0]):
            kept, kept_ls = run, num_ls
    (ess_min, sem_min, acceptance_rate_cp, acceptance_rate_ncp, mcmc_time, samples, normalized_ess_final, extra,
     rhat_arrays) = kept
    flags.num_leapfrog_steps = 2 * kept_ls
    if parallel.world()[0] != 0:
        return kept
    save_hmc_results(file_path=file_path, initial_step_size_ncp=step_ncp, initial_step_size_cp=step_cp,
                     num_leapfrog_steps=kept_ls, ess_min=float(ess_min), sem_min=float(sem_min),
                     acceptance_rate_cp=float(acceptance_rate_cp), acceptance_rate_ncp=float(acceptance_rate_ncp),
                     mcmc_time_sec=mcmc_time, **extra)
    save_ess(file_path_base=file_path[:-5], samples=samples, param_names=_param_names(model_config),
             normalized_ess_final=normalized_ess_final, num_chains_to_save=flags.num_chains_to_save)
    _save_diagnostics(file_path[:-5], rhat_arrays)
    return kept


def save_hmc_results(file_path, **record):
    """Append one run to the result file: every key of the JSON object is a list with one entry per run (the file contract
    of reference main.py:531-550 -- analyze.py and a later cVIP -> dVIP step read these lists)."""
    history = {}
    if os.path.exists(file_path):
        with open(file_path) as f:
            history = json.load(f)
    for key, value in record.items():
        history.setdefault(key, []).append(value)
    _write_json_atomic(file_path, history)


def save_ess(file_path_base, samples, normalized_ess_final, param_names, num_chains_to_save=0):
    """The side files of a sampling run (file contract of reference main.py:552-585): `<base>_ess.npz` with one [C, *event]
    array of normalised ESS per latent part, `<base>_ess.txt` with the same arrays printed, then their mean and standard
    deviation over chains, and -- with --num_chains_to_save -- `<base>_traces.npz` with the first chains' samples."""
    ess_by_part = {name: np.asarray(e) for name, e in zip(param_names, normalized_ess_final)}
    np.savez(file_path_base + "_ess.npz", **ess_by_part)
    lines = ["{}: {}\n\n".format(name, e) for name, e in ess_by_part.items()]
    lines.append("\n\n")
    for name, e in ess_by_part.items():
        lines.append("{} mean: {}\n".format(name, e.mean(axis=0)))
        lines.append("{} stddev: {}\n\n".format(name, e.std(axis=0)))
    with open(file_path_base + "_ess.txt", "w") as f:
        f.writelines(lines)
    if num_chains_to_save > 0:
        np.savez(file_path_base + "_traces.npz",
                 **{name: x[:, :num_chains_to_save] for name, x in zip(param_names, samples)})


def main(argv=None, flags=FLAGS, out=None):
    """reference main.py:190-231.  `out`: an optional dict a plain HMC run leaves its kernel results in (tests, tools)."""
    if argv is not None:
        flags.parse(list(argv))
    if flags.reparameterise_variational:
        # util.make_variational_model_special (reference util.py:334-391) is outside the hot path this build covers;
        # accepting the flag silently would write a *_reparam_variational*.json that holds ordinary mean-field results
        raise NotImplementedError("--reparameterise_variational is not supported by this build (SURVEY.md section 2)")
    check_predictive(flags)
    check_loo_groups(flags)
    check_loo_moment_match(flags)
    check_predictive_checks(flags)
    check_predictive_redraw(flags)
    check_predictive_groups(flags)
    check_sensitivity(flags)
    check_sensitivity_sites(flags)
    check_prior_predictive(flags)
    check_vi_diagnostics(flags)
    _sbc.check_sbc(flags)
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    if ws > 1:
        # launched by torch.distributed.run: one rank per GPU, RCCL for the statistics exchange
        import torch
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0"))
        if util.debug_switch("ARP_SHARE_GPU") and torch.cuda.device_count():
            local %= torch.cuda.device_count()     # tests only: several ranks on one GPU (with the gloo backend below)
        flags.device = "cuda:%d" % local
        if torch.cuda.is_available():          # (the engine itself fails loudly without a GPU)
            torch.cuda.set_device(local)
        if flags.inference == "VI":
            # VI is a one-workgroup-per-learning-rate job with nothing to exchange: rank 0 runs it and writes the
            # JSON, the other ranks leave, and NO process group is created -- a communicator whose peers have exited
            # (or a barrier sitting in the RCCL watchdog for as long as the fit takes) is exactly what to avoid.
            if (dist.get_rank() if dist.is_initialized() else int(os.environ.get("RANK", "0"))) != 0:
                return None
        elif not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            backend = util.debug_switch("ARP_DIST_BACKEND") or "nccl"   # "nccl" is RCCL; "gloo": tests that share one GPU
            if backend != "nccl":
                dist.init_process_group(backend)
            else:
                try:
                    dist.init_process_group("nccl", device_id=torch.device(flags.device))
                except TypeError:                                     # older torch: no device_id keyword
                    dist.init_process_group("nccl")
    util.print_("Loading model {} with dataset {}.".format(flags.model, flags.dataset))
    model_config = models.get_model_by_name(flags.model, dataset=flags.dataset)
    results_dir = flags.results_dir if flags.results_dir != "" else flags.model + "_" + flags.dataset
    if not os.path.exists(results_dir):
        os.makedirs(results_dir)
    filename = "{}{}{}{}{}.json".format(
        flags.method,
        ("_" + flags.learnable_parameterisation_type if "VIP" in flags.method else ""),
        ("_tied" if flags.tied_pparams else ""),
        ("_reparam_variational" if "VIP" in flags.method and flags.reparameterise_variational else ""),
        ("_discrete_prior" if "VIP" in flags.method and flags.discrete_prior else ""))
    file_path = os.path.join(results_dir, filename)
    if flags.inference == "VI":
        return run_vi(model_config, results_dir, file_path, flags)
    if flags.inference == "SBC":
        return _sbc.run_sbc(model_config, results_dir, file_path, flags, out=out)
    if flags.inference not in ("HMC", "HMCtuning"):
        raise Exception("unknown inference {}".format(flags.inference))
    try:
        if flags.inference == "HMC":
            if flags.method == "i":
                return run_interleaved_hmc(model_config, results_dir, file_path, flags)
            return run_hmc(model_config, results_dir, file_path, tuning=False, flags=flags, out=out)
        return run_hmc(model_config, results_dir, file_path, tuning=True, flags=flags)
    finally:
        # Every rank reads the result file at the top of a sampling phase (step sizes, tuning_runs -> the leapfrog count)
        # and rank 0 rewrites it at the end of one: no rank may enter the next phase before rank 0's write has landed,
        # or the ranks could sample with different leapfrog counts.  (A rank that raised never reaches its peers'
        # barrier; the launcher then tears the job down.)
        if sys.exc_info()[0] is None:
            parallel.barrier()


if __name__ == "__main__":
    main(sys.argv[1:])
