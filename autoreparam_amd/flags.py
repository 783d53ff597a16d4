"""Command-line flags with the reference's names and defaults (main.py:37-113 and
program_transformations.py:44-49).  absl is not a dependency: a small parser
accepts the same ``--flag=value`` / ``--flag value`` / ``--[no]flag`` spellings,
and the values live on a module-level ``FLAGS`` object as in the reference (the
library functions take it as an explicit ``flags=`` argument with FLAGS as default).
"""
import copy

_DEFS = [
    # name, type, default, help
    ("model", str, "8schools", "Model to be used."),
    ("dataset", str, "", "Dataset to be used."),
    ("inference", str, "VI", "Inference method to be used: VI, HMCtuning, HMC, or SBC (simulation-based calibration of the "
                             "whole VI + HMC flow on data simulated from the prior: --sbc_replications)."),
    ("method", str, "CP", "Method to be used: CP, NCP, i (only if inference = HMC), cVIP, dVIP."),
    ("learnable_parameterisation_type", str, "eig", "Type of learnable parameterisation (scalar models ignore it)."),
    ("reparameterise_variational", bool, False, "Not supported by this build (off in the reference too)."),
    ("discrete_prior", bool, False, "Prior encouraging the parameterisation parameters to be 0 or 1."),
    ("tied_pparams", bool, True, "Tie the loc and scale parameterisation parameters (a=b)."),
    ("results_dir", str, "", "Directory to write results."),
    ("learning_rates", list, [0.02, 0.05, 0.1, 0.2, 0.4], "Learning rates (list)"),
    ("num_optimization_steps", int, 3000, "Number of steps to optimize the ELBO."),
    ("num_mc_samples", int, 256, "Number of Monte Carlo samples to use in the ELBO."),
    ("num_leapfrog_steps", int, None, "Number of leapfrog steps."),
    ("count_in_leapfrog_steps", bool, False, "Interpret sample/burn-in/adaptation counts as gradient evaluations."),
    ("num_samples", int, 50000, "Number of HMC samples."),
    ("num_chains", int, 100, "Number of HMC chains."),
    ("num_burnin_steps", int, 10000, "Number of warm-up steps."),
    ("num_adaptation_steps", int, 6000, "Number of adaptation steps."),
    ("num_chains_to_save", int, 0, "Number of chains to save traces for."),
    ("float64", bool, False, "Unused by the scalar-Normal models of this build."),
    # build-specific additions (the reference is unseeded and single-device)
    ("seed", int, 0, "Seed of the sampler's counter-based RNG and of the variational initial states."),
    ("device", str, "cuda:0", "GPU to run on."),
    ("trace_chunk_rows", int, None, "Force the streaming mode (moments and batch means accumulated inside the kernels, "
                                    "a whole trace only for --ess_chains chains; batch length of the batch-means ESS = "
                                    "this / 8).  Default: automatic, only "
                                    "when the trace does not fit in HBM."),
    ("ess_chains", int, 1024, "Streaming mode: the chains with global id below this keep their whole [S, k, D] trace on "
                              "the device, and the reported ESS is the reference's autocorrelation ESS of those chains "
                              "(the batch-means figure of all chains is written next to it)."),
    ("convergence_diagnostics", bool, True, "Sampling runs: split R-hat across chains and the pooled posterior mean / sd of "
                                            "every element (JSON keys, <base>_rhat.npz), computed after the mcmc clock "
                                            "has stopped; --noconvergence_diagnostics skips all of it."),
    ("rank_normalized_rhat", bool, False, "Sampling runs, with --convergence_diagnostics: also the rank-normalised, folded "
                                          "split R-hat (bulk, tail; Vehtari et al. 2021) and the pooled posterior median, "
                                          "5 % and 95 % quantiles of every element over the chains split R-hat covers "
                                          "(rank_rhat_* JSON keys, five more families in <base>_rhat.npz).  One process only: "
                                          "a sharded job writes null."),
    ("bulk_tail_ess", bool, False, "Sampling runs, with --convergence_diagnostics: also the multi-chain bulk-ESS, tail-ESS "
                                   "and Monte-Carlo standard error of the posterior mean of every element (Vehtari et al. "
                                   "2021; what Stan, posterior and ArviZ report next to the rank-normalised R-hat) over the "
                                   "chains split R-hat covers (ess_bulk_min, ess_tail_min, ess_mean_min, "
                                   "mcse_mean_over_sd_max JSON keys, four more families in <base>_rhat.npz).  ess_min "
                                   "stays the reference's per-chain figure.  One process only: a sharded job writes null."),
    ("superchain_size", int, 0, "Nested R-hat (Margossian et al. 2024): M >= 2 ties the initial population into "
                                "num_chains / M superchains of M adjacent chains that start from one point (chain c takes "
                                "the initial state of chain (c // M) * M) and run on their own random streams; with "
                                "--convergence_diagnostics the run then reports nested R-hat over ALL chains, streaming "
                                "and sharded jobs included, and its profile over the recorded steps (nested_rhat_* JSON "
                                "keys and arrays in <base>_rhat.npz).  M must divide num_chains (and every rank's share) "
                                "and leave at least two superchains.  0: off."),
    ("energy_diagnostics", bool, False, "Sampling runs, with --convergence_diagnostics: probe the finished run's integrator "
                                        "(arp_energy_probe): one fresh-momentum trajectory, with the run's own step sizes "
                                        "and leapfrog count, from the final state of every chain and from "
                                        "--energy_probe_steps recorded steps of the device trace -- not a replay of the "
                                        "transitions the sampler took.  Reports the rate of divergent trajectories (energy "
                                        "error not finite or above 1000, Stan's threshold), the energy error's mean and sd, "
                                        "the expected acceptance and the kinetic share of the energy variance "
                                        "(divergence_rate, energy_* JSON keys, <base>_energy.npz with the states where "
                                        "trajectories diverged).  Sharded jobs included."),
    ("energy_probe_steps", int, 8, "With --energy_diagnostics: how many evenly spaced recorded steps of the device trace "
                                   "are probed (the first and the last among them; fewer if fewer were recorded)."),
    ("trajectory_profile", int, 0, "Sampling runs, with --convergence_diagnostics: LMAX in 1 ... 256 profiles the trajectory "
                                   "length (arp_trajectory_probe, arp_jump_sums).  From the states --energy_diagnostics "
                                   "probes, one fresh-momentum trajectory of LMAX leapfrog steps with the run's own step "
                                   "sizes, every step recorded: the Metropolis-weighted expected squared jump distance of "
                                   "the worst element, per gradient, for every leapfrog count 1 ... LMAX at once, and the "
                                   "count that maximises it (trajectory_* JSON keys, <base>_trajectory.npz).  Not a replay "
                                   "of the sampler's transitions; the step sizes are those adapted for the run's own "
                                   "count; a one-transition criterion, not an ESS.  0: off."),
    ("geometry_diagnostics", bool, False, "Sampling runs, with --convergence_diagnostics: the posterior geometry report -- why "
                                          "this parameterisation mixes the way it does.  The cross-element second moments of "
                                          "the recorded draws (arp_gram_sums, on the matrix cores) over the chains split R-hat "
                                          "covers, centred and in the sampler's own coordinates: the condition number of the "
                                          "correlation matrix, the same for the covariance scaled by the run's base steps, the "
                                          "most correlated pair of elements, the stiff and the soft direction, and the scale "
                                          "coupling of every pair, which sees the funnels that linear correlation does not "
                                          "(geometry_* JSON keys, <base>_geometry.npz).  A second-order summary pooled over "
                                          "chains, not a local metric; unconverged chains inflate it.  Sharded jobs included."),
    ("predictive_diagnostics", bool, False, "Sampling runs, with --convergence_diagnostics: judge the MODEL, not the sampler. "
                                            "The pointwise log-likelihood of every observation at --loo_draws draws of the "
                                            "chains split R-hat covers (arp_pointwise_loglik), then Pareto-smoothed "
                                            "importance-sampling leave-one-out cross-validation and WAIC per observation "
                                            "(arp_psis_loo; Vehtari, Gelman, Gabry 2017; Vehtari et al. 2024): elpd_loo, "
                                            "p_loo, elpd_waic, p_waic with standard errors and the Pareto k-hat of every "
                                            "observation (loo_*, elpd_*, pareto_k_* JSON keys, <base>_loo.npz; two models of "
                                            "the same data are compared by analyze --loo_compare).  No r_eff correction, no "
                                            "moment matching or refits for high k-hat, no K-fold.  One process only: a "
                                            "sharded job writes null.  Refused for neals_funnel, which has no observations."),
    ("loo_draws", int, 65536, "With --predictive_diagnostics: the draws per observation, taken as loo_draws // chains evenly "
                              "spaced recorded steps of the device trace (at least one, at most all; the last step among "
                              "them)."),
    ("predictive_checks", bool, False, "Sampling runs, with --convergence_diagnostics: posterior predictive checks -- does "
                                       "data simulated from the fitted model look like the data?  For every draw the "
                                       "--predictive_diagnostics report would take (--loo_draws of the chains split R-hat "
                                       "covers) one replicated data set at the observed covariates (arp_predictive_check; "
                                       "Gelman, Meng, Stern 1996), folded on the device: posterior predictive p-values of "
                                       "the mean, sd, min, max and deviance, the predictive mean and sd of every observation "
                                       "and its PIT value with their calibration (ppc_* JSON keys, <base>_ppc.npz).  The "
                                       "posterior PIT (the leave-one-out PIT: --loo_predictive); group-level statistics: "
                                       "--predictive_checks_groups; no user-defined statistic.  "
                                       "Every quantity is a sum over draws: sharded jobs included.  Refused for "
                                       "neals_funnel, which has no observations."),
    ("predictive_checks_redraw", str, "", "With --predictive_checks only: PART[,PART...], latent parts of the model (e.g. m for "
                                          "radon, theta for 8schools, beta_log_scales,beta for "
                                          "german_credit_gammascale).  The MIXED predictive check (Gelman, Meng, Stern 1996; "
                                          "Marshall, Spiegelhalter 2007) next to the posterior one, on the same draws: every "
                                          "draw keeps its hyperparameters, the named parts are drawn anew from their "
                                          "conditional prior given them (arp_site_redraw over ModelSpec.site_table) and the "
                                          "data are replicated from the redrawn rows (arp_predictive_check).  The posterior "
                                          "check replicates at group effects fitted to the very data they are checked "
                                          "against; the mixed one asks whether a NEW group under these hyperparameters would "
                                          "have produced an observation -- leave-group-out cross-validation without a refit "
                                          "(ppc_mixed_* JSON keys, <base>_ppc_mixed.npz; analyze --ppc prints a second line).  "
                                          "Every output of --predictive_checks is bit for bit unchanged.  The selection is by "
                                          "part, not by element or group; the data are replicated at the observed "
                                          "covariates; per-group test statistics: --predictive_checks_groups.  Refused: the flag without "
                                          "--predictive_checks, neals_funnel, a name that is no part of the model, a "
                                          "duplicate, an empty name, and a selection that is not closed under descent -- a "
                                          "part that stays as recorded although it was drawn from a redrawn one (mua without "
                                          "m); the message names the parts to add."),
    ("predictive_checks_groups", str, "", "With --predictive_checks only: PART, one latent part of the model whose elements "
                                          "group the observations (m for radon: the counties; a for election: the states; a "
                                          "or b for electric; theta for 8schools).  The predictive check per GROUP: the same "
                                          "replicated data, bit for bit, folded per group and draw (arp_group_predictive_check) "
                                          "into the posterior predictive p-values of every group's mean, sd, min, max and "
                                          "deviance -- a whole-data mean over 919 observations hides a county of six that the "
                                          "model cannot produce (ppc_group_* JSON keys, <base>_ppc_groups.npz; analyze --ppc "
                                          "prints a line).  With --predictive_checks_redraw the same per group at the redrawn "
                                          "group effects (ppc_group_mixed_*; Marshall, Spiegelhalter 2007): which group is "
                                          "not a draw from its prior layer.  A group is the set of observations whose linear "
                                          "predictor reads one element of the part; an observation that reads none is in no "
                                          "group, an element nobody reads is an empty group; both are counted in the keys.  "
                                          "Groups are flagged at 0.005 / (non-empty groups), Bonferroni at the customary 1 %, "
                                          "when the draws resolve that.  Every other output is bit for bit unchanged.  One "
                                          "part per run; no groups by covariate; no user-defined statistic; the posterior "
                                          "p-values are conservative, the group effect having been fitted to the group.  "
                                          "Refused: the flag without --predictive_checks, neals_funnel, a name that is no "
                                          "part, a part of one element (the whole-data check), a part no observation reads, "
                                          "a part of which an observation reads several elements (beta of German credit)."),
    ("loo_predictive", bool, False, "With --predictive_diagnostics only: the leave-one-out predictive report.  The predictive "
                                    "mean, variance and PIT value of every observation at every draw, folded with the "
                                    "Pareto-smoothed weights of its own leave-one-out posterior (arp_psis_weights, "
                                    "arp_loo_predictive; Vehtari, Gelman, Gabry 2017): the LOO predictive mean and sd and the "
                                    "LOO-PIT of every observation -- the honest counterpart of the posterior PIT of "
                                    "--predictive_checks -- with their calibration, RMSE and R^2 (Normal data) or Brier "
                                    "score and accuracy (Bernoulli data) (loo_pred_*, loo_pit_*, loo_* JSON keys, "
                                    "<base>_loopred.npz).  No r_eff, no predictive quantiles or intervals, no moment "
                                    "matching; an observation with a high Pareto k-hat is as unreliable here as its "
                                    "elpd_loo.  Every other output of --predictive_diagnostics is bit for bit unchanged.  "
                                    "One process only: a sharded job writes null."),
    ("loo_groups", str, "", "With --predictive_diagnostics only: PART, one latent part of the model whose elements group the "
                            "observations (m for radon: the counties; theta for 8schools; a or b for electric; a for "
                            "election -- the rule of --predictive_checks_groups).  PSIS leave-one-GROUP-out cross-validation "
                            "on the draws of the report: how well does the model predict a county it has not seen?  "
                            "Per group and draw the joint log-likelihood of the group's observations (arp_group_loglik) in "
                            "two forms: CONDITIONAL, at the recorded group effect, whose importance ratios usually have "
                            "a high Pareto k-hat; and MARGINAL, the group's own effect integrated against its conditional "
                            "prior N(loc, exp(s)) in closed form (Normal data; Merkle, Furr, Rabe-Hesketh 2019), whose "
                            "reciprocal is the exact leave-group-out ratio.  arp_psis_loo reads either in the place of a "
                            "pointwise log-likelihood (elpd_logo, logo_* JSON keys, <base>_logo.npz; analyze --loo prints a "
                            "line, analyze --logo_compare pairs two models by group).  Bernoulli data (election) get the "
                            "conditional form only: no quadrature.  No moment matching or refits for high k-hat, one part "
                            "per run, the data at the observed covariates, and k-hat is itself an estimate.  Every other "
                            "output of --predictive_diagnostics is bit for bit unchanged.  Refused: the flag without "
                            "--predictive_diagnostics, neals_funnel, and what --predictive_checks_groups refuses of a part."),
    ("loo_moment_match", bool, False, "With --predictive_diagnostics only: moment matching for the observations -- and, with "
                                      "--loo_groups, the groups in their CONDITIONAL form -- whose Pareto k-hat is above the "
                                      "threshold (implicitly adaptive importance sampling: Paananen, Piironen, Buerkner, "
                                      "Vehtari 2021; loo::loo_moment_match).  The draws are moved by an affine map in the "
                                      "centred coordinates until their weighted mean (T1) and marginal variance (T2) match, the "
                                      "centred log joint and the left-out term are evaluated there, the tail is fitted again, "
                                      "and the estimate is taken from the split of the paper's section 4 (arp_weighted_moments, "
                                      "arp_affine_rows; loo_mm_* and logo_mm_* JSON keys, <base>_loo_mm.npz, <base>_logo_mm.npz; "
                                      "analyze --loo prints a line).  No refit of the model.  No covariance map (T3), no "
                                      "moment-matched --loo_predictive figures, no r_eff, not the marginal group form; the log "
                                      "joint is float32.  Every other output of --predictive_diagnostics is bit for bit "
                                      "unchanged.  One process only: a sharded job writes null.  Refused: the flag without "
                                      "--predictive_diagnostics, neals_funnel."),
    ("loo_moment_match_max", int, 64, "With --loo_moment_match: the most observations (and the most groups) taken, the worst "
                                      "k-hat first; the others above the threshold are counted (loo_mm_not_attempted).  "
                                      "1 ... 4096."),
    ("sensitivity_diagnostics", bool, False, "Sampling runs, with --convergence_diagnostics: how much of each posterior "
                                             "marginal comes from the prior, how much from the data?  Power-scaling "
                                             "sensitivity (Kallioinen, Paananen, Buerkner, Vehtari 2023; priorsense, ArviZ "
                                             "psens) on the draws --predictive_diagnostics takes (--loo_draws of the chains "
                                             "split R-hat covers, centred): the prior -- the joint density of all latent "
                                             "sites, the hierarchical layers included -- and the likelihood are raised to "
                                             "1 / 1.01 and 1.01, the draws importance-weighted by the Pareto-smoothed ratios "
                                             "(arp_psis_weights), every element's pooled draws ordered (arp_element_order) and "
                                             "the cumulative Jensen-Shannon distance between the unweighted and the weighted "
                                             "ECDF folded on the device (arp_cjs_sums).  Sensitivities above 0.05 are "
                                             "diagnosed: prior and likelihood -- prior-data conflict; prior alone -- weak "
                                             "likelihood or strong prior (psens_* JSON keys, <base>_psens.npz; analyze "
                                             "--psens).  delta is fixed, no power-scaling sequence; a choice of prior sites: "
                                             "--sensitivity_prior_parts.  "
                                             "One process only: a sharded job writes null.  Refused for neals_funnel, which "
                                             "has no observations."),
    ("sensitivity_prior_parts", str, "", "With --sensitivity_diagnostics only: NAME[,NAME...], latent parts of the model (a "
                                         "part is one of the model's random variables, e.g. b1,log_sigma_a for election).  A "
                                         "second report on the same draws power-scales the priors of the named parts ALONE "
                                         "-- the sum of their sites' log densities (arp_site_logprior over "
                                         "ModelSpec.site_table) -- instead of the joint prior, which in a hierarchical model "
                                         "also scales the group level: is the posterior sensitive to the priors I chose?  "
                                         "(psens_sites_* JSON keys, <base>_psens_sites.npz; analyze --psens prints a second "
                                         "line).  Every output of --sensitivity_diagnostics is bit for bit unchanged.  The "
                                         "selection is by part, not by element; delta is fixed and there is no power-scaling "
                                         "sequence here either.  Refused: a name that is no part of the model, a duplicate, "
                                         "an empty name, the flag without --sensitivity_diagnostics."),
    ("prior_predictive_checks", bool, False, "Sampling runs, with --convergence_diagnostics: prior predictive checks, the "
                                             "first step of the Bayesian workflow (Gabry et al. 2019) -- what data does the "
                                             "model generate before it has seen any, and how far did the data move every "
                                             "marginal?  --loo_draws ancestral draws from the latent site table "
                                             "(arp_site_prior_draws over ModelSpec.site_table; no device trace is needed), one "
                                             "replicated data set each (arp_predictive_check): where the observed mean, sd, "
                                             "min, max and deviance sit among the prior-predicted ones and the prior 90 % band "
                                             "of the replicated mean and sd; and per element the posterior contraction "
                                             "1 - (posterior sd / prior sd)^2 and the z-score (posterior mean - prior median) "
                                             "/ prior sd, the prior's sd taken from its 5 % and 95 % points (a log-scale prior "
                                             "N(0, 10) has no usable sample variance), the posterior's the pooled moment "
                                             "(prior_* JSON keys, <base>_prior.npz; analyze --prior).  No warning: no "
                                             "threshold can be derived for a prior predictive p-value, a weak prior is meant "
                                             "to be wider than the data.  No prior draws at new covariates, no "
                                             "simulation-based calibration, no user-defined statistic.  Rank 0 of a sharded "
                                             "job runs it alone.  Every other output is bit for bit unchanged.  Refused for "
                                             "neals_funnel, which has no observations."),
    ("vi_diagnostics", bool, False, "--inference=VI: judge the mean-field FIT the sampler takes its step sizes, its initial "
                                    "population and (cVIP, dVIP) its parameterisation from.  After the fit's clock has "
                                    "stopped, --vi_check_draws draws from the fitted q in the coordinates of the "
                                    "parameterisation the fit ended in (arp_vi_draws), their log importance ratios "
                                    "log p - log q, the Pareto k-hat of the ratios' tail (arp_psis_weights; Yao, Vehtari, "
                                    "Simpson, Gelman 2018) and one fold (arp_vi_fold): had the optimiser converged (the "
                                    "ELBO's gradient at the final parameters), is q close to the posterior (k-hat, the "
                                    "evidence, KL), and if so how far off are loc and scale (vi_* JSON keys, "
                                    "<base>_vicheck.npz).  A check of the final iterate of the best learning rate only; it "
                                    "changes no step size and no initial state.  A result file written without the flag "
                                    "is checked from its stored fit, without refitting."),
    ("vi_check_draws", int, 65536, "With --vi_diagnostics: the draws from q, 1024 ... 2^20."),
    ("sbc_replications", int, 256, "--inference=SBC: N in 8 ... 16384, the replicates of simulation-based calibration (Talts "
                                   "et al. 2018).  Each is one ancestral draw from the prior (arp_site_prior_draws), one data "
                                   "set simulated from it at the observed covariates (arp_predictive_check) and one refit of "
                                   "the whole flow on that data -- the VI fit, then --num_chains chains of HMC with "
                                   "--num_leapfrog_steps, seeded by --seed + 1 + r -- whose draws at --sbc_steps recorded steps "
                                   "are ranked against the truth, per element and for the joint log-likelihood "
                                   "(arp_sbc_fold).  Uniform ranks are what a sampler of the model's posterior returns "
                                   "(sbc_* keys in <method>_sbc.json, <method>_sbc.npz; analyze --sbc).  --method=CP or NCP, "
                                   "one process, a model with observations."),
    ("sbc_steps", int, 1, "--inference=SBC: how many evenly spaced recorded steps of every replicate's trace are ranked (the "
                          "last among them), 1 ... the recorded steps of the run; L = sbc_steps * num_chains draws per "
                          "replicate.  Draws of consecutive steps are dependent: above 1 the rank histogram gains a U-shape "
                          "of its own."),
    ("lanes_per_chain", int, 0, "Lanes of a wave64 a chain is spread over (0 = automatic)."),
]


class FlagValues(object):
    def __init__(self):
        for name, _, default, _ in _DEFS:
            setattr(self, name, copy.copy(default))

    def copy(self):
        return copy.deepcopy(self)

    def parse(self, argv):
        """Parse ``argv`` (without the program name); returns the non-flag leftovers."""
        types = {n: t for n, t, _, _ in _DEFS}
        rest = []
        i = 0
        while i < len(argv):
            arg = argv[i]
            i += 1
            if not arg.startswith("--"):
                rest.append(arg)
                continue
            body = arg[2:]
            if "=" in body:
                name, val = body.split("=", 1)
            else:
                name, val = body, None
            if name not in types and name.startswith("no") and types.get(name[2:]) is bool and val is None:
                setattr(self, name[2:], False)
                continue
            if name not in types:
                raise ValueError("Unknown command line flag '%s'" % name)
            t = types[name]
            if t is bool:
                if val is None:
                    setattr(self, name, True)
                else:
                    if val.lower() in ("true", "t", "1", "yes"):
                        setattr(self, name, True)
                    elif val.lower() in ("false", "f", "0", "no"):
                        setattr(self, name, False)
                    else:
                        raise ValueError("flag --%s: bad boolean %r" % (name, val))
                continue
            if val is None:
                if i >= len(argv):
                    raise ValueError("flag --%s needs a value" % name)
                val = argv[i]
                i += 1
            if t is list:
                setattr(self, name, [v for v in val.split(",") if v != ""])
            elif t is int:
                setattr(self, name, int(val))
                if name == "trajectory_profile":
                    check_trajectory_profile(self.trajectory_profile)
            else:
                setattr(self, name, val)
        return rest


VI_CHECK_DRAWS_MIN, VI_CHECK_DRAWS_MAX = 1024, 1 << 20      # the range of --vi_check_draws


def check_vi_check_draws(value):
    """--vi_check_draws as an int in VI_CHECK_DRAWS_MIN ... VI_CHECK_DRAWS_MAX; raises ValueError outside."""
    value = int(value)
    if not VI_CHECK_DRAWS_MIN <= value <= VI_CHECK_DRAWS_MAX:
        raise ValueError("--vi_check_draws must lie in %d ... %d, not %d" % (VI_CHECK_DRAWS_MIN, VI_CHECK_DRAWS_MAX, value))
    return value


TRAJECTORY_PROFILE_MAX = 256      # the largest --trajectory_profile (arp_trajectory_probe's n_leapfrog_max)


def check_trajectory_profile(value):
    """--trajectory_profile as an int in 0 ... TRAJECTORY_PROFILE_MAX; raises ValueError outside."""
    value = int(value or 0)
    if not 0 <= value <= TRAJECTORY_PROFILE_MAX:
        raise ValueError("--trajectory_profile must lie in 0 (off) ... %d, not %d" % (TRAJECTORY_PROFILE_MAX, value))
    return value


FLAGS = FlagValues()
