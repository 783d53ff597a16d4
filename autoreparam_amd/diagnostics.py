"""Convergence diagnostics across chains: the potential scale reduction factor R-hat (Gelman-Rubin; the split form of
BDA3 / Stan / ArviZ, without rank normalisation) and the pooled posterior mean / sd of every element; and, on request,
the rank-normalised, folded form of Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021 (`rank_rhat`: what Stan, posterior
and ArviZ report as R-hat now) with the pooled posterior median and 5 % / 95 % quantiles; and the numbers the same paper
reports next to it, bulk-ESS, tail-ESS and the Monte-Carlo standard error of the mean (`bulk_tail_ess`), from one
multi-chain autocorrelation estimator on the device (`arp_ess_multichain`); and nested R-hat over superchains (Margossian,
Hoffman, Sountsov, Riou-Durand, Vehtari, Gelman 2024: `nested_fold`, `nested_step_sums`), the form for many short chains;
and the energy report of probed trajectories (`energy_sums`, `energy_from_sums` on Engine.energy_probe's output: divergent
trajectories, energy-error moments, expected acceptance, the kinetic share of the energy variance); and the
trajectory-length profile (`profile_from_sums` on Engine.trajectory_sums' output: the worst element's expected squared jump
distance per gradient for every leapfrog count up to Lmax, from fresh-momentum trajectories with every step recorded);
and the posterior geometry report (`gram_sums` on `arp_gram_sums`, the cross moments of a trace on the matrix cores;
`geometry_from_sums`: correlation matrix, its condition number, the stiff and the soft direction, the step-scaled
condition number; `scale_coupling`, `coupling_from_sums`: the funnel detector); and, the one report that judges the model
and not the sampler, PSIS-LOO and WAIC (`pointwise_loglik` on `arp_pointwise_loglik`, `psis_loo` on `arp_psis_loo`;
`loo_summary`, `loo_compare`, `pareto_k_threshold`: the host float64 folds) and the posterior predictive check
(`predictive_check` on `arp_predictive_check`: replicated observations folded on the device; `combine_draw_stats`,
`ppc_summary`: the test statistics, their p-values, the per-observation predictive moments and the PIT calibration) with
its leave-one-out counterpart (`loo_predictive` on `arp_loo_predictive`: the same predictive quantities folded with the
smoothed weights of `psis_weights`; `loo_predictive_summary`: the LOO predictive mean and sd, the LOO-PIT); and
the one report that judges the variational fit the sampler inherits its steps and its start from (`vi_check` on
`arp_vi_draws`, `arp_psis_weights` and `arp_vi_fold`; `vi_check_summary`: the Pareto k-hat of the importance ratios p / q,
the ELBO and its gradient at the final parameters, the importance-corrected loc and scale; Yao et al. 2018); and
power-scaling sensitivity (`powerscale_lw`, `element_order` on `arp_element_order`, `cjs_sums` on `arp_cjs_sums`,
`loglik_total`; `psens_summary`: how far every marginal moves when the prior or the likelihood is raised to a power
slightly off 1, as a cumulative Jensen-Shannon distance; Kallioinen et al. 2023), with the log prior density of every
latent site, summed over chosen groups of elements, for power-scaling chosen priors alone (`upload_site_table`,
`site_logprior` on `arp_site_logprior`); and the prior itself (`site_prior_draws` on `arp_site_prior_draws`: ancestral draws
from the site table; `prior_predictive_summary`, `prior_contraction_summary`: what data the prior generates, and how far
the data moved every marginal away from it), and the same walk over recorded draws (`site_redraw` on `arp_site_redraw`: the
parts `redraw_selection` flags drawn anew from their conditional prior, the rest kept -- the rows a mixed predictive check
replicates its data from); and the predictive check per group of observations (`group_selection`: the groups a latent part
forms; `group_predictive_check` on `arp_group_predictive_check`: the same replicated data folded per group and draw;
`ppc_group_counts`, `ppc_group_summary`: `ppc_counts` and `ppc_from_counts` applied group by group).

Build-specific (the reference runs 100 chains and reports the within-chain ESS only).  The per-chain moments come from
one pass over a trace that is already on the device (`arp_split_moments`) or from the in-kernel statistics of a
streaming run (`arp_hmc_io.stats` through engine.stats_summary); `arp_moments_fold` sums them over chains into five
[D] vectors that are additive over chains, hence over ranks; the statistic itself is a few lines of float64 numpy.

With m rows (chains, or half-chains) of n draws each, W = mean of the rows' variances and B/n = variance of the rows'
means:  rhat = sqrt(((n-1)/n W + B/n) / W),  pooled sd = sqrt((n-1)/n W + B/n),  pooled mean = mean of the rows' means.
"""
import collections
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

# rhat, mean, sd: [D] float64 (NaN where W = 0 or fewer than two rows have a finite variance); rows = m, the number of
# rows with a finite variance; constant_rows = how many of them never moved (variance exactly 0)
Rhat = collections.namedtuple("Rhat", ["rhat", "mean", "sd", "rows", "constant_rows"])
# bulk, tail: the split R-hat of the rank-normalised and of the folded, rank-normalised trace; rhat = fmax of the two;
# median, q05, q95: order statistics of the pooled draws; rows, constant_rows as above (of the bulk trace); [D] float64
RankRhat = collections.namedtuple("RankRhat", ["bulk", "tail", "rhat", "median", "q05", "q95", "rows", "constant_rows"])

# bulk, tail, mean: the multi-chain ESS of the rank-normalised trace, of the 5 % / 95 % indicators (the smaller) and of the
# draws; mcse_mean = sd / sqrt(mean); sd: the pooled posterior sd; [D] float64
BulkTailEss = collections.namedtuple("BulkTailEss", ["bulk", "tail", "mean", "mcse_mean", "sd"])

# Nested R-hat, [D] float64: rhat = sqrt(1 + excess), excess = between / within (B / W: its stationary value is at most
# 1 / M), superchains = K that counted, left_out = superchains with a non-finite row.  NaN where W = 0 or K < 2.
NestedRhat = collections.namedtuple("NestedRhat", ["rhat", "excess", "between", "within", "superchains", "left_out"])

# Energy report of probed trajectories (Engine.energy_probe).  divergence_rate = divergent / rows; divergent: the energy
# error is not finite or above DIVERGENCE_THRESHOLD; nonfinite: the not-finite ones among them; error_mean, error_sd: of
# the energy error over the other rows; accept_prob: mean of min(1, exp(-error)), divergent rows counting 0;
# kinetic_share = (D / 2) / Var(E0).  NaN where there are too few rows.
Energy = collections.namedtuple("Energy", ["divergence_rate", "divergent", "nonfinite", "rows", "error_mean", "error_sd",
                                           "accept_prob", "kinetic_share"])
# Trajectory-length profile from the jump sums of probed trajectories (Engine.trajectory_sums), one entry per leapfrog
# count l = 1 ... Lmax ([Lmax] arrays): rows, divergent, nonfinite, left_out as energy_sums counts them per l;
# accept_prob = mean alpha; esjd [Lmax, D] = J / (rows v), the Metropolis-weighted expected squared jump distance of
# every element in units of its posterior variance (2 (1 - rho_1) at stationarity); esjd_min and esjd_min_element: the
# worst element among those with a finite, positive variance (-1: none); per_gradient = esjd_min / l; best_leapfrogs: the
# smallest l that attains the largest per_gradient (0: none is finite).  NaN where there is nothing to divide by.
Profile = collections.namedtuple("Profile", ["leapfrogs", "rows", "divergent", "nonfinite", "left_out", "accept_prob",
                                             "divergence_rate", "esjd", "esjd_min", "esjd_min_element", "per_gradient",
                                             "best_leapfrogs"])
# Posterior geometry from the cross moments of `gram_sums` (geometry_from_sums).  rows, rows_left_out: the counts (NaN for
# rows_left_out where D = 1 leaves no room for it); mean, sd [D] float64 (sd NaN for an element left out); left_out: the
# indices of the elements whose variance is not finite or not > 0, kept: the others, k of them; cov, correlation [k, k] and
# eigenvalues [k] (ascending, of the correlation matrix) over the kept elements; condition_number = largest / smallest
# eigenvalue (inf when the smallest is <= 0, NaN when k = 0); softest_direction, stiffest_direction [D]: the unit eigenvectors
# of the largest and the smallest eigenvalue, zeros at the elements left out; max_abs_correlation and
# max_correlation_pair (i, j) in the indices of all D elements, (-1, -1) when k < 2; step_scaled_eigenvalues [k] and
# step_scaled_condition_number: of diag(1 / eps0) cov diag(1 / eps0), None / NaN without eps0.
Geometry = collections.namedtuple("Geometry", ["rows", "rows_left_out", "mean", "sd", "kept", "left_out", "cov", "correlation",
                                               "eigenvalues", "condition_number", "softest_direction", "stiffest_direction",
                                               "max_abs_correlation", "max_correlation_pair", "step_scaled_eigenvalues",
                                               "step_scaled_condition_number"])
JUMP_HEAD = 5                     # scalars in front of J in a row of the jump sums (csrc/jump.hip)
DIVERGENCE_THRESHOLD = 1000.0     # Stan's: a trajectory whose energy error exceeds it is reported as divergent
GRAM_WINDOW = 256                 # rows a float32 accumulator of arp_gram_sums runs over (csrc/gram.hip: kGramWindow)
GRAM_MAX_D = 512                  # the widest matrix arp_gram_sums takes
COUPLING_FLOOR = 1e-12            # v = 0.5 log(u^2 + this): keeps the log finite at u = 0 (scale_coupling)


def split_moments(trace, split=True):
    """(mean, var) [P, C, D] float32 device tensors of a recorded [S, C, D] float32 trace on the GPU: P = 2 halves of
    S // 2 draws (split) or P = 1.  A leading or inner block of chains of a wider trace is taken in place, as
    util.effective_sample_size does; the workspace of the long-trace route is owned here."""
    x, S, Cn, D, row_stride = _lib.trace_view(trace, "split_moments")
    P = 2 if split else 1
    mean = torch.empty(P, Cn, D, dtype=torch.float32, device=trace.device)
    var = torch.empty(P, Cn, D, dtype=torch.float32, device=trace.device)
    if Cn == 0 or D == 0:
        return mean, var
    if S == 0:
        return mean.fill_(float("nan")), var.fill_(float("nan"))
    L = _lib.lib()
    _lib.call(x.device, L.arp_split_moments, _lib.ptr(x), S, Cn * D, row_stride, int(bool(split)), _lib.ptr(mean),
              _lib.ptr(var), workspace=L.arp_moments_workspace_bytes(S, Cn * D, int(bool(split))))
    return mean, var


def _rows(moments):
    """[..., D] moments as the contiguous float32 [rows, D] matrix the fold kernels read."""
    return moments.reshape(-1, int(moments.shape[-1])).to(torch.float32).contiguous()


def fold(mean, var):
    """The [5, D] float64 device tensor of `arp_moments_fold` over every leading axis of `mean`, `var` ([..., D] float32
    on the GPU): count, sum of mean, sum of mean^2, sum of var over the rows with a finite var, and how many have var == 0."""
    if not (mean.is_cuda and mean.shape == var.shape):
        raise ValueError("fold: mean and var of one shape on the GPU are required (there is no CPU fallback)")
    m, v = _rows(mean), _rows(var)
    D = int(m.shape[1])
    sums = torch.empty(5, D, dtype=torch.float64, device=mean.device)
    if D == 0:
        return sums
    _lib.call(mean.device, _lib.lib().arp_moments_fold, _lib.ptr(m), _lib.ptr(v), m.shape[0], D, _lib.ptr(sums))
    return sums


def rhat_from_sums(sums, n):
    """The statistic from the (all-reduced) [5, D] sums of `fold` over rows of `n` draws each -> Rhat."""
    s = _lib.host64(sums)
    n = float(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = s[0]
        nan = np.full_like(m, np.nan)
        w = np.where(m >= 1, s[3] / m, nan)
        b_n = np.where(m >= 2, (s[2] - s[1] * s[1] / m) / (m - 1), nan)
        b_n = np.maximum(b_n, 0.0)                     # (propagates NaN)
        v = (n - 1.0) / n * w + b_n if n > 0 else nan
        rhat = np.where(w > 0, np.sqrt(v / w), nan)
        return Rhat(rhat, np.where(m >= 1, s[1] / m, nan), np.sqrt(v), m, s[4])


def from_stats(mean, var):
    """The sums for the UN-split R-hat of every chain of a streaming run from the per-chain (mean, var) [C, D] that
    engine.stats_summary returns (the statistics planes keep no half-way snapshot)."""
    return fold(mean, var)


def _workspace_bytes(symbol, S, Cn, D, flag):
    """What the library's sizing function `symbol` asks for a [S, Cn, D] trace: 0 for an empty one, raises on a refusal."""
    if S <= 0 or Cn <= 0 or D <= 0:
        return 0
    need = int(getattr(_lib.lib(), symbol)(S, Cn, D, int(bool(flag))))
    if need <= 0:
        _lib.check(1)
    return need


def rank_workspace_bytes(S, Cn, D, fold=False):
    """Bytes of device workspace `rank_normalize` takes for a [S, Cn, D] trace (next to its [S, Cn, D] float32 result)."""
    return _workspace_bytes("arp_rank_workspace_bytes", S, Cn, D, fold)


def rank_normalize(trace, fold=False, probs=None, rank2=None):
    """(z, median, quantiles) device tensors of a recorded [S, C, D] float32 trace on the GPU (`arp_rank_normalize`):
    z [S, C, D] float32, the normal score Phi^-1((r - 3/8) / (N + 1/4)) of every draw's average rank r among the
    N = S C pooled draws of its element -- of the draw itself, or (fold) of its float32 distance from the element's
    median; median [D] float32 and quantiles [len(probs), D] float32 (None without probs): order statistics of the
    pooled draws, x_(k) with k = ceil(p N).  rank2: an optional contiguous [S, C, D] int32 device tensor that receives
    2 r - 1 as unsigned 32-bit words.  A leading or inner block of chains of a wider trace is taken in place, as
    split_moments takes it; the workspace is owned here."""
    x, S, Cn, D, row_stride = _lib.trace_view(trace, "rank_normalize")
    probs = None if probs is None else [float(p) for p in probs]
    z = torch.empty(S, Cn, D, dtype=torch.float32, device=trace.device)
    median = torch.full((D,), float("nan"), dtype=torch.float32, device=trace.device)
    quantiles = None if probs is None else torch.full((len(probs), D), float("nan"), dtype=torch.float32, device=trace.device)
    _lib.device_operand(rank2, torch.int32, (S, Cn, D), "rank_normalize", "rank2", "S, C, D")
    if S == 0 or Cn == 0 or D == 0:
        return z, median, quantiles
    pr = (C.c_double * len(probs))(*probs) if probs else None
    _lib.call(x.device, _lib.lib().arp_rank_normalize, _lib.ptr(x), S, Cn, D, row_stride, int(bool(fold)), _lib.ptr(z),
              _lib.ptr(rank2), _lib.ptr(median), pr, len(probs) if probs else 0, _lib.ptr(quantiles if probs else None),
              workspace=rank_workspace_bytes(S, Cn, D, fold))
    return z, median, quantiles


def ess_multichain_workspace_bytes(S, Cn, D, split=True):
    """Bytes of device workspace `ess_multichain` takes for a [S, Cn, D] trace."""
    return _workspace_bytes("arp_ess_multichain_workspace_bytes", S, Cn, D, split)


def ess_multichain(trace, split=True, threshold=None, n_rho=0):
    """(ess, max_t, rho) device tensors of a recorded [S, C, D] float32 trace on the GPU (`arp_ess_multichain`): the
    multi-chain effective sample size of every element, ess [D] float32 (NaN for an element that never moved or with
    fewer than four draws per row); max_t [D] int32, where Geyer's initial sequence was cut; rho [n_rho, D] float32 (None
    for n_rho = 0), the pooled autocorrelations up to lag max_t + 1 and NaN beyond.  split: rows are half-chains.
    threshold: an optional [D] float32 device tensor; the statistic is then that of the indicator x <= threshold[d],
    which is never written out.  A leading or inner block of chains of a wider trace is taken in place, as rank_normalize
    takes it; the workspace is owned here."""
    x, S, Cn, D, row_stride = _lib.trace_view(trace, "ess_multichain")
    n_rho = int(n_rho)
    _lib.device_operand(threshold, torch.float32, (D,), "ess_multichain", "threshold", "D")
    ess = torch.full((D,), float("nan"), dtype=torch.float32, device=trace.device)
    max_t = torch.zeros(D, dtype=torch.int32, device=trace.device)
    rho = torch.full((n_rho, D), float("nan"), dtype=torch.float32, device=trace.device) if n_rho > 0 else None
    if S == 0 or Cn == 0 or D == 0:
        return ess, max_t, rho
    _lib.call(x.device, _lib.lib().arp_ess_multichain, _lib.ptr(x), S, Cn, D, row_stride, int(bool(split)),
              _lib.ptr(threshold), _lib.ptr(ess), _lib.ptr(max_t), _lib.ptr(rho), n_rho,
              workspace=ess_multichain_workspace_bytes(S, Cn, D, split))
    return ess, max_t, rho


def bulk_tail_ess(trace):
    """Bulk-ESS, tail-ESS and the Monte-Carlo standard error of the mean of every element of a [S, C, D] float32 trace on
    the GPU (Vehtari et al. 2021) -> BulkTailEss: `bulk` is ess_multichain (split) of the rank-normalised z trace, `tail`
    the smaller of ess_multichain of the indicators x <= q05 and x <= q95 (q: the pooled order statistic x_(ceil(p N)) of
    rank_normalize -- posterior interpolates its quantile, one draw's rank away), `mean` that of the draws themselves,
    mcse_mean = sd / sqrt(mean) with the pooled sd of split_moments -> fold -> rhat_from_sums."""
    S = int(trace.shape[0])
    z, _, q = rank_normalize(trace, fold=False, probs=(0.05, 0.95))
    bulk = ess_multichain(z, True)[0]
    del z
    lo = ess_multichain(trace, True, threshold=q[0].contiguous())[0]
    hi = ess_multichain(trace, True, threshold=q[1].contiguous())[0]
    mean = ess_multichain(trace, True)[0]
    sd = rhat_from_sums(fold(*split_moments(trace, True)), S // 2).sd
    lo, hi, mean = _lib.host64(lo), _lib.host64(hi), _lib.host64(mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        return BulkTailEss(_lib.host64(bulk), np.minimum(lo, hi), mean, sd / np.sqrt(mean), sd)


def rank_rhat(trace):
    """The rank-normalised split R-hat of every element of a [S, C, D] float32 trace on the GPU -> RankRhat: `bulk` from
    the normal scores of the draws, `tail` from those of their distances from the median, `rhat` the larger, each through
    split_moments -> fold -> rhat_from_sums on the z-score trace.  The ranks are taken over all S rows: for odd S the
    middle draw is ranked but belongs to no half; for even S this is the value of Stan and posterior::rhat."""
    S = int(trace.shape[0])
    z, median, q = rank_normalize(trace, fold=False, probs=(0.05, 0.95))
    bulk = rhat_from_sums(fold(*split_moments(z, True)), S // 2)
    del z
    z, _, _ = rank_normalize(trace, fold=True)
    tail = rhat_from_sums(fold(*split_moments(z, True)), S // 2)
    del z
    q = _lib.host64(q)
    return RankRhat(bulk.rhat, tail.rhat, np.fmax(bulk.rhat, tail.rhat), _lib.host64(median), q[0], q[1], bulk.rows,
                    bulk.constant_rows)


def nested_fold(mean, var, M):
    """The [6, D] float64 device tensor of `arp_moments_fold_nested` over the [C, D] per-chain moments (float32 on the
    GPU; leading axes are flattened): superchains of M adjacent chains.  Rows: the superchains that count (all M chains
    finite), sum of g, sum of g^2, sum of b, sum of w, superchains left out.  var = None: one draw per chain, every
    within-chain variance is 0."""
    if not (mean.is_cuda and (var is None or (var.is_cuda and var.shape == mean.shape))):
        raise ValueError("nested_fold: mean (and var, of the same shape) on the GPU are required (there is no CPU fallback)")
    m, v = _rows(mean), None if var is None else _rows(var)
    D = int(m.shape[1])
    sums = torch.empty(6, D, dtype=torch.float64, device=mean.device)
    if D == 0:
        return sums
    _lib.call(mean.device, _lib.lib().arp_moments_fold_nested, _lib.ptr(m), _lib.ptr(v), m.shape[0], D, int(M), _lib.ptr(sums))
    return sums


def _nested(k, sg, sgg, sb, sw):
    """(rhat, excess, B, W) from sums over k superchains, float64 numpy of any one shape."""
    with np.errstate(divide="ignore", invalid="ignore"):
        nan = np.full_like(k, np.nan)
        between = np.where(k >= 2, np.maximum(sgg - sg * sg / k, 0.0) / (k - 1), nan)
        within = np.where(k >= 1, (sb + sw) / k, nan)
        excess = np.where(within > 0, between / within, nan)
        return np.sqrt(1.0 + excess), excess, between, within


def nested_rhat_from_sums(sums):
    """The statistic from the (all-reduced) [6, D] sums of `nested_fold` -> NestedRhat."""
    s = _lib.host64(sums)
    rhat, excess, between, within = _nested(s[0], s[1], s[2], s[3], s[4])
    return NestedRhat(rhat, excess, between, within, s[0], s[5])


def nested_step_workspace_bytes(S, Cn, D, M):
    """Bytes of device workspace `nested_step_sums` takes for a [S, Cn, D] trace (0: none)."""
    return int(_lib.lib().arp_nested_step_workspace_bytes(S, Cn, D, int(M)))


def nested_step_sums(trace, M):
    """The [4, S, D] float64 device tensor of `arp_nested_step_sums` for a recorded [S, C, D] float32 trace on the GPU: for
    every row s the one-draw-per-chain sums over superchains of M adjacent chains -- the superchains that count, sum of g,
    sum of g^2, sum of b.  A leading or inner block of chains of a wider trace is taken in place, as split_moments takes
    it; the workspace is owned here."""
    x, S, Cn, D, row_stride = _lib.trace_view(trace, "nested_step_sums")
    sums = torch.zeros(4, S, D, dtype=torch.float64, device=trace.device)
    if S == 0 or Cn == 0 or D == 0:
        return sums
    _lib.call(x.device, _lib.lib().arp_nested_step_sums, _lib.ptr(x), S, Cn, D, row_stride, int(M), _lib.ptr(sums),
              workspace=nested_step_workspace_bytes(S, Cn, D, M))
    return sums


def nested_rhat_by_step(sums4):
    """[S, D] float64 nested R-hat of every row from the (all-reduced) [4, S, D] sums of `nested_step_sums`."""
    s = _lib.host64(sums4)
    return _nested(s[0], s[1], s[2], s[3], np.zeros_like(s[3]))[0]


def energy_sums(out4):
    """The float64 [9] tensor of sums over the rows of `out4` ([N, 4]: logp and kinetic energy at the start and at the end
    of a probed trajectory, Engine.energy_probe), additive over rows, hence over probe calls and ranks: plain torch
    reductions on the device `out4` lives on (the probe's output never leaves the GPU for them).  With
    the energy error dh = (lp0 - lp1) + (ke1 - ke0) formed in float64 and E0 = ke0 - lp0: rows; divergent rows (dh not finite
    or above DIVERGENCE_THRESHOLD); rows with a non-finite dh; sum of dh and of dh^2 over the other rows; sum of
    min(1, exp(-dh)), a divergent row counting 0; sum of E0 and of E0^2; sum of ke0."""
    if not (torch.is_tensor(out4) and out4.dim() == 2 and out4.shape[1] == 4):
        raise ValueError("energy_sums: an [N, 4] tensor is required")
    o = out4.to(torch.float64)
    lp0, ke0, lp1, ke1 = o[:, 0], o[:, 1], o[:, 2], o[:, 3]
    dh = (lp0 - lp1) + (ke1 - ke0)
    finite = torch.isfinite(dh)
    divergent = ~finite | (dh > DIVERGENCE_THRESHOLD)
    zero = torch.zeros_like(dh)
    d = torch.where(divergent, zero, dh)
    acc = torch.where(divergent, zero, torch.exp(-d).clamp(max=1.0))
    e0 = ke0 - lp0
    return torch.stack([torch.tensor(float(o.shape[0]), dtype=torch.float64, device=o.device),
                        divergent.sum().to(torch.float64), (~finite).sum().to(torch.float64), d.sum(), (d * d).sum(),
                        acc.sum(), e0.sum(), (e0 * e0).sum(), ke0.sum()])


def energy_from_sums(sums, D):
    """The report from the (all-reduced) [9] sums of `energy_sums` over trajectories of a D-dimensional state -> Energy.
    kinetic_share = (D / 2) / Var(E0) is Betancourt's E-BFMI, E[Var(E | q)] / Var(E), with the numerator exact: given q the
    energy varies by the kinetic energy alone, half a chi-square of D degrees of freedom, whose variance is D / 2.  Stan
    estimates the same quantity from consecutive transitions (lag one), and that estimator reads about twice as large on a
    well-mixed chain: its numerator is the mean squared change of E between two transitions, which for an accurate
    integrator is that of a momentum resampling, E[(K' - K)^2] = 2 Var(K) = D, twice the numerator here.  Stan's customary
    threshold (0.3) is therefore not this figure's, and none is applied."""
    s = _lib.host64(sums).reshape(9)
    rows, divergent, nonfinite = int(round(s[0])), int(round(s[1])), int(round(s[2]))
    good = rows - divergent
    nan = float("nan")
    error_mean = s[3] / good if good >= 1 else nan
    error_sd = float(np.sqrt(max(s[4] - s[3] * s[3] / good, 0.0) / (good - 1))) if good >= 2 else nan
    var_e0 = (s[7] - s[6] * s[6] / rows) / (rows - 1) if rows >= 2 else nan
    share = 0.5 * D / var_e0 if np.isfinite(var_e0) and var_e0 > 0 else nan
    return Energy(divergent / rows if rows else nan, divergent, nonfinite, rows, error_mean, error_sd,
                  s[5] / rows if rows else nan, share)


def profile_from_sums(sums, var):
    """The trajectory-length profile from the (all-reduced) [Lmax, 5 + D] jump sums of Engine.trajectory_sums and the
    run's pooled posterior variance `var` [D] -> Profile.  The worst element's expected squared jump distance per gradient
    is the customary criterion for a trajectory length (Pasarica & Gelman 2010); it is the one-transition counterpart of
    the min-ESS-per-gradient figure a set of tuning runs is compared by, not an ESS.  The trajectories behind the sums start
    from fresh momenta (no replay of the sampler's transitions) and use the step sizes the run adapted for its own leapfrog
    count; a run at another count would adapt others.  An empty or degenerate input gives NaN, never an exception."""
    s, v = _lib.host64(sums), _lib.host64(var).reshape(-1)
    if s.ndim != 2 or s.shape[1] < JUMP_HEAD:
        s = np.zeros((0, JUMP_HEAD + v.size))
    Lmax, D = s.shape[0], s.shape[1] - JUMP_HEAD
    if v.size != D:
        v = np.full(D, np.nan)
    leapfrogs = np.arange(1, Lmax + 1)
    rows = s[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        nan = np.full(Lmax, np.nan)
        some = rows > 0
        accept = np.where(some, s[:, 3] / rows, nan)
        rate = np.where(some, s[:, 1] / rows, nan)
        esjd = np.where(some[:, None], s[:, JUMP_HEAD:] / (rows[:, None] * v[None, :]), np.nan)
    usable = np.isfinite(v) & (v > 0)
    esjd_min, at = nan.copy(), np.full(Lmax, -1, np.int64)
    for l in range(Lmax):
        e = np.where(usable & np.isfinite(esjd[l]), esjd[l], np.inf)
        if e.size and np.isfinite(e).any():
            at[l] = int(e.argmin())
            esjd_min[l] = e[at[l]]
    per_gradient = esjd_min / leapfrogs
    ok = np.isfinite(per_gradient)
    best = int(leapfrogs[ok][per_gradient[ok].argmax()]) if ok.any() else 0    # (argmax: the first, hence smallest, l of a tie)
    return Profile(leapfrogs, rows, s[:, 1], s[:, 2], s[:, 4], accept, rate, esjd, esjd_min, at, per_gradient, best)


def gram_sums(trace_or_matrix, shift=None):
    """The [D + 2, D] float64 device tensor of `arp_gram_sums` for a recorded [S, C, D] float32 trace or a plain [n, D]
    float32 matrix on the GPU: rows 0 ... D - 1 hold G = sum_r u_r u_r^T with u_r = x_r - shift (float32, one rounding)
    over the rows without a non-finite element, row D the sum of u_r, row D + 1 the rows that counted and the rows left
    out.  shift: a [D] float32 device tensor or None (zeros).  Additive over rows, hence over calls and ranks that use
    one shift.  A leading or inner block of chains of a wider trace, and a matrix whose rows are further apart than D, are
    read in place; the workspace is owned here.  An empty input gives zeros."""
    x = trace_or_matrix
    if torch.is_tensor(x) and x.dim() == 2:
        if not (x.is_cuda and x.dtype == torch.float32):
            raise ValueError("gram_sums: a float32 [S, C, D] trace or [n, D] matrix on the GPU is required (there is no CPU fallback)")
        n, D = (int(v) for v in x.shape)
        if not (x.is_contiguous() or (x.stride(1) == 1 and x.stride(0) >= D)):
            x = x.contiguous()
        S, Cn, row_stride = n, 1, (int(x.stride(0)) if n > 1 else D)
    else:
        x, S, Cn, D, row_stride = _lib.trace_view(x, "gram_sums")
    _lib.device_operand(shift, torch.float32, (D,), "gram_sums", "shift", "D")
    sums = torch.zeros(D + 2, D, dtype=torch.float64, device=x.device)
    if S == 0 or Cn == 0 or D == 0:
        return sums
    L = _lib.lib()
    _lib.call(x.device, L.arp_gram_sums, _lib.ptr(x), S, Cn, D, row_stride, _lib.ptr(shift), _lib.ptr(sums),
              workspace=L.arp_gram_workspace_bytes(S, Cn, D))
    return sums


def _moments_from_sums(sums):
    """(n, left out, m = mean of u, cov) in float64 from [D + 2, D] sums; cov is NaN throughout for n < 2."""
    s = _lib.host64(sums)
    if s.ndim != 2 or s.shape[0] != s.shape[1] + 2:
        raise ValueError("a [D + 2, D] array of sums is required")
    D = s.shape[1]
    n = float(s[D + 1, 0])
    left = float(s[D + 1, 1]) if D > 1 else float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        m = s[D] / n if n >= 1 else np.full(D, np.nan)
        cov = (s[:D] - n * np.outer(m, m)) / (n - 1.0) if n >= 2 else np.full((D, D), np.nan)
    return n, left, m, cov


def _condition(eig):
    """largest / smallest of ascending eigenvalues: inf when the smallest is <= 0, NaN for none."""
    if eig.size == 0 or not np.all(np.isfinite(eig)):
        return float("nan")
    return float(eig[-1] / eig[0]) if eig[0] > 0 else float("inf")


def geometry_from_sums(sums, eps0=None, shift=None):
    """The shape of the posterior, in the coordinates the sums were taken in, from the (all-reduced) [D + 2, D] sums of
    `gram_sums` -> Geometry; pure numpy float64.  shift: what gram_sums subtracted (None: zeros), added back to the mean.
    eps0: the run's per-element base steps; with them the eigenvalues and the condition number of
    diag(1 / eps0) cov diag(1 / eps0), the shape the integrator works in with the run's own steps -- its square root is
    the customary estimate of leapfrogs per independent draw.  A second-order summary pooled over chains: not a local
    metric, and chains that have not converged inflate it.  Degenerate input (no rows, one row, constant columns) gives
    NaN and empty matrices, never an exception."""
    n, left, m, cov = _moments_from_sums(sums)
    D = m.size
    sh = np.zeros(D) if shift is None else _lib.host64(shift).reshape(D)
    var = np.diag(cov).copy()
    ok = np.isfinite(var) & (var > 0)
    kept, out = np.flatnonzero(ok), np.flatnonzero(~ok)
    k = kept.size
    sd_k = np.sqrt(var[kept])
    sd = np.full(D, np.nan)
    sd[kept] = sd_k
    c = cov[np.ix_(kept, kept)]
    c = 0.5 * (c + c.T)
    R = c / np.outer(sd_k, sd_k)
    if k:
        np.fill_diagonal(R, 1.0)
    soft, stiff = np.zeros(D), np.zeros(D)
    eig = np.zeros(0)
    if k and np.all(np.isfinite(R)):
        eig, vec = np.linalg.eigh(R)
        soft[kept], stiff[kept] = vec[:, -1], vec[:, 0]
    elif k:
        eig = np.full(k, np.nan)
    worst, pair = float("nan"), (-1, -1)
    if k >= 2 and np.all(np.isfinite(R)):
        off = np.abs(R - np.diag(np.diag(R)))
        i, j = np.unravel_index(int(off.argmax()), off.shape)
        worst, pair = float(off[i, j]), (int(kept[min(i, j)]), int(kept[max(i, j)]))
    scaled, scaled_cond = None, float("nan")
    if eps0 is not None:
        e = _lib.host64(eps0).reshape(D)[kept]
        with np.errstate(divide="ignore", invalid="ignore"):
            a = c / np.outer(e, e)
        scaled = np.linalg.eigvalsh(a) if k and np.all(np.isfinite(a)) else np.full(k, np.nan)
        scaled_cond = _condition(scaled)
    return Geometry(n, left, sh + m, sd, kept, out, c, R, eig, _condition(eig), soft, stiff, worst, pair, scaled, scaled_cond)


def scale_coupling(rows, mean, sd):
    """The funnel detector's raw sums.  rows: [n, D] (or [S, C, D]) float32 on the GPU; mean, sd: [D] (numpy or tensor),
    pass one's pooled figures.  In float32 on the device u = (x - mean) / sd and v = 0.5 log(u^2 + COUPLING_FLOOR); the
    [2 D + 2, 2 D] float64 sums of `gram_sums` over the [n, 2 D] matrix [u, v] with a NULL shift are returned, so that calls
    and ranks can add them (`coupling_from_sums` turns them into K).  An element whose sd is not finite or not > 0 takes
    u = 0: it is constant and its couplings come out as 0.  A funnel is invisible to linear correlation -- x_j ~ N(0, e^y)
    is uncorrelated with y -- but log |x_j| is linear in y.  2 D <= GRAM_MAX_D."""
    if not (torch.is_tensor(rows) and rows.is_cuda and rows.dtype == torch.float32 and rows.dim() in (2, 3)):
        raise ValueError("scale_coupling: float32 [n, D] rows on the GPU are required (there is no CPU fallback)")
    D = int(rows.shape[-1])
    if 2 * D > GRAM_MAX_D:
        raise ValueError("scale_coupling: at most %d elements" % (GRAM_MAX_D // 2))
    x = rows.reshape(-1, D)
    vec = lambda a: torch.as_tensor(_lib.host64(a).reshape(D)).to(x.device)
    mean64, sd64 = vec(mean), vec(sd)
    ok = torch.isfinite(sd64) & (sd64 > 0) & torch.isfinite(mean64)
    m32 = torch.where(ok, mean64, torch.zeros_like(mean64)).to(torch.float32)
    s32 = torch.where(ok, sd64, torch.ones_like(sd64)).to(torch.float32)
    both = torch.empty(x.shape[0], 2 * D, dtype=torch.float32, device=x.device)
    u = both[:, :D]
    torch.sub(x, m32, out=u)
    u.div_(s32)
    u[:, ~ok] = 0.0
    v = both[:, D:]
    torch.mul(u, u, out=v)
    v.add_(COUPLING_FLOOR).log_().mul_(0.5)
    return gram_sums(both)


def coupling_from_sums(sums):
    """K [D, D] float64 from the (all-reduced) [2 D + 2, 2 D] sums of `scale_coupling`: K[i][j] = the correlation of u_i
    with v_j = log |u_j|, how strongly element i drives the SCALE of element j; the diagonal (an element with its own
    log-magnitude) is set to 0, and so is every entry of an element without a finite, positive variance."""
    n, _, _, cov = _moments_from_sums(sums)
    D = cov.shape[0] // 2
    var = np.diag(cov)
    with np.errstate(divide="ignore", invalid="ignore"):
        K = cov[:D, D:] / np.sqrt(np.outer(var[:D], var[D:]))
    ok = np.isfinite(var) & (var > 0)
    K = np.where(np.outer(ok[:D], ok[D:]) & np.isfinite(K), K, 0.0)
    np.fill_diagonal(K, 0.0)
    return K


# ---- predictive diagnostics: pointwise log-likelihood, PSIS-LOO and WAIC (csrc/loglik.hip, csrc/psis.hip) ----
# An observation table (models.ObservationTable) in device memory: kind, T and N as ints; idx [N, T] int32, w [N, T]
# float32, y, log_scale [N] float32 and scale_idx [N] int32 as contiguous device tensors; y_host: y as numpy float32.
DeviceTable = collections.namedtuple("DeviceTable", ["kind", "T", "N", "idx", "w", "y", "scale_idx", "log_scale", "y_host"])
# Totals of the report (loo_summary), floats: elpd_loo = sum_n elpd_loo_n with se = sqrt(N var_n), p_loo =
# sum_n (lppd_n - elpd_loo_n); elpd_waic_n = lppd_n - p_waic_n likewise, p_waic = sum_n p_waic_n.
LooSummary = collections.namedtuple("LooSummary", ["elpd_loo", "elpd_loo_se", "p_loo", "elpd_waic", "elpd_waic_se", "p_waic"])
PSIS_COLUMNS = ("elpd_loo", "pareto_k", "lppd", "p_waic", "tail_len", "cutoff", "gpd_sigma", "draws_used")
PSIS_MAX_DRAWS = 1 << 24          # the most draws per observation arp_psis_loo takes (csrc/psis.hip: kPsMaxR)
LOGLIK_MAX_D = 255                # the widest state arp_pointwise_loglik takes (csrc/obs_table.h: kObsMaxD)
PARETO_K_CAP = 0.7                # the k-hat above which PSIS is unreliable at any sample size (Vehtari et al. 2024)


def upload_table(table, D, device):
    """models.ObservationTable -> DeviceTable on `device`, checked against a state of D elements: every idx in [0, D),
    every scale_idx in [-1, D) -- the kernel addresses its LDS tile with them."""
    idx = np.ascontiguousarray(table.idx, np.int32)
    w = np.ascontiguousarray(table.w, np.float32)
    if idx.ndim != 2 or idx.shape != w.shape or idx.shape[1] < 1:
        raise ValueError("observation table: idx and w of one [N, T] shape, T >= 1, are required")
    N, T = idx.shape
    y, ls = (np.ascontiguousarray(v, np.float32).reshape(-1) for v in (table.y, table.log_scale))
    si = np.ascontiguousarray(table.scale_idx, np.int32).reshape(-1)
    if not (y.size == N and ls.size == N and si.size == N):
        raise ValueError("observation table: y, scale_idx and log_scale must have one entry per observation")
    if N and (idx.min() < 0 or idx.max() >= D or si.min() < -1 or si.max() >= D):
        raise ValueError("observation table: an index lies outside the state's %d elements" % D)
    if int(table.kind) not in (0, 1):
        raise ValueError("observation table: kind must be 0 (Normal) or 1 (Bernoulli-logit)")
    dev = lambda a: torch.as_tensor(a, device=device)
    return DeviceTable(int(table.kind), int(T), int(N), dev(idx), dev(w), dev(y), dev(si), dev(ls), y)


def _table_call(trace, table, n0, n1, who):
    """How the wrappers over an observation table open -> (view, n0, n1, R): _lib.trace_view's tuple of the trace, the
    resolved observation range and R = S C draws; an empty range or trace is refused."""
    view = _lib.trace_view(trace, who)
    n1 = table.N if n1 is None else int(n1)
    n0 = int(n0)
    if not 0 <= n0 < n1 <= table.N:
        raise ValueError("%s: 0 <= n0 < n1 <= %d observations is required" % (who, table.N))
    R = view[1] * view[2]
    if R == 0 or view[3] == 0:
        raise ValueError("%s: an empty trace" % who)
    return view, n0, n1, R


def _mask_pair(R, dev):
    """(mask [R] uint8, n_masked: an int64 scalar at 0) on `dev`: what every kernel that leaves draws out writes."""
    return torch.empty(R, dtype=torch.uint8, device=dev), torch.zeros((), dtype=torch.int64, device=dev)


def _table_args(view, table, n0, n1):
    """The leading C arguments of those entry points: the trace, the table, the range."""
    x, S, Cn, D, row_stride = view
    return (_lib.ptr(x), S, Cn, D, row_stride, table.kind, _lib.ptr(table.idx), _lib.ptr(table.w), table.T, _lib.ptr(table.y),
            _lib.ptr(table.scale_idx), _lib.ptr(table.log_scale), n0, n1)


def _draw_matrix(t, dtype, rows, R, who, name):
    """`t`, a `dtype` [>= rows, >= R] device matrix with unit column stride -> (t, row stride)."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape[0] >= rows and t.shape[1] >= R
            and t.stride(1) == 1 and (t.stride(0) >= R or t.shape[0] == 1)):
        raise ValueError("%s: %s must be a %s [>= n1 - n0, >= S C] matrix on the GPU with unit column stride"
                         % (who, name, str(dtype).replace("torch.", "")))
    return t, (int(t.stride(0)) if t.shape[0] > 1 else max(R, int(t.shape[1])))


def _obs_workspace_bytes(symbol, N, R, who, most_draws):
    """What the library's sizing function `symbol` asks for N observations of R draws; raises on a shape it refuses."""
    need = int(getattr(_lib.lib(), symbol)(int(N), int(R)))
    if need <= 0:
        raise ValueError("%s: 1 <= N < 2^31 observations of 1 ... %s draws are required" % (who, most_draws))
    return need


def pointwise_loglik(trace, table, n0=0, n1=None, out=None):
    """(ll, mask, n_masked) of `arp_pointwise_loglik` for a recorded CENTRED [S, C, D] float32 trace on the GPU and the
    observations [n0, n1) of a DeviceTable: ll [n1 - n0, S C] float32, ll[n - n0, s C + c] the log-likelihood of
    observation n at draw (s, c); mask [S C] uint8, 1 for a draw with a non-finite element (its ll entries are 0 and not
    to be read); n_masked: their count, an int64 device scalar.  A leading or inner block of chains of a wider trace is
    read in place, as gram_sums reads it.  out: an optional float32 device matrix of at least n1 - n0 rows whose rows are
    at least S C apart, written in place (ll is then a view of it)."""
    view, n0, n1, R = _table_call(trace, table, n0, n1, "pointwise_loglik")
    dev = view[0].device
    if out is None:
        out = torch.empty(n1 - n0, R, dtype=torch.float32, device=dev)
    out, ll_stride = _draw_matrix(out, torch.float32, n1 - n0, R, "pointwise_loglik", "out")
    mask, n_masked = _mask_pair(R, dev)
    _lib.call(dev, _lib.lib().arp_pointwise_loglik, *_table_args(view, table, n0, n1), _lib.ptr(out), ll_stride, _lib.ptr(mask),
              _lib.ptr(n_masked))
    return out[:n1 - n0, :R], mask, n_masked


def psis_workspace_bytes(N, R):
    """Bytes of device workspace `psis_loo` takes for N observations of R draws; raises on a shape that is refused."""
    return _obs_workspace_bytes("arp_psis_workspace_bytes", N, R, "psis_loo", "2^24")


def _ll_matrix(ll, mask, who):
    """ll [N, R] float32 on the GPU as the PSIS entry points read it -> (ll, N, R, row stride): rows at least R apart, a
    contiguous copy otherwise; the optional mask [R] uint8 is checked on the way."""
    if not (torch.is_tensor(ll) and ll.is_cuda and ll.dtype == torch.float32 and ll.dim() == 2):
        raise ValueError("%s: a float32 [N, R] matrix on the GPU is required (there is no CPU fallback)" % who)
    N, R = (int(v) for v in ll.shape)
    if N == 0 or R == 0:
        raise ValueError("%s: an empty matrix" % who)
    if not (ll.stride(1) == 1 and (N == 1 or ll.stride(0) >= R)):
        ll = ll.contiguous()
    _lib.device_operand(mask, torch.uint8, (R,), who, "mask", "R")
    return ll, N, R, (int(ll.stride(0)) if N > 1 else R)


def psis_loo(ll, mask=None):
    """out [N, 8] float64 device tensor of `arp_psis_loo` for ll [N, R] float32 on the GPU (rows may be further apart
    than R), columns PSIS_COLUMNS: per observation elpd_loo, the Pareto k-hat of its importance ratios, lppd, p_waic, the
    tail length M, the cut-off (the largest shifted log ratio not in the tail), the fitted GPD's sigma and the draws
    used.  mask: an optional [R] uint8 device tensor, draws with a non-zero entry are left out (pointwise_loglik's).
    k-hat = +inf where no tail was fitted (M < 5, a constant tail, a non-finite ll).  The workspace is owned here."""
    ll, N, R, stride = _ll_matrix(ll, mask, "psis_loo")
    out = torch.empty(N, 8, dtype=torch.float64, device=ll.device)
    _lib.call(ll.device, _lib.lib().arp_psis_loo, _lib.ptr(ll), N, R, stride, _lib.ptr(mask), _lib.ptr(out),
              workspace=psis_workspace_bytes(N, R))
    return out


def pareto_k_threshold(R):
    """min(1 - 1 / log10(R), 0.7): the k-hat up to which PSIS with R draws is reliable (Vehtari et al. 2024); NaN for R < 2."""
    R = float(R)
    return min(1.0 - 1.0 / np.log10(R), PARETO_K_CAP) if R > 1 else float("nan")


def _se_of_sum(v):
    """sqrt(N var_n(v)), the standard error of sum_n v_n over N observations (var with divisor N - 1); NaN for N < 2."""
    v = np.asarray(v, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return float(np.sqrt(v.size * np.var(v, ddof=1))) if v.size > 1 else float("nan")


def loo_summary(elpd_loo_i, lppd_i, p_waic_i):
    """The totals of the per-observation columns of `psis_loo` -> LooSummary; float64 numpy.  A non-finite column entry
    carries through (a -inf elpd_loo_i makes elpd_loo -inf and its se NaN): nothing is skipped silently."""
    e, l, p = (_lib.host64(v).reshape(-1) for v in (elpd_loo_i, lppd_i, p_waic_i))
    if not (e.size == l.size == p.size):
        raise ValueError("loo_summary: columns of one length are required")
    with np.errstate(invalid="ignore"):
        w = l - p
        return LooSummary(float(e.sum()), _se_of_sum(e), float((l - e).sum()), float(w.sum()), _se_of_sum(w), float(p.sum()))


def loo_compare(a, b):
    """(diff, se_diff) of two models' pointwise elpd over the SAME observations: diff = sum_n (a_n - b_n), se_diff =
    sqrt(N var_n(a_n - b_n)) -- the paired comparison of Vehtari, Gelman, Gabry 2017.  a, b: dicts (or npz files) with
    `elpd_loo_i` and `y`; refused unless N and the observed y agree, since the pairing is what the se rests on."""
    ea, eb = (np.asarray(m["elpd_loo_i"], np.float64).reshape(-1) for m in (a, b))
    ya, yb = (np.asarray(m["y"], np.float64).reshape(-1) for m in (a, b))
    if ea.size != eb.size or ya.size != yb.size or ea.size != ya.size:
        raise ValueError("loo_compare: the two models have different numbers of observations")
    if not np.array_equal(ya, yb):
        raise ValueError("loo_compare: the two models were not fitted to the same observations (y differs)")
    with np.errstate(invalid="ignore"):
        d = ea - eb
        return float(d.sum()), _se_of_sum(d)


# ---- posterior predictive check: replicated observations folded on the device (csrc/ppc.hip) ----
PPC_DRAW_COLUMNS = ("sum_y_rep", "sum_y_rep_sq", "min_y_rep", "max_y_rep", "deviance_rep", "deviance_obs", "sum_mu", "observations")
PPC_OBS_COLUMNS = ("sum_mu", "sum_second_moment", "sum_pit", "count_rep_le_obs")
PPC_STATISTICS = ("mean", "sd", "min", "max", "deviance")
# what ppc_counts returns, in order: draws used, draws left out, then per statistic of PPC_STATISTICS #{T_rep >= T_obs} and
# the sum of T_rep over the draws used, then the sum of the observed deviance -- all additive over draws, hence over ranks
PPC_COUNTS = 2 + 2 * len(PPC_STATISTICS) + 1
# The report (ppc_from_counts).  draws_used, draws_left_out, observations: ints.  p, rep, obs: dicts over PPC_STATISTICS --
# the posterior predictive p-value #{T_rep >= T_obs} / draws_used, the mean of T_rep over the draws used, and T_obs (of y
# itself; for the deviance, a realised discrepancy, the mean over draws of the observed deviance); None where it is not
# defined (no draw used; sd, min and max of Bernoulli data, which are functions of the mean or trivial).
# predictive_mean, predictive_sd, pit, rep_le_obs: [N] float64 per observation (NaN without draws).  pit_ks: the
# Kolmogorov distance of the pit values from uniform; coverage_90: the share of observations with pit in [0.05, 0.95];
# both None for Bernoulli data.
PpcSummary = collections.namedtuple("PpcSummary", ["draws_used", "draws_left_out", "observations", "p", "rep", "obs",
                                                   "predictive_mean", "predictive_sd", "pit", "rep_le_obs", "pit_ks",
                                                   "coverage_90"])


def predictive_workspace_bytes(N, R):
    """Bytes of device workspace `predictive_check` takes for N observations of R draws; raises on a shape that is refused."""
    return _obs_workspace_bytes("arp_predictive_workspace_bytes", N, R, "predictive_check", "2^31 - 1")


def predictive_check(trace, table, n0=0, n1=None, seed=0, draw_offset=0, want_y_rep=False):
    """(draw_stats, obs_sums, y_rep, mask, n_masked) of `arp_predictive_check` for a recorded CENTRED [S, C, D] float32
    trace on the GPU and the observations [n0, n1) of a DeviceTable, all device tensors: draw_stats [S C, 8] float64
    (PPC_DRAW_COLUMNS, per draw over these observations; two ranges combine through `combine_draw_stats`), obs_sums
    [n1 - n0, 4] float64 (PPC_OBS_COLUMNS, per observation over the draws not left out), y_rep [n1 - n0, S C] float32
    with want_y_rep (None otherwise), mask and n_masked as pointwise_loglik's.  The replicated value of (observation n,
    draw r) is a function of (seed, n, draw_offset + r) alone: `draw_offset` is the global number of this trace's first
    draw when the draws of a job are spread over calls or ranks.  A block of chains of a wider trace is read in place;
    the workspace is owned here."""
    view, n0, n1, R = _table_call(trace, table, n0, n1, "predictive_check")
    dev = view[0].device
    if int(draw_offset) < 0:
        raise ValueError("predictive_check: draw_offset >= 0 is required")
    draw_stats = torch.empty(R, len(PPC_DRAW_COLUMNS), dtype=torch.float64, device=dev)
    obs_sums = torch.empty(n1 - n0, len(PPC_OBS_COLUMNS), dtype=torch.float64, device=dev)
    y_rep = torch.empty(n1 - n0, R, dtype=torch.float32, device=dev) if want_y_rep else None
    mask, n_masked = _mask_pair(R, dev)
    _lib.call(dev, _lib.lib().arp_predictive_check, *_table_args(view, table, n0, n1), int(seed) & 0xFFFFFFFFFFFFFFFF,
              int(draw_offset), _lib.ptr(draw_stats), _lib.ptr(obs_sums), _lib.ptr(y_rep), R, _lib.ptr(mask), _lib.ptr(n_masked),
              workspace=predictive_workspace_bytes(n1 - n0, R))
    return draw_stats, obs_sums, y_rep, mask, n_masked


def combine_draw_stats(a, b):
    """The [R, 8] draw statistics of two observation ranges over the same draws as those of their union: columns combine
    by +, +, min, max, +, +, +, +.  Tensors (on one device) or numpy arrays; the result is of the same kind."""
    if tuple(a.shape) != tuple(b.shape) or len(a.shape) != 2 or a.shape[1] != len(PPC_DRAW_COLUMNS):
        raise ValueError("combine_draw_stats: two [R, 8] arrays of one shape are required")
    out = a + b
    if torch.is_tensor(out):
        out[:, 2], out[:, 3] = torch.minimum(a[:, 2], b[:, 2]), torch.maximum(a[:, 3], b[:, 3])
    else:
        out[:, 2], out[:, 3] = np.minimum(a[:, 2], b[:, 2]), np.maximum(a[:, 3], b[:, 3])
    return out


def _ppc_observed(y):
    """T_obs of the first four statistics from y itself, float64 (sd with divisor N - 1, NaN for N < 2)."""
    y = np.asarray(y, np.float64).reshape(-1)
    sd = float(np.std(y, ddof=1)) if y.size > 1 else float("nan")
    return float(y.mean()), sd, float(y.min()), float(y.max())


def _ppc_replicated(c, N):
    """(mean, sd, min, max) of the replicated data set of every row of c, the [R', 8] draw statistics over all N
    observations: mean = c0 / N, sd^2 = (c1 - c0^2 / N) / (N - 1) (NaN for N < 2), min = c2, max = c3.  One definition for
    the p-values (ppc_counts) and the prior predictive quantiles (prior_predictive_summary)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        rep_sd = np.sqrt(np.maximum(c[:, 1] - c[:, 0] * c[:, 0] / N, 0.0) / (N - 1)) if N > 1 else np.full(c.shape[0], np.nan)
        return c[:, 0] / N, rep_sd, c[:, 2], c[:, 3]


def ppc_counts(draw_stats, y, mask=None):
    """The [PPC_COUNTS] float64 vector behind the p-values, from the [R, 8] draw statistics of ALL N observations and the
    observed y [N]: additive over draws, so a job whose draws are spread over ranks adds its ranks' vectors.  mask: [R],
    non-zero for a draw that is left out.  The replicated statistics of draw r: mean = c0 / N, sd^2 = (c1 - c0^2 / N) /
    (N - 1), min = c2, max = c3, deviance = c4, against mean, sd, min, max of y and the draw's own observed deviance c5;
    a tie counts as T_rep >= T_obs.  The kind of data does not enter: ppc_from_counts leaves out what Bernoulli data do
    not define."""
    c = _lib.host64(draw_stats).reshape(-1, len(PPC_DRAW_COLUMNS))
    y = np.asarray(_lib.host64(y), np.float64).reshape(-1)
    N = y.size
    if N < 1:
        raise ValueError("ppc_counts: at least one observation is required")
    used = np.ones(c.shape[0], bool) if mask is None else (_lib.host64(mask).reshape(-1) == 0)
    if used.size != c.shape[0]:
        raise ValueError("ppc_counts: mask must have one entry per draw")
    c = c[used]
    if c.size and not np.all(c[:, 7] == N):
        raise ValueError("ppc_counts: the draw statistics must cover all %d observations" % N)
    out = np.zeros(PPC_COUNTS)
    out[0], out[1] = c.shape[0], used.size - c.shape[0]
    obs_mean, obs_sd, obs_min, obs_max = _ppc_observed(y)
    with np.errstate(divide="ignore", invalid="ignore"):
        rep_mean, rep_sd, rep_min, rep_max = _ppc_replicated(c, N)
        pairs = ((rep_mean, obs_mean), (rep_sd, obs_sd), (rep_min, obs_min), (rep_max, obs_max), (c[:, 4], c[:, 5]))
        for j, (rep, obs) in enumerate(pairs):
            out[2 + j] = np.sum(rep >= obs)
            out[2 + len(pairs) + j] = np.sum(rep)
    out[2 + 2 * len(PPC_STATISTICS)] = np.sum(c[:, 5])
    return out


def _pit_calibration(pit):
    """(pit_ks, coverage_90) of a non-empty vector of PIT values: the Kolmogorov distance of their empirical distribution
    from the uniform, and the share of them in [0.05, 0.95].  One definition for the posterior PIT (ppc_from_counts) and
    the leave-one-out PIT (loo_predictive_summary)."""
    return kolmogorov_distance(pit), float(np.mean((pit >= 0.05) & (pit <= 0.95)))


def kolmogorov_distance(u):
    """The Kolmogorov distance sup |F_n - F| of the empirical distribution of a non-empty vector of values in [0, 1]
    from the uniform one.  The one definition behind ppc_pit_ks, loo_pit_ks and sbc_summary's ks."""
    s = np.sort(u)
    i = np.arange(1, s.size + 1, dtype=np.float64)
    return float(max(np.max(i / s.size - s), np.max(s - (i - 1.0) / s.size)))


def ppc_from_counts(counts, obs_sums, y, kind):
    """The report from the (all-reduced) vector of `ppc_counts`, the (all-reduced) [N, 4] obs_sums and y -> PpcSummary;
    pure numpy float64.  Never raises on a job without a usable draw: everything is then None or NaN."""
    t = np.asarray(counts, np.float64).reshape(PPC_COUNTS)
    o = _lib.host64(obs_sums).reshape(-1, len(PPC_OBS_COLUMNS))
    y = np.asarray(_lib.host64(y), np.float64).reshape(-1)
    if o.shape[0] != y.size:
        raise ValueError("ppc_from_counts: obs_sums must have one row per observation")
    used, left = int(round(t[0])), int(round(t[1]))
    normal = int(kind) == 0
    defined = {"mean": True, "sd": normal and y.size > 1, "min": normal, "max": normal, "deviance": True}
    obs_first = dict(zip(PPC_STATISTICS[:4], _ppc_observed(y))) if y.size else {}
    k = len(PPC_STATISTICS)
    p, rep, obs = {}, {}, {}
    for j, name in enumerate(PPC_STATISTICS):
        ok = defined[name] and used > 0
        p[name] = float(t[2 + j] / used) if ok else None
        rep[name] = float(t[2 + k + j] / used) if ok else None
        obs[name] = (float(t[2 + 2 * k] / used) if ok else None) if name == "deviance" else \
            (obs_first.get(name) if defined[name] else None)
    with np.errstate(divide="ignore", invalid="ignore"):
        nan = np.full(y.size, np.nan)
        mean = o[:, 0] / used if used else nan
        sd = np.sqrt(np.maximum(o[:, 1] / used - mean * mean, 0.0)) if used else nan
        pit = o[:, 2] / used if used else nan
        le = o[:, 3] / used if used else nan
    ks, coverage = _pit_calibration(pit) if normal and used and y.size else (None, None)
    return PpcSummary(used, left, int(y.size), p, rep, obs, mean, sd, pit, le, ks, coverage)


def ppc_summary(draw_stats, obs_sums, y, kind, mask=None):
    """The posterior predictive check of one process, the single place where its statistics are defined -> PpcSummary;
    pure numpy float64.  draw_stats [R, 8] over ALL N observations (PPC_DRAW_COLUMNS), obs_sums [N, 4]
    (PPC_OBS_COLUMNS), y [N], kind 0 (Normal) or 1 (Bernoulli-logit), mask [R] (non-zero: the draw is left out of R_used).
    Test statistics T in PPC_STATISTICS: T_obs of mean, sd (divisor N - 1), min and max from y itself; the observed
    deviance is per draw (a realised discrepancy); p_T = #{r used: T_rep,r >= T_obs(,r)} / R_used, a tie counting as >=.
    For Bernoulli data sd, min and max are functions of the mean or trivial: None.  Per observation: the predictive mean,
    the predictive sd sqrt(E[mu^2 + var] - mean^2), the posterior PIT (the leave-one-out PIT: loo_predictive) and its empirical
    counterpart #{y_rep <= y} / R_used.  Calibration, Normal data only: pit_ks and coverage_90.  = ppc_from_counts of
    ppc_counts: a job whose draws are spread over ranks adds the counts and obs_sums of its ranks first."""
    return ppc_from_counts(ppc_counts(draw_stats, y, mask), obs_sums, y, kind)


# ---- grouped predictive check: the same replicated data folded per group of observations (csrc/ppc_group.hip) ----
GROUPS_FLAG = "--predictive_checks_groups"
# order [n_grouped] and group_start [G + 1] int32 on the device (include/autoreparam.h: arp_group_predictive_check);
# sizes [G]: the groups' sizes, host int64
DeviceGroups = collections.namedtuple("DeviceGroups", ["G", "n_obs", "n_grouped", "order", "group_start", "sizes"])
# Per group ([G] float64 arrays in dicts over PPC_STATISTICS, NaN where ppc_from_counts says None): p, rep, obs as
# PpcSummary's, each over the observations of one group; draws_used, draws_left_out: ints, of the whole job; sizes [G] int64
PpcGroupSummary = collections.namedtuple("PpcGroupSummary", ["draws_used", "draws_left_out", "sizes", "p", "rep", "obs"])


def group_selection(table, spec, part, flag=GROUPS_FLAG):
    """(group_of [N] int32, names) -- THE grouping rule of the grouped predictive check (--predictive_checks_groups=PART):
    the groups are the elements of the latent part `part` of `spec` (anything with part_names, part_shapes and offsets),
    group_of[n] is the element of it that the linear predictor of observation n of `table` (ModelSpec.observation_table)
    reads with a non-zero weight, -1 when it reads none (such an observation is in no group); names: one per element, as
    the geometry report names them (`m[17]`).  An element nobody reads is an empty group.  Pure numpy.  Refused, by a
    ValueError that names the flag: a name that is no part; a part of one element (that is the whole-data check); a part
    no observation reads; a part of which some observation reads more than one element (beta of German credit: a
    regression coefficient groups nothing).  flag: the flag the messages name (--loo_groups groups by the same rule)."""
    from .report_common import element_names
    names = list(spec.part_names)
    if part not in names:
        raise ValueError("%s: %s is no latent part of %s; its parts: %s" % (flag, part, spec.name, ", ".join(names)))
    k = names.index(part)
    lo, hi = int(spec.offsets[k]), int(spec.offsets[k + 1])
    if hi - lo < 2:
        raise ValueError("%s: %s has one element, so its one group is all the data: %s" % (
            flag, part, "that is --predictive_checks itself" if flag == GROUPS_FLAG else "leaving it out leaves nothing to predict it from"))
    idx, w = np.asarray(table.idx, np.int64), np.asarray(table.w)
    reads = (w != 0) & (idx >= lo) & (idx < hi)
    if not reads.any():
        raise ValueError("%s: no observation's linear predictor reads %s" % (flag, part))
    first = np.where(reads, idx - lo, hi - lo).min(axis=1)
    last = np.where(reads, idx - lo, -1).max(axis=1)
    several = np.flatnonzero(reads.any(axis=1) & (first != last))
    if several.size:
        raise ValueError("%s: %d observation(s) read more than one element of %s (the first: observation %d), so its elements "
                         "do not group the data" % (flag, several.size, part, int(several[0])))
    return last.astype(np.int32), element_names(spec)[lo:hi]


def group_order(group_of, n_groups):
    """(order [n_grouped], group_start [n_groups + 1]) int32 of group_of [N] (entries in [-1, n_groups)): the grouped
    observations sorted by group, ascending observation index within a group, and where every group's stretch begins."""
    group_of = np.asarray(group_of, np.int64).reshape(-1)
    G = int(n_groups)
    if G < 1 or (group_of.size and (group_of.min() < -1 or group_of.max() >= G)):
        raise ValueError("group_order: group_of entries in [-1, %d) and at least one group are required" % G)
    grouped = np.flatnonzero(group_of >= 0)
    order = grouped[np.argsort(group_of[grouped], kind="stable")]
    start = np.concatenate([[0], np.cumsum(np.bincount(group_of[grouped], minlength=G))])
    return order.astype(np.int32), start.astype(np.int32)


def upload_groups(order, group_start, n_obs, device):
    """order and group_start (group_order's) -> DeviceGroups on `device`, checked against a table of n_obs observations
    first, as upload_table checks idx: every order entry in [0, n_obs), group_start ascending from 0 to len(order) -- the
    kernel addresses the table and `order` with them."""
    order = np.ascontiguousarray(order, np.int32).reshape(-1)
    start = np.ascontiguousarray(group_start, np.int32).reshape(-1)
    n_obs = int(n_obs)
    if start.size < 2:
        raise ValueError("observation groups: at least one group is required (group_start has n_groups + 1 entries)")
    if order.size and (order.min() < 0 or order.max() >= n_obs):
        raise ValueError("observation groups: an order entry lies outside the table's %d observations" % n_obs)
    if start[0] != 0 or start[-1] != order.size or np.any(np.diff(start.astype(np.int64)) < 0):
        raise ValueError("observation groups: group_start must ascend from 0 to the %d grouped observations" % order.size)
    dev = lambda a: torch.as_tensor(a, device=device)
    # (an empty order still needs an address: one unread entry)
    return DeviceGroups(int(start.size - 1), n_obs, int(order.size), dev(order if order.size else np.zeros(1, np.int32)),
                        dev(start), np.diff(start.astype(np.int64)))


def _group_call(trace, table, groups, g0, g1, who):
    """How the wrappers over the groups of a whole observation table open -> (view, g0, g1, R): _table_call over the whole
    table, the resolved group range; groups of another table or an empty range are refused."""
    view, _, _, R = _table_call(trace, table, 0, None, who)
    g1 = groups.G if g1 is None else int(g1)
    g0 = int(g0)
    if groups.n_obs != table.N:
        raise ValueError("%s: the groups were uploaded for a table of %d observations, not %d" % (who, groups.n_obs, table.N))
    if not 0 <= g0 < g1 <= groups.G:
        raise ValueError("%s: 0 <= g0 < g1 <= %d groups is required" % (who, groups.G))
    return view, g0, g1, R


def group_predictive_check(trace, table, groups, g0=0, g1=None, seed=0, draw_offset=0):
    """(group_stats, mask, n_masked) of `arp_group_predictive_check` for a recorded CENTRED [S, C, D] float32 trace on the
    GPU, a DeviceTable (whole) and the groups [g0, g1) of a DeviceGroups over it, all device tensors: group_stats
    [g1 - g0, S C, 8] float64, PPC_DRAW_COLUMNS over the observations of one group (an empty group: 0, 0, +inf, -inf, 0,
    0, 0, 0; a draw left out: a zero row); mask, n_masked as predictive_check's.  The replicated value of (observation n,
    draw r) is predictive_check's under the same seed and draw_offset, bit for bit, and a group's row depends neither on
    [g0, g1) nor on how the draws are spread over calls.  A block of chains of a wider trace is read in place."""
    who = "group_predictive_check"
    view, g0, g1, R = _group_call(trace, table, groups, g0, g1, who)
    dev = view[0].device
    if int(draw_offset) < 0:
        raise ValueError("%s: draw_offset >= 0 is required" % who)
    stats = torch.empty(g1 - g0, R, len(PPC_DRAW_COLUMNS), dtype=torch.float64, device=dev)
    mask, n_masked = _mask_pair(R, dev)
    _lib.call(dev, _lib.lib().arp_group_predictive_check, *_table_args(view, table, 0, table.N)[:-2], table.N,
              _lib.ptr(groups.order), groups.n_grouped, _lib.ptr(groups.group_start), groups.G, g0, g1,
              int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw_offset), _lib.ptr(stats), _lib.ptr(mask), _lib.ptr(n_masked))
    return stats, mask, n_masked


def ppc_group_counts(group_stats, y, group_of, mask=None, g0=0):
    """[G', PPC_COUNTS] float64: row i is ppc_counts(group_stats[i], y[group_of == g0 + i], mask) -- the one definition of
    the statistics (_ppc_replicated, _ppc_observed), applied to the observations of one group -- for the [G', R, 8]
    statistics of the groups g0 ... g0 + G' - 1 (group_predictive_check).  An empty group yields a zero row; a group of one
    has no sd (NaN compares false: its count is 0, and ppc_from_counts leaves it out).  Additive over draws, as
    ppc_counts is."""
    c = _lib.host64(group_stats)
    if c.ndim != 3 or c.shape[2] != len(PPC_DRAW_COLUMNS):
        raise ValueError("ppc_group_counts: [G, R, 8] group statistics are required")
    y = np.asarray(_lib.host64(y), np.float64).reshape(-1)
    group_of = np.asarray(group_of).reshape(-1)
    if group_of.size != y.size:
        raise ValueError("ppc_group_counts: group_of must have one entry per observation")
    mask = None if mask is None else _lib.host64(mask)                         # (one copy from the device, not one per group)
    out = np.zeros((c.shape[0], PPC_COUNTS))
    for i in range(c.shape[0]):
        members = y[group_of == int(g0) + i]
        if members.size:
            out[i] = ppc_counts(c[i], members, mask)
    return out


def ppc_group_summary(counts, y, group_of, kind):
    """The per-group report from the (all-reduced) [G, PPC_COUNTS] counts of `ppc_group_counts` -> PpcGroupSummary: every
    group's p, rep and obs are ppc_from_counts' of its own counts and observations (its rules: no sd for a group of one
    or for Bernoulli data, nothing without a draw), NaN where that says None -- so an empty group is NaN throughout."""
    counts = np.asarray(counts, np.float64).reshape(-1, PPC_COUNTS)
    y = np.asarray(_lib.host64(y), np.float64).reshape(-1)
    group_of = np.asarray(group_of).reshape(-1)
    G = counts.shape[0]
    p, rep, obs = ({name: np.full(G, np.nan) for name in PPC_STATISTICS} for _ in range(3))
    sizes = np.bincount(group_of[group_of >= 0], minlength=G).astype(np.int64)
    for g in range(G):
        members = y[group_of == g]
        s = ppc_from_counts(counts[g], np.zeros((members.size, len(PPC_OBS_COLUMNS))), members, kind)
        for name in PPC_STATISTICS:
            for to, frm in ((p, s.p), (rep, s.rep), (obs, s.obs)):
                if frm[name] is not None:
                    to[name][g] = frm[name]
    filled = np.flatnonzero(sizes > 0)
    used = int(round(counts[filled[0], 0])) if filled.size else 0
    left = int(round(counts[filled[0], 1])) if filled.size else 0
    return PpcGroupSummary(used, left, sizes, p, rep, obs)


# ---- leave-one-group-out cross-validation: the group log-likelihood, conditional and marginal (csrc/logo.hip) ----
LOGO_FLAG = "--loo_groups"
# DeviceGroups' fields and, on the device, slope [n_grouped] float32 parallel to order and elem [G] int32
# (include/autoreparam.h: arp_group_loglik)
DeviceLogoGroups = collections.namedtuple("DeviceLogoGroups", DeviceGroups._fields + ("slope", "elem"))
# total: the LooSummary of the non-empty groups' rows (elpd_loo, its se OVER GROUPS, p_loo, and the marginal or conditional
# group WAIC); groups, empty: ints
LogoSummary = collections.namedtuple("LogoSummary", ["total", "groups", "empty"])


def marginal_selection(site_table, table, spec, part):
    """(group_of [N] int32, names, slope [N] float32, elem [G] int32, marginal_ok, why) for leave-one-group-out by the
    elements of the latent part `part` (--loo_groups=PART): group_of and names are group_selection's (its refusals name
    --loo_groups), slope[n] is the sum of the weights with which observation n reads its group's element (0 for an
    observation in no group), elem[g] the index of group g's element in the state.  marginal_ok: whether the MARGINAL
    group likelihood -- the element integrated against its conditional prior N(loc, exp(s)) of `site_table`
    (ModelSpec.site_table) -- has the closed form arp_group_loglik computes; `why` says why not (None otherwise): Bernoulli
    data; an element whose site is not of the form SITE_NORMAL; an element that a later site reads with a non-zero weight
    (not a leaf: integrating it changes that site's density too); an observation whose scale reads an element of the part
    (the likelihood is then not Gaussian in it).  The conditional form needs none of these.  Pure numpy."""
    group_of, names = group_selection(table, spec, part, flag=LOGO_FLAG)
    k = list(spec.part_names).index(part)
    lo, hi = int(spec.offsets[k]), int(spec.offsets[k + 1])
    idx, w = np.asarray(table.idx, np.int64), np.asarray(table.w, np.float32).astype(np.float64)
    own = (idx == (lo + group_of.astype(np.int64))[:, None]) & (group_of >= 0)[:, None]
    slope = np.where(own, w, 0.0).sum(axis=1).astype(np.float32)
    elem = np.arange(lo, hi, dtype=np.int32)
    form = np.asarray(site_table.form, np.int64).reshape(-1)
    inside = lambda i: (np.asarray(i, np.int64) >= lo) & (np.asarray(i, np.int64) < hi)
    reads_loc = (np.asarray(site_table.loc_w) != 0) & inside(site_table.loc_idx) & (form != 2)[:, None]
    reads_scale = (np.asarray(site_table.scale_w) != 0) & inside(site_table.scale_idx)
    children = np.flatnonzero(reads_loc.any(axis=1) | reads_scale.any(axis=1))
    scaled = np.flatnonzero(inside(np.asarray(table.scale_idx).reshape(-1)))
    why = None
    if int(table.kind) != 0:
        why = "the data are Bernoulli: the marginal group likelihood has no closed form (quadrature is not implemented)"
    elif np.any(form[lo:hi] != 0):
        why = "the prior of %s is not a Normal with scale exp(s) (site form %d)" % (part, int(form[lo:hi][form[lo:hi] != 0][0]))
    elif children.size:
        why = "%s is not a leaf: the site of element %d reads it, so integrating it changes that density too" % (
            part, int(children[0]))
    elif scaled.size:
        why = "the scale of observation %d reads %s: the likelihood is not Gaussian in it" % (int(scaled[0]), part)
    return group_of, names, slope, elem, why is None, why


def upload_logo_groups(order, group_start, slope, elem, n_obs, D, device):
    """upload_groups(order, group_start, n_obs, device), its checks included, plus `slope` -- [n_obs] float32, one per
    OBSERVATION (marginal_selection's); it is uploaded in order's sequence, slope[order] -- and `elem` [G] int32, every
    entry in [0, D): the kernel addresses its tile and the site table with it -> DeviceLogoGroups."""
    g = upload_groups(order, group_start, n_obs, device)
    slope = np.ascontiguousarray(slope, np.float32).reshape(-1)
    elem = np.ascontiguousarray(elem, np.int32).reshape(-1)
    if slope.size != g.n_obs or not np.all(np.isfinite(slope)):
        raise ValueError("observation groups: slope must have one finite entry per observation (%d)" % g.n_obs)
    if elem.size != g.G or elem.min() < 0 or elem.max() >= int(D):
        raise ValueError("observation groups: elem must have one entry per group (%d) inside the state's %d elements" % (g.G, int(D)))
    in_order = slope[np.ascontiguousarray(order, np.int64).reshape(-1)] if g.n_grouped else np.zeros(1, np.float32)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)
    return DeviceLogoGroups(*g, dev(in_order), dev(elem))


def group_loglik(trace, table, groups, site=None, g0=0, g1=None, out=None):
    """(lc, lm or None, mask, n_masked) of `arp_group_loglik` for a recorded CENTRED [S, C, D] float32 trace on the GPU, a
    DeviceTable (whole) and the groups [g0, g1) of a DeviceLogoGroups over it: lc [g1 - g0, S C] float32, the CONDITIONAL
    log-likelihood of group g at draw r -- float32 of the float64 sum, ascending, of pointwise_loglik's values of the
    group's observations; lm, with `site` (a DeviceSiteTable) and Normal data, the MARGINAL one: the group's element
    integrated against its conditional prior in closed form, float64 behind the per-observation float32 values.  An empty
    group and a draw left out are 0 in both; mask, n_masked as pointwise_loglik's.  A row depends neither on [g0, g1) nor
    on how the draws are spread over calls; without `site` lc is bitwise the same.  A block of chains of a wider trace is
    read in place.  out: an optional float32 device matrix with unit column stride whose rows are at least S C apart, of
    at least g1 - g0 rows (2 (g1 - g0) with `site`: lc is a view of the first g1 - g0, lm of the next)."""
    who = "group_loglik"
    if not isinstance(groups, DeviceLogoGroups):
        raise ValueError("%s: a DeviceLogoGroups is required (upload_logo_groups)" % who)
    view, g0, g1, R = _group_call(trace, table, groups, g0, g1, who)
    dev = view[0].device
    if site is not None and not isinstance(site, DeviceSiteTable):
        raise ValueError("%s: site must be a DeviceSiteTable (upload_site_table)" % who)
    if site is not None and site.D != view[3]:
        raise ValueError("%s: the trace has %d elements, the site table %d" % (who, view[3], site.D))
    n, rows = g1 - g0, (g1 - g0) * (2 if site is not None else 1)
    if out is None:
        out = torch.empty(rows, R, dtype=torch.float32, device=dev)
    out, stride = _draw_matrix(out, torch.float32, rows, R, who, "out")
    lc, lm = out[:n], (out[n:2 * n] if site is not None else None)
    mask, n_masked = _mask_pair(R, dev)
    columns = [getattr(site, name, None) for name in ("loc_idx", "loc_w", "loc0", "scale_idx", "scale_w", "log_scale0")]
    _lib.call(dev, _lib.lib().arp_group_loglik, *_table_args(view, table, 0, table.N)[:-2], table.N, _lib.ptr(groups.order),
              _lib.ptr(groups.slope), groups.n_grouped, _lib.ptr(groups.group_start), _lib.ptr(groups.elem), groups.G, g0, g1,
              *(_lib.ptr(c) for c in columns), _lib.ptr(lc), _lib.ptr(lm), stride, _lib.ptr(mask), _lib.ptr(n_masked))
    return lc[:, :R], (None if lm is None else lm[:, :R]), mask, n_masked


def logo_summary(columns):
    """The totals of leave-one-group-out from the [G, 8] per-group columns of psis_loo (host float64; an EMPTY group is a
    row of NaN throughout) -> LogoSummary: loo_summary over the rows of the non-empty groups -- so its standard errors are
    over groups, sqrt(G' var_g) -- and the counts.  A non-finite entry of a non-empty group carries through, as in
    loo_summary."""
    c = np.asarray(_lib.host64(columns), np.float64).reshape(-1, len(PSIS_COLUMNS))
    empty = np.all(np.isnan(c), axis=1)
    f = c[~empty]
    return LogoSummary(loo_summary(f[:, 0], f[:, 2], f[:, 3]), int(c.shape[0]), int(empty.sum()))


# ---- moment matching for a high Pareto k-hat (csrc/mmatch.hip; Paananen, Piironen, Buerkner, Vehtari 2021) ----
MM_FLAG = "--loo_moment_match"
MM_MAX_ITERATIONS = 30            # the most maps accepted per target (loo::loo_moment_match's max_iters)
MM_MAX_D = 255                    # the widest matrix arp_weighted_moments and arp_affine_rows take
MM_MAX_TARGETS = 4096             # the most targets they take in one call
MM_HEAD = ("lw_max", "sum_w", "sum_w_sq", "draws_kept")        # in front of the D pairs (sum w e, sum w e^2) of a row
# What moment_match returns, one entry per target, host numpy: attempted [T] bool (the plain k-hat was above the threshold);
# elpd [T] (the split's where a map was accepted, the plain one otherwise); pareto_k (the loop's final k-hat; the plain one
# where nothing was accepted or attempted); pareto_k_full (the k-hat of the full posterior's ratios under the last accepted
# map; 0 where attempted and nothing was accepted), pareto_k_split, is_ess (of the split's weights) -- NaN where they do not
# exist; iterations [T] int (maps accepted) and maps [T] str ("112": T1, T1, T2); scale, shift [T, D]: S and U - m0 of
# theta = (x - m0) S + U, NaN where not attempted; centre [D]: m0.
MomentMatch = collections.namedtuple("MomentMatch", ["attempted", "elpd", "pareto_k", "pareto_k_full", "pareto_k_split", "is_ess",
                                                     "iterations", "maps", "scale", "shift", "centre"])


def _mm_rows(x, who):
    """x, a float32 [R, D] device matrix with unit column stride, read in place -> (x, R, D, row stride)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.numel() > 0):
        raise ValueError("%s: a non-empty float32 [R, D] matrix on the GPU is required (there is no CPU fallback)" % who)
    R, D = (int(v) for v in x.shape)
    if not (x.stride(1) == 1 and (R == 1 or x.stride(0) >= D)):
        x = x.contiguous()
    if D > MM_MAX_D:
        raise ValueError("%s: at most %d columns" % (who, MM_MAX_D))
    return x, R, D, (int(x.stride(0)) if R > 1 else D)


def _mm_targets(B, who):
    if not 1 <= int(B) <= MM_MAX_TARGETS:
        raise ValueError("%s: 1 ... %d targets per call are required" % (who, MM_MAX_TARGETS))
    return int(B)


def weighted_moments_workspace_bytes(R, D, B):
    """Bytes of device workspace `weighted_moments` takes for B targets over [R, D]; raises on a shape that is refused."""
    need = int(_lib.lib().arp_weighted_moments_workspace_bytes(int(R), int(D), int(B)))
    if need <= 0:
        raise ValueError("weighted_moments: 1 <= R < 2^31 rows, 1 <= D <= %d and 1 ... %d targets are required" % (MM_MAX_D, MM_MAX_TARGETS))
    return need


def weighted_moments(x, lw, centre):
    """out [B, 4 + 2 D] float64 device tensor of `arp_weighted_moments`: x [R, D] float32 on the GPU (rows may be further
    apart than D, read in place), lw [B, R] float64 log weights (-inf: the draw is left out; arp_psis_weights' layout, rows
    may be further apart than R), centre [D] float32.  Row b: MM_HEAD, then per column the pair sum w e, sum w e^2 with
    w = exp(lw - lw_max) and e = x - centre, float64.  The workspace is owned here."""
    who = "weighted_moments"
    x, R, D, stride = _mm_rows(x, who)
    lw, lw_stride = _draw_matrix(lw, torch.float64, 1, R, who, "lw")
    if lw.shape[1] != R:
        raise ValueError("%s: lw must have one column per row of x" % who)
    B = _mm_targets(lw.shape[0], who)
    _lib.device_operand(centre, torch.float32, (D,), who, "centre", "D")
    if centre is None:
        raise ValueError("%s: centre is required" % who)
    out = torch.empty(B, len(MM_HEAD) + 2 * D, dtype=torch.float64, device=x.device)
    _lib.call(x.device, _lib.lib().arp_weighted_moments, _lib.ptr(x), R, D, stride, _lib.ptr(lw), B, lw_stride, _lib.ptr(centre),
              _lib.ptr(out), workspace=weighted_moments_workspace_bytes(R, D, B))
    return out


def affine_rows_bytes(R, D, B):
    """Bytes of the [B, R, D] float32 output of `affine_rows`."""
    return 4 * int(R) * int(D) * int(B)


def affine_rows(x, m, s, u, parity=-1, out=None):
    """out [B, R, D] float32 device tensor of `arp_affine_rows`: out[b, r] = (x[r] - m[b]) * s[b] + u[b], three float32
    roundings in that order, for every row (parity < 0) or the rows with (r & 1) == parity; the other rows are copies of
    x's, bit for bit.  x [R, D] float32 on the GPU, read in place; m, s, u [B, D] float32 contiguous.  out: an optional
    contiguous float32 tensor of at least B R D elements, written in place (the result is a view of it)."""
    who = "affine_rows"
    x, R, D, stride = _mm_rows(x, who)
    if not (torch.is_tensor(m) and m.dim() == 2 and m.shape[1] == D):
        raise ValueError("%s: m, s and u must be float32 [B, D] tensors on the GPU" % who)
    B = _mm_targets(m.shape[0], who)
    for name, t in (("m", m), ("s", s), ("u", u)):
        if t is None:
            raise ValueError("%s: %s is required" % (who, name))
        _lib.device_operand(t, torch.float32, (B, D), who, name, "B, D")
    parity = int(parity)
    if parity > 1:
        raise ValueError("%s: parity must be negative (every row), 0 or 1" % who)
    if out is None:
        out = torch.empty(B, R, D, dtype=torch.float32, device=x.device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= B * R * D):
        raise ValueError("%s: out must be a contiguous float32 tensor of at least B R D elements on the GPU" % who)
    res = out.reshape(-1)[:B * R * D].view(B, R, D)
    _lib.call(x.device, _lib.lib().arp_affine_rows, _lib.ptr(x), R, D, stride, _lib.ptr(m), _lib.ptr(s), _lib.ptr(u), B, parity,
              _lib.ptr(res))
    return res


def _mm_ratio_rows(rho, kept):
    """Log ratios rho [n, R] float64 as psis_weights reads them: the NEGATED ratio in float32, about each row's mean over
    the kept draws (it cancels; float32 then resolves the ratios and not their size -- powerscale_lw's rule).  A row with a
    non-finite kept ratio comes out non-finite and is not fitted."""
    zero = torch.zeros_like(rho)
    centre = torch.where(kept[None], rho, zero).sum(dim=1, keepdim=True) / kept.sum().clamp(min=1)
    return (-torch.where(kept[None], rho - centre, zero)).to(torch.float32).contiguous()


def _mm_moments(sums, D):
    """(mean [n, D], variance [n, D], sum w, sum w^2, lw_max) of e = x - centre from rows of weighted_moments, host float64."""
    with np.errstate(all="ignore"):
        sw = sums[:, 1:2]
        pairs = sums[:, len(MM_HEAD):].reshape(-1, D, 2)
        mean = pairs[:, :, 0] / sw
        return mean, pairs[:, :, 1] / sw - mean * mean, sums[:, 1], sums[:, 2], sums[:, 0]


def moment_match(x, left, logp_fn, loglik_fn, targets, plain_k, plain_elpd, threshold, batch=1):
    """Implicitly adaptive importance sampling (Paananen, Piironen, Buerkner, Vehtari 2021; loo::loo_moment_match with
    its maps T1 and T2 and the split of its section 4) for the targets whose plain Pareto k-hat is above `threshold` ->
    MomentMatch.  THE definition of the algorithm here; the reports only feed it.
      x [R, D] float32 on the GPU: the draws, in coordinates where every element is unconstrained (the centred trace);
      left [R] bool or uint8 on the GPU: draws that are left out of everything;
      logp_fn(rows [n, D] float32) -> [n]: the log joint density of the full posterior up to a constant;
      loglik_fn(target, rows [n, D]) -> [n]: the log-likelihood term that leaving `target` out removes;
      targets: T labels handed to loglik_fn; plain_k, plain_elpd [T]: their plain PSIS figures;
      batch: targets per call of the kernels (report_common.mm_batch_size).
    State.  m0 = float32 of the unweighted mean of the kept draws (one weighted_moments call with zero log weights about
    0); L0 = logp_fn(x); l0 = loglik_fn(t, x).  The draws of a target are always the TOTAL map applied to the original
    ones, theta = (x - m0) S + U (S = 1, U = m0 at the start; float64 on the host, rounded to float32 once per affine_rows
    call), so no rounding accumulates.  The weighted (rows lw) and unweighted (a row of zeros) mean and variance of theta
    come from one weighted_moments call on x about m0, mapped through (S, U) on the host.
    Loop, per target, from (lw, k) = psis_weights(l0) and k_f = 0, while k > threshold and fewer than MM_MAX_ITERATIONS
    maps are accepted:  T1: U' = U + (mu_w - mu);  refused -> T2, f = sqrt(v_w / v): S' = S f, U' = (U - mu) f + mu_w.  A
    candidate's ratios rho = -l' + L' - L0 and rho_f = L' - L0 are smoothed by one psis_weights call; it is accepted iff
    k' < k (a non-finite kept ratio gives k' = +inf).  Both refused: the loop ends.  The Jacobian is constant and cancels.
    Split, where a map was accepted: A = x with the total map on its even rows, B = x with the inverse map
    (x - U) / S + m0 on its odd rows; rho = -l(A) + L(A) - logaddexp(L(A), L(B) - sum_d log S_d), smoothed to lw_s;
    elpd = log sum exp(lw_s + l(A)) - log sum exp(lw_s) and the ESS (sum w)^2 / sum w^2, the sums from weighted_moments.
    Every active target of a batch goes through each kernel call together; a target's figures do not depend on `batch`."""
    who = "moment_match"
    x, R, D, _ = _mm_rows(x, who)
    dev = x.device
    T = len(targets)
    plain_k, plain_elpd = (np.array(_lib.host64(v), np.float64).reshape(-1) for v in (plain_k, plain_elpd))
    if plain_k.size != T or plain_elpd.size != T:
        raise ValueError("%s: plain_k and plain_elpd must have one entry per target" % who)
    batch = _mm_targets(int(batch) + 1, who) - 1                               # (and one row for the unweighted moments)
    threshold = float(threshold)
    with np.errstate(invalid="ignore"):
        attempted = ~(plain_k <= threshold) if np.isfinite(threshold) else ~np.isfinite(plain_k)
    nan = lambda *shape: np.full(shape, np.nan)
    res = MomentMatch(attempted, plain_elpd.copy(), plain_k.copy(), nan(T), nan(T), nan(T), np.zeros(T, np.int64), [""] * T,
                      nan(T, D), nan(T, D), None)
    left = torch.as_tensor(left, device=dev).reshape(-1) != 0
    if left.numel() != R:
        raise ValueError("%s: left must have one entry per draw" % who)
    f64 = lambda t: t.to(torch.float64).reshape(-1)
    L0 = f64(logp_fn(x))
    left = left | ~torch.isfinite(L0)
    kept, mask = ~left, left.to(torch.uint8).contiguous()
    base = torch.where(kept, torch.zeros(R, dtype=torch.float64, device=dev),
                       torch.full((R,), float("-inf"), dtype=torch.float64, device=dev))
    zero_centre = torch.zeros(D, dtype=torch.float32, device=dev)
    m0 = _mm_moments(weighted_moments(x, base[None], zero_centre).cpu().numpy(), D)[0][0].astype(np.float32)
    res = res._replace(centre=m0.astype(np.float64))
    m0_d = torch.as_tensor(m0, device=dev)
    m0 = m0.astype(np.float64)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32), device=dev)
    out_buffer = torch.empty(batch * R * D, dtype=torch.float32, device=dev)

    def densities(ids, rows):
        """(L, l) [n, R] float64 at rows [n, R, D]: one logp_fn call, one loglik_fn call per target."""
        n = len(ids)
        L = f64(logp_fn(rows.view(n * R, D))).view(n, R)
        return L, torch.stack([f64(loglik_fn(targets[t], rows[j])) for j, t in enumerate(ids)])

    def candidates(ids, S, U):
        """The k-hat, the full posterior's k-hat and the log weights of the maps (S, U) [n, D] of the targets `ids`."""
        rows = affine_rows(x, m0_d[None].expand(len(ids), D).contiguous(), up(S), up(U), -1, out=out_buffer)
        L, l = densities(ids, rows)
        rho_f = L - L0[None]
        out8, lw = psis_weights(_mm_ratio_rows(torch.cat([rho_f - l, rho_f]), kept), mask)
        k = out8[:, 1].cpu().numpy()
        return k[:len(ids)], k[len(ids):], lw[:len(ids)]

    todo = [int(t) for t in np.flatnonzero(attempted)]
    for b0 in range(0, len(todo), batch):
        ids = todo[b0:b0 + batch]
        n = len(ids)
        l0 = torch.stack([loglik_fn(targets[t], x).to(torch.float32).reshape(-1) for t in ids]).contiguous()
        out8, lw = psis_weights(l0, mask)
        k = out8[:, 1].cpu().numpy().copy()
        k_f = np.zeros(n)
        S, U = np.ones((n, D)), np.tile(m0, (n, 1))
        maps = [""] * n
        active = [j for j in range(n) if k[j] > threshold or not np.isfinite(k[j])]
        while active:
            sums = weighted_moments(x, torch.cat([lw[active], base[None]]).contiguous(), m0_d).cpu().numpy()
            mean_e, var_e, _, _, _ = _mm_moments(sums, D)
            Sa, Ua = S[active], U[active]
            with np.errstate(all="ignore"):
                mu_w, v_w = mean_e[:-1] * Sa + Ua, var_e[:-1] * Sa * Sa
                mu, v = mean_e[-1:] * Sa + Ua, var_e[-1:] * Sa * Sa
                f = np.sqrt(v_w / v)
            trial = [(Sa, Ua + (mu_w - mu), "1"), (Sa * f, (Ua - mu) * f + mu_w, "2")]
            pending, accepted = list(range(len(active))), []
            for S_c, U_c, name in trial:
                if not pending:
                    break
                pick = [active[i] for i in pending]
                k_c, kf_c, lw_c = candidates([ids[j] for j in pick], S_c[pending], U_c[pending])
                still = []
                for pos, (i, j) in enumerate(zip(pending, pick)):
                    if k_c[pos] < k[j]:
                        S[j], U[j], k[j], k_f[j] = S_c[i], U_c[i], k_c[pos], kf_c[pos]
                        lw[j] = lw_c[pos]
                        maps[j] += name
                        accepted.append(j)
                    else:
                        still.append(i)
                pending = still
            active = [j for j in sorted(accepted) if k[j] > threshold and len(maps[j]) < MM_MAX_ITERATIONS]
        for j, t in enumerate(ids):
            res.pareto_k[t], res.pareto_k_full[t], res.iterations[t], res.maps[t] = k[j], k_f[j], len(maps[j]), maps[j]
            res.scale[t], res.shift[t] = S[j], U[j] - m0
        # the split, for the targets that moved: A and B share the buffer, half a batch at a time
        moved = [j for j in range(n) if maps[j]]
        half = max(1, batch // 2)
        for c0 in range(0, len(moved), half):
            js = moved[c0:c0 + half]
            nj, sub = len(js), [ids[j] for j in js]
            A = affine_rows(x, m0_d[None].expand(nj, D).contiguous(), up(S[js]), up(U[js]), 0, out=out_buffer)
            if batch >= 2:
                B_out = out_buffer[nj * R * D:]
            else:
                B_out = None
            Bm = affine_rows(x, up(U[js]), up(1.0 / S[js]), m0_d[None].expand(nj, D).contiguous(), 1, out=B_out)
            LA, lA = densities(sub, A)
            LB = f64(logp_fn(Bm.view(nj * R, D))).view(nj, R)
            log_det = torch.as_tensor(np.log(S[js]).sum(axis=1), device=dev)[:, None]
            rho = -lA + LA - torch.logaddexp(LA, LB - log_det)
            out8, lw_s = psis_weights(_mm_ratio_rows(rho, kept), mask)
            k_s = out8[:, 1].cpu().numpy()
            lA = torch.where(kept[None], lA, torch.zeros_like(lA))            # (lw_s is -inf there)
            sums = weighted_moments(x, torch.cat([lw_s + lA, lw_s]).contiguous(), m0_d).cpu().numpy()
            with np.errstate(all="ignore"):
                log_sum = sums[:, 0] + np.log(sums[:, 1])
                for pos, t in enumerate(sub):
                    res.elpd[t] = log_sum[pos] - log_sum[nj + pos]
                    res.is_ess[t] = sums[nj + pos, 1] ** 2 / sums[nj + pos, 2]
                    res.pareto_k_split[t] = k_s[pos]
    return res


# ---- leave-one-out predictive report: the predictive quantities folded with the PSIS weights (csrc/loopred.hip) ----
LOO_PRED_COLUMNS = ("sum_w", "sum_w_sq", "sum_w_mu", "sum_w_second_moment", "sum_w_pit", "draws_counted")
# The report (loo_predictive_summary).  observations: those whose four figures are finite; left_out: the others.  loo_mean,
# loo_sd, loo_pit, is_ess: [N] float64 per observation (NaN where there is nothing to divide by).  Floats, None where not
# defined for the data kind or the data: pit_ks, coverage_90, rmse, r2 (Normal); brier, accuracy, balanced_accuracy
# (Bernoulli); is_ess_min and is_ess_min_observation (-1: none) for both.
LooPredSummary = collections.namedtuple("LooPredSummary", ["observations", "left_out", "loo_mean", "loo_sd", "loo_pit", "is_ess",
                                                           "pit_ks", "coverage_90", "rmse", "r2", "brier", "accuracy",
                                                           "balanced_accuracy", "is_ess_min", "is_ess_min_observation"])


def loo_predictive_workspace_bytes(N, R):
    """Bytes of device workspace `loo_predictive` takes for N observations of R draws; raises on a shape that is refused."""
    return _obs_workspace_bytes("arp_loo_predictive_workspace_bytes", N, R, "loo_predictive", "2^31 - 1")


def loo_predictive(trace, table, lw, n0=0, n1=None):
    """obs_sums [n1 - n0, 6] float64 device tensor of `arp_loo_predictive` (LOO_PRED_COLUMNS) for a recorded CENTRED
    [S, C, D] float32 trace on the GPU, the observations [n0, n1) of a DeviceTable and lw, a float64 [>= n1 - n0, >= S C]
    device matrix with unit column stride: lw[n - n0, s C + c] is the log weight of draw (s, c) for observation n
    (psis_weights' lw of pointwise_loglik's ll over the same draws and the same range).  Per observation, over the draws
    with lw != -inf and W = exp(lw): sum W, sum W^2, sum W mu, sum W (mu^2 + var), sum W pit and the draws counted, mu, var
    and pit as predictive_check defines them.  A block of chains of a wider trace is read in place; the workspace is
    owned here."""
    view, n0, n1, R = _table_call(trace, table, n0, n1, "loo_predictive")
    dev = view[0].device
    lw, lw_stride = _draw_matrix(lw, torch.float64, n1 - n0, R, "loo_predictive", "lw")
    obs_sums = torch.empty(n1 - n0, len(LOO_PRED_COLUMNS), dtype=torch.float64, device=dev)
    _lib.call(dev, _lib.lib().arp_loo_predictive, *_table_args(view, table, n0, n1), _lib.ptr(lw), lw_stride,
              _lib.ptr(obs_sums), workspace=loo_predictive_workspace_bytes(n1 - n0, R))
    return obs_sums


def loo_predictive_summary(obs_sums, y, kind):
    """The leave-one-out predictive report, the single place where its statistics are defined -> LooPredSummary; pure
    numpy float64.  obs_sums [N, 6] (LOO_PRED_COLUMNS: S0 ... S5), y [N], kind 0 (Normal) or 1 (Bernoulli-logit).  Per
    observation, the self-normalised importance-sampling estimates under the weights behind the sums (Vehtari, Gelman,
    Gabry 2017): loo_mean = S2 / S0, loo_sd = sqrt(max(S3 / S0 - loo_mean^2, 0)), loo_pit = S4 / S0, is_ess = S0^2 / S1.
    An observation counts when all four are finite; the others are counted as left out and enter no total.  Normal data:
    pit_ks and coverage_90 of the LOO-PIT values (ppc_summary's definition on another input), rmse = sqrt(mean (y -
    loo_mean)^2), r2 = 1 - sum (y - loo_mean)^2 / sum (y - mean y)^2 (None for fewer than two observations or constant y).
    Bernoulli data: brier = mean (y - loo_mean)^2, accuracy = the share with (loo_mean > 0.5) == (y > 0.5),
    balanced_accuracy = the mean of the two per-class shares (None when a class is absent); the mid-p PIT of a binary
    outcome says nothing, so pit_ks and coverage_90 are None, ppc_summary's rule.  Both: is_ess_min and its observation.
    No r_eff, no quantiles, no moment matching; the figures of an observation with a high Pareto k-hat are as unreliable
    as its elpd_loo.  Never raises on degenerate sums: everything is then None or NaN."""
    o = _lib.host64(obs_sums).reshape(-1, len(LOO_PRED_COLUMNS))
    y = np.asarray(_lib.host64(y), np.float64).reshape(-1)
    if o.shape[0] != y.size:
        raise ValueError("loo_predictive_summary: obs_sums must have one row per observation")
    normal = int(kind) == 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mean = o[:, 2] / o[:, 0]
        sd = np.sqrt(np.maximum(o[:, 3] / o[:, 0] - mean * mean, 0.0))
        pit = o[:, 4] / o[:, 0]
        ess = o[:, 0] * o[:, 0] / o[:, 1]
    ok = np.isfinite(mean) & np.isfinite(sd) & np.isfinite(pit) & np.isfinite(ess)
    n = int(ok.sum())
    ks = coverage = rmse = r2 = brier = accuracy = balanced = ess_min = None
    at = -1
    if n:
        yk, mk = y[ok], mean[ok]
        sq = (yk - mk) ** 2
        at = int(np.flatnonzero(ok)[np.argmin(ess[ok])])
        ess_min = float(ess[at])
        if normal:
            ks, coverage = _pit_calibration(pit[ok])
            rmse = float(np.sqrt(np.mean(sq)))
            total = float(np.sum((yk - np.mean(yk)) ** 2))
            r2 = float(1.0 - np.sum(sq) / total) if n >= 2 and total > 0 else None
        else:
            brier = float(np.mean(sq))
            hit = (mk > 0.5) == (yk > 0.5)
            accuracy = float(np.mean(hit))
            pos = yk > 0.5
            balanced = float(0.5 * (np.mean(hit[pos]) + np.mean(hit[~pos]))) if pos.any() and (~pos).any() else None
    return LooPredSummary(n, int(y.size) - n, mean, sd, pit, ess, ks, coverage, rmse, r2, brier, accuracy, balanced, ess_min, at)


# ---- check of a mean-field fit: draws from q, Pareto-smoothed importance ratios, one fold (csrc/vicheck.hip, psis.hip) ----
VI_ELEM_COLUMNS = ("sum_u", "sum_u_sq", "sum_uz", "sum_uz_sq", "sum_u_plus_z_sq", "sum_wz", "sum_wz_sq", "sum_wc", "sum_wc_sq")
VI_TOT_COLUMNS = ("kept", "sum_w", "sum_w_sq", "sum_ll", "min_ll")
VI_MAX_DRAWS = 1 << 24            # the most draws arp_vi_draws and arp_vi_fold take
# What vi_check leaves on the host: elem [D, 9] and tot [5] float64 (arp_vi_fold), out8 [8] float64 (PSIS_COLUMNS of the one
# row of log ratios), e0 [D] float64 (the centred image of loc), logp_const (the density's additive constant), left_out
# (draws with a non-finite logp, gradient or centred element), log_ratio [R] float32 (log p - log q without the constant;
# NaN or +-inf where the draw was left out), log_weight [R] float64 (arp_psis_weights' lw; -inf where left out).
ViCheck = collections.namedtuple("ViCheck", ["elem", "tot", "out8", "e0", "logp_const", "left_out", "log_ratio", "log_weight"])
# The report (vi_check_summary).  Floats, None where not defined: draws, elbo_final, elbo_final_se, pareto_k,
# pareto_k_threshold, tail_length, is_ess, log_evidence, log_evidence_se, kl_estimate, kl_estimate_se; [D] float64:
# elbo_grad_loc, elbo_grad_loc_se, elbo_grad_scale, elbo_grad_scale_se, score_gap, loc_shift, sd_ratio, is_mean, is_sd.
ViCheckSummary = collections.namedtuple("ViCheckSummary", [
    "draws", "elbo_final", "elbo_final_se", "pareto_k", "pareto_k_threshold", "tail_length", "is_ess", "log_evidence",
    "log_evidence_se", "kl_estimate", "kl_estimate_se", "elbo_grad_loc", "elbo_grad_loc_se", "elbo_grad_scale",
    "elbo_grad_scale_se", "score_gap", "loc_shift", "sd_ratio", "is_mean", "is_sd"])


def _rows_out(t, R, D, who, name):
    """`t`, an optional float32 [R, >= D] device matrix with unit column stride that `who` writes in place -> (t, stride)."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] == R
            and t.shape[1] >= D and t.stride(1) == 1 and (R == 1 or t.stride(0) >= t.shape[1])):
        raise ValueError("%s: %s must be a float32 [n_draws, >= D] matrix on the GPU with unit column stride" % (who, name))
    return t, (int(t.stride(0)) if R > 1 else int(t.shape[1]))


def vi_draws(loc, scale, draws, seed=0, draw_offset=0, device=None, out=None):
    """(x, z, logq) of `arp_vi_draws`: `draws` draws x = loc + scale z from the mean-field normal, z [draws, D] float32 the
    standard normals behind them and logq [draws] float64 = log q(x), device tensors.  loc, scale: [D], anything numpy
    reads; a scale that is not finite and positive is refused here, before upload.  Draw r is a function of (seed,
    draw_offset + r) alone.  out: an optional pair (x, z) of float32 [draws, >= D] device matrices of one row stride,
    written in place in their first D columns (the others are not touched)."""
    loc32 = np.ascontiguousarray(_lib.host64(loc).reshape(-1), np.float32)
    scale32 = np.ascontiguousarray(_lib.host64(scale).reshape(-1), np.float32)
    D, R = int(loc32.size), int(draws)
    if D < 1 or scale32.size != D:
        raise ValueError("vi_draws: loc and scale of one length D >= 1 are required")
    if not (np.all(np.isfinite(scale32)) and np.all(scale32 > 0)):
        raise ValueError("vi_draws: every scale must be finite and positive")
    if not 1 <= R <= VI_MAX_DRAWS:
        raise ValueError("vi_draws: 1 <= draws <= 2^24 is required")
    if int(draw_offset) < 0:
        raise ValueError("vi_draws: draw_offset >= 0 is required")
    if out is None:
        if device is None or torch.device(device).type != "cuda":
            raise ValueError("vi_draws: a GPU device is required (there is no CPU fallback)")
        dev = torch.device(device)
        x, z = (torch.empty(R, D, dtype=torch.float32, device=dev) for _ in range(2))
        stride = D
    else:
        (x, stride), (z, zs) = _rows_out(out[0], R, D, "vi_draws", "x"), _rows_out(out[1], R, D, "vi_draws", "z")
        if zs != stride or z.device != x.device:
            raise ValueError("vi_draws: x and z must have one row stride and one device")
        dev = x.device
    logq = torch.empty(R, dtype=torch.float64, device=dev)
    loc_d, scale_d = torch.as_tensor(loc32, device=dev), torch.as_tensor(scale32, device=dev)
    _lib.call(dev, _lib.lib().arp_vi_draws, _lib.ptr(loc_d), _lib.ptr(scale_d), D, R, int(seed) & 0xFFFFFFFFFFFFFFFF,
              int(draw_offset), _lib.ptr(x), _lib.ptr(z), stride, _lib.ptr(logq))
    return x, z, logq


def psis_weights(ll, mask=None):
    """(out, lw) of `arp_psis_weights` for ll [N, R] float32 on the GPU: out [N, 8] float64 is psis_loo's bit for bit, lw
    [N, R] float64 the max-shifted, Pareto-smoothed log weight of every draw (raw where the row was not fitted, -inf for a
    masked draw, NaN throughout the kept draws of a row with a non-finite kept ll).  The workspace is owned here."""
    ll, N, R, stride = _ll_matrix(ll, mask, "psis_weights")
    need = _obs_workspace_bytes("arp_psis_weights_workspace_bytes", N, R, "psis_weights", "2^24")
    out = torch.empty(N, 8, dtype=torch.float64, device=ll.device)
    lw = torch.empty(N, R, dtype=torch.float64, device=ll.device)
    _lib.call(ll.device, _lib.lib().arp_psis_weights, _lib.ptr(ll), N, R, stride, _lib.ptr(mask), _lib.ptr(out), _lib.ptr(lw), R,
              workspace=need)
    return out, lw


def vi_fold(z, grad, e, ll, lw, scale, e0):
    """(elem [D, 9], tot [5]) float64 device tensors of `arp_vi_fold` (VI_ELEM_COLUMNS, VI_TOT_COLUMNS): z, grad, e contiguous
    float32 [R, D] on the GPU, ll [R] float32, lw [R] float64, scale and e0 [D] float32.  The workspace is owned here."""
    if not (torch.is_tensor(z) and z.is_cuda and z.dtype == torch.float32 and z.dim() == 2 and z.is_contiguous()):
        raise ValueError("vi_fold: z must be a contiguous float32 [R, D] matrix on the GPU (there is no CPU fallback)")
    R, D = (int(v) for v in z.shape)
    if R == 0 or D == 0:
        raise ValueError("vi_fold: an empty matrix")
    for name, t, dtype, shape, dims in (("grad", grad, torch.float32, (R, D), "R, D"), ("e", e, torch.float32, (R, D), "R, D"),
                                        ("ll", ll, torch.float32, (R,), "R"), ("lw", lw, torch.float64, (R,), "R"),
                                        ("scale", scale, torch.float32, (D,), "D"), ("e0", e0, torch.float32, (D,), "D")):
        if t is None:
            raise ValueError("vi_fold: %s is required" % name)
        _lib.device_operand(t, dtype, shape, "vi_fold", name, dims)
    need = int(_lib.lib().arp_vi_fold_workspace_bytes(R, D))
    if need <= 0:
        raise ValueError("vi_fold: 1 <= R <= 2^24 draws of 1 <= D <= 2^24 elements are required")
    elem = torch.empty(D, len(VI_ELEM_COLUMNS), dtype=torch.float64, device=z.device)
    tot = torch.empty(len(VI_TOT_COLUMNS), dtype=torch.float64, device=z.device)
    _lib.call(z.device, _lib.lib().arp_vi_fold, _lib.ptr(z), _lib.ptr(grad), _lib.ptr(e), D, _lib.ptr(ll), _lib.ptr(lw),
              _lib.ptr(scale), _lib.ptr(e0), R, D, _lib.ptr(elem), _lib.ptr(tot), workspace=need)
    return elem, tot


def vi_check(eng, loc, scale, which=0, draws=65536, seed=0):
    """The device half of the check of a mean-field normal fit q = N(loc, diag(scale^2)) against the density of
    parameterisation `which` of the engine `eng`, in that parameterisation's coordinates -> ViCheck (host arrays):
    1. x, z, logq of vi_draws; logp and its gradient at x (Engine.logp_grad), the centred image of x and of loc
       (Engine.transform);
    2. ll = float32(logq - float64(logp)), the negated log importance ratio (without the density's constant);
    3. the mask: a draw whose logp, any gradient element or any centred element is not finite is left out and counted;
    4. psis_weights of the one row ll: the Pareto fit of the ratios' tail and every draw's smoothed weight;
    5. vi_fold.
    What the numbers mean is vi_check_summary's business."""
    dev = eng.device
    x, z, logq = vi_draws(loc, scale, draws, seed=seed, device=dev)
    D = int(x.shape[1])
    if D != int(eng.D):
        raise ValueError("vi_check: loc and scale must have the engine's %d elements" % int(eng.D))
    logp, grad = eng.logp_grad(x, which=which)
    e = eng.transform(x, which=which, to_centered=True)
    loc32 = np.ascontiguousarray(_lib.host64(loc).reshape(1, D), np.float32)
    e0 = eng.transform(loc32, which=which, to_centered=True).reshape(D)
    ll = (logq - logp.to(torch.float64)).to(torch.float32)
    bad = ~(torch.isfinite(logp) & torch.isfinite(grad).all(dim=1) & torch.isfinite(e).all(dim=1))
    out8, lw = psis_weights(ll.reshape(1, -1), bad.to(torch.uint8))
    scale_d = torch.as_tensor(np.ascontiguousarray(_lib.host64(scale).reshape(D), np.float32), device=dev)
    elem, tot = vi_fold(z, grad, e, ll, lw.reshape(-1), scale_d, e0.contiguous())
    return ViCheck(_lib.host64(elem), _lib.host64(tot), _lib.host64(out8).reshape(8), _lib.host64(e0),
                   float(eng.logp_const(which)), int(bad.sum().item()), (-ll).cpu().numpy(), _lib.host64(lw).reshape(-1))


def vi_check_summary(elem, tot, out8, loc, scale, e0, logp_const):
    """The check of a mean-field fit, the single place where its statistics are defined -> ViCheckSummary; pure numpy
    float64.  elem [D, 9], tot [5] (arp_vi_fold: VI_ELEM_COLUMNS, VI_TOT_COLUMNS), out8 [8] (PSIS_COLUMNS of the one row of
    negated log ratios ll = log q - log p), loc, scale [D] (q), e0 [D] (the centred image of loc), logp_const (what the
    density leaves out of log p).  With R' = tot[0] kept draws, u = scale_d dlogp/dx_d, w the smoothed importance weights:
      elbo_final = -sum ll / R' + const, the ELBO OF THE FINAL PARAMETERS (not the optimiser's running figure), with
        elbo_final_se = sqrt(var(ll) / R'), var(ll) = out8[3] the two-pass variance;
      pareto_k = out8[1] (None: no tail was fitted) against pareto_k_threshold(R'); tail_length = out8[4];
      is_ess = (sum w)^2 / sum w^2;
      log_evidence = -min ll + log sum w - log R' + const, the importance-sampling estimate of log Z, with
        log_evidence_se = sqrt(1 / is_ess - 1 / R') (the delta method on the self-normalised weights);
      kl_estimate = log_evidence - elbo_final = KL(q || p), kl_estimate_se the root sum of squares of the two se -- both are
        functions of the same draws and their covariance is IGNORED;
      elbo_grad_loc[d] = sum u / R' = scale_d dELBO/dloc_d, elbo_grad_scale[d] = sum u z / R' + 1 = dELBO/dlog scale_d, with
        standard errors from the squared sums: both 0 at a stationary point whatever the posterior is;
      score_gap[d] = sqrt(sum (u + z)^2 / R'): 0 where q's score equals the posterior's along d;
      loc_shift[d] = sum w z / sum w (in units of q's sd), sd_ratio[d] = sqrt(sum w z^2 / sum w - loc_shift^2): the
        importance-corrected mean and sd of z; is_mean, is_sd: the same two of the centred coordinates (e0 + ...).
    Never raises on a check without a usable draw: everything is then None or NaN."""
    el = np.asarray(_lib.host64(elem), np.float64)
    t = np.asarray(_lib.host64(tot), np.float64).reshape(len(VI_TOT_COLUMNS))
    o = np.asarray(_lib.host64(out8), np.float64).reshape(8)
    D = int(np.asarray(loc).size)
    el = el.reshape(D, len(VI_ELEM_COLUMNS))
    e0 = np.asarray(_lib.host64(e0), np.float64).reshape(D)
    if int(np.asarray(scale).size) != D:
        raise ValueError("vi_check_summary: loc, scale and e0 of one length are required")
    n = float(t[0])
    num = lambda v: float(v) if np.isfinite(v) else None
    nanv = np.full(D, np.nan)
    if not n >= 1:
        return ViCheckSummary(0, None, None, None, None, 0, None, None, None, None, None, *([nanv] * 9))
    const = float(logp_const)
    with np.errstate(divide="ignore", invalid="ignore"):
        elbo = -t[3] / n + const
        elbo_se = np.sqrt(o[3] / n)
        ess = t[1] * t[1] / t[2]
        evidence = -t[4] + np.log(t[1]) - np.log(n) + const
        evidence_se = np.sqrt(max(1.0 / ess - 1.0 / n, 0.0)) if np.isfinite(ess) and ess > 0 else np.nan
        se_of_mean = lambda s1, s2: np.sqrt(np.maximum(s2 - s1 * s1 / n, 0.0) / (n - 1.0) / n) if n > 1 else nanv
        g_loc, g_loc_se = el[:, 0] / n, se_of_mean(el[:, 0], el[:, 1])
        g_scale, g_scale_se = el[:, 2] / n + 1.0, se_of_mean(el[:, 2], el[:, 3])
        gap = np.sqrt(el[:, 4] / n)
        shift = el[:, 5] / t[1]
        ratio = np.sqrt(np.maximum(el[:, 6] / t[1] - shift * shift, 0.0))
        cm = el[:, 7] / t[1]
        is_sd = np.sqrt(np.maximum(el[:, 8] / t[1] - cm * cm, 0.0))
    return ViCheckSummary(int(round(n)), num(elbo), num(elbo_se), num(o[1]), num(pareto_k_threshold(n)), int(round(o[4])),
                          num(ess), num(evidence), num(evidence_se), num(evidence - elbo),
                          num(np.sqrt(evidence_se * evidence_se + elbo_se * elbo_se)), g_loc, g_loc_se, g_scale, g_scale_se,
                          gap, shift, ratio, e0 + cm, is_sd)


# ---- power-scaling sensitivity: how much of a marginal is the prior's, how much the data's (csrc/psens.hip) ----
PSENS_DELTA = 0.01                # alpha = 1 + delta and 1 / (1 + delta) (Kallioinen et al. 2023; priorsense, ArviZ psens)
PSENS_THRESHOLD = 0.05            # a sensitivity above it is reported (the same sources)
CJS_COLUMNS = ("kept", "sum_w", "sum_wu", "sum_wu_sq", "a_pq", "a_qp", "i_p", "i_q")
CJS_MAX_ROWS = 8                  # the most weight rows arp_cjs_sums takes
# the weight rows of the report, in the order powerscale_lw writes and psens_summary reads them: the last is the
# unweighted one (lw = 0), which gives the pooled mean and sd the shifts are measured in
PSENS_ROWS = ("prior_lower", "prior_upper", "likelihood_lower", "likelihood_upper", "unweighted")
# The report (psens_summary), [D] float64, NaN for a constant element: prior, likelihood: the sensitivities;
# mean_shift_*: (weighted mean - pooled mean) / pooled sd of the upper row; sd_ratio_*: weighted sd / pooled sd of the
# upper row.  constant: the number of constant elements; conflict, weak_likelihood: the indices of the diagnosed elements.
PsensSummary = collections.namedtuple("PsensSummary", ["prior", "likelihood", "mean_shift_prior", "mean_shift_likelihood",
                                                       "sd_ratio_prior", "sd_ratio_likelihood", "constant", "conflict",
                                                       "weak_likelihood"])


def loglik_total(ll, total):
    """`arp_loglik_total`: adds every draw's column of ll [n, R] float32 on the GPU (rows may be further apart than R) to
    total [R] float64, in place, observations ascending -- tiles walked in ascending order compose bit for bit.  Returns
    total."""
    ll, n, R, stride = _ll_matrix(ll, None, "loglik_total")
    _lib.device_operand(total, torch.float64, (R,), "loglik_total", "total", "R")
    if total is None:
        raise ValueError("loglik_total: total is required")
    _lib.call(ll.device, _lib.lib().arp_loglik_total, _lib.ptr(ll), n, R, stride, _lib.ptr(total))
    return total


def element_order(trace, want_sorted=True):
    """(order, sorted) of `arp_element_order` for a recorded [S, C, D] float32 trace on the GPU: order [D, S C] int32 (the
    words are unsigned), order[d, i] the draw index r = s C + c of the i-th smallest value of element d, ties in
    ascending r; sorted [D, S C] float32, those values (None without want_sorted).  A leading or inner block of chains of
    a wider trace is taken in place, as rank_normalize takes it; the workspace is owned here."""
    x, S, Cn, D, row_stride = _lib.trace_view(trace, "element_order")
    if S == 0 or Cn == 0 or D == 0:
        raise ValueError("element_order: an empty trace")
    L = _lib.lib()
    need = int(L.arp_element_order_workspace_bytes(S, Cn, D))
    if need <= 0:
        _lib.check(1)
    order = torch.empty(D, S * Cn, dtype=torch.int32, device=x.device)
    values = torch.empty(D, S * Cn, dtype=torch.float32, device=x.device) if want_sorted else None
    _lib.call(x.device, L.arp_element_order, _lib.ptr(x), S, Cn, D, row_stride, _lib.ptr(order), _lib.ptr(values),
              workspace=need)
    return order, values


def cjs_sums(values, order, lw, shift=None):
    """out [K, D, 8] float64 device tensor of `arp_cjs_sums` (CJS_COLUMNS): values, order [D, N] as element_order returns
    them, lw [K, >= N] float64 on the GPU with unit column stride (1 <= K <= 8 rows of log weights, psis_weights'; -inf
    leaves a draw out of its row), shift: an optional [D] float32 device tensor the weighted moments are taken about."""
    if not (torch.is_tensor(values) and values.is_cuda and values.dtype == torch.float32 and values.dim() == 2
            and values.is_contiguous()):
        raise ValueError("cjs_sums: sorted values must be a contiguous float32 [D, N] matrix on the GPU (there is no CPU fallback)")
    D, N = (int(v) for v in values.shape)
    if D == 0 or N == 0:
        raise ValueError("cjs_sums: an empty matrix")
    _lib.device_operand(order, torch.int32, (D, N), "cjs_sums", "order", "D, N")
    _lib.device_operand(shift, torch.float32, (D,), "cjs_sums", "shift", "D")
    if order is None or not (torch.is_tensor(lw) and lw.dim() == 2 and 1 <= int(lw.shape[0]) <= CJS_MAX_ROWS):
        raise ValueError("cjs_sums: order and 1 ... 8 rows of lw are required")
    K = int(lw.shape[0])
    lw, lw_stride = _draw_matrix(lw, torch.float64, K, N, "cjs_sums", "lw")
    out = torch.empty(K, D, len(CJS_COLUMNS), dtype=torch.float64, device=values.device)
    _lib.call(values.device, _lib.lib().arp_cjs_sums, _lib.ptr(values), _lib.ptr(order), N, D, _lib.ptr(lw), lw_stride, K,
              _lib.ptr(shift), _lib.ptr(out))
    return out


# A latent site table (models.SiteTable) in device memory: D and P (the number of parts) as ints; the columns as contiguous
# device tensors (form, part [D] int32; loc_idx, scale_idx [D, 2] int32; loc_w, scale_w [D, 2] and loc0, log_scale0, norm [D]
# float32); host: a models.SiteTable of the same columns as numpy arrays, the float ones ROUNDED to float32 -- what the
# kernel reads, for a float64 evaluation of the very same table.
DeviceSiteTable = collections.namedtuple("DeviceSiteTable", ["D", "P", "form", "loc_idx", "loc_w", "loc0", "scale_idx", "scale_w",
                                                             "log_scale0", "norm", "part", "host"])
SITE_TERMS = 2                    # terms of a site's loc and of its log-scale (include/autoreparam.h: ARP_SITE_TERMS)


def upload_site_table(table, D, device):
    """models.SiteTable -> DeviceSiteTable on `device`, checked against a state of D elements as upload_table checks an
    observation table: one row per element, every index in [0, D), every form in {0, 1, 2}, part >= 0 -- and the ancestral
    order: a term of non-zero weight points at an element before its own.  The float columns are rounded to float32."""
    D = int(D)
    form, part = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (table.form, table.part))
    loc_idx, scale_idx = (np.ascontiguousarray(v, np.int32) for v in (table.loc_idx, table.scale_idx))
    loc_w, scale_w = (np.ascontiguousarray(v, np.float32) for v in (table.loc_w, table.scale_w))
    loc0, log_scale0, norm = (np.ascontiguousarray(v, np.float32).reshape(-1) for v in (table.loc0, table.log_scale0, table.norm))
    if D < 1 or not all(v.size == D for v in (form, part, loc0, log_scale0, norm)):
        raise ValueError("site table: form, loc0, log_scale0, norm and part must have one entry per element (%d)" % D)
    if not all(v.shape == (D, SITE_TERMS) for v in (loc_idx, loc_w, scale_idx, scale_w)):
        raise ValueError("site table: loc_idx, loc_w, scale_idx and scale_w of shape [%d, %d] are required" % (D, SITE_TERMS))
    if min(loc_idx.min(), scale_idx.min()) < 0 or max(loc_idx.max(), scale_idx.max()) >= D:
        raise ValueError("site table: an index lies outside the state's %d elements" % D)
    if not np.isin(form, (0, 1, 2)).all():
        raise ValueError("site table: form must be 0 (Normal), 1 (Normal, softplus scale) or 2 (log-Gamma)")
    if part.min() < 0:
        raise ValueError("site table: part must not be negative")
    d = np.arange(D)[:, None]
    if not all(np.all((w == 0) | (i < d)) for i, w in ((loc_idx, loc_w), (scale_idx, scale_w))):
        raise ValueError("site table: a term of non-zero weight must point at an earlier element (the ancestral order)")
    dev = lambda a: torch.as_tensor(a, device=device)
    host = type(table)(form, loc_idx, loc_w, loc0, scale_idx, scale_w, log_scale0, norm, part)
    return DeviceSiteTable(D, int(part.max()) + 1, dev(form), dev(loc_idx), dev(loc_w), dev(loc0), dev(scale_idx), dev(scale_w),
                           dev(log_scale0), dev(norm), dev(part), host)


def site_logprior(trace, table, group_of=None, want_elements=False):
    """(group_lp, elem_lp, mask, n_masked) of `arp_site_logprior` for a recorded CENTRED [S, C, D] float32 trace on the GPU
    and a DeviceSiteTable: group_lp [S C, G] float64, the log prior density of every group of elements at draw s C + c
    (the float32 element values added in float64, in a fixed order); elem_lp [S C, D] float32, the elements' own values
    (None without want_elements); mask [S C] uint8 and n_masked as pointwise_loglik's -- a masked draw's rows are 0.
    group_of: the group of every element, anything numpy reads as [D] integers (validated into [0, G), G = its largest
    entry + 1 <= D; need not be contiguous; a group without elements is 0); None: the table's parts.  A leading or inner
    block of chains of a wider trace is read in place, as pointwise_loglik reads it."""
    who = "site_logprior"
    x, S, Cn, D, row_stride = _lib.trace_view(trace, who)
    R = S * Cn
    if R == 0 or D == 0:
        raise ValueError("%s: an empty trace" % who)
    if D != table.D:
        raise ValueError("%s: the trace has %d elements, the table %d" % (who, D, table.D))
    dev = x.device
    if group_of is None:
        groups, G = table.part, table.P
    else:
        g = np.asarray(group_of)
        if g.shape != (D,) or g.dtype.kind not in "iu" or g.min() < 0 or g.max() >= D:
            raise ValueError("%s: group_of must be [%d] integers in [0, G), G <= D" % (who, D))
        groups, G = torch.as_tensor(np.ascontiguousarray(g, np.int32), device=dev), int(g.max()) + 1
    group_lp = torch.empty(R, G, dtype=torch.float64, device=dev)
    elem_lp = torch.empty(R, D, dtype=torch.float32, device=dev) if want_elements else None
    mask, n_masked = _mask_pair(R, dev)
    _lib.call(dev, _lib.lib().arp_site_logprior, _lib.ptr(x), S, Cn, D, row_stride, _lib.ptr(table.form), _lib.ptr(table.loc_idx),
              _lib.ptr(table.loc_w), _lib.ptr(table.loc0), _lib.ptr(table.scale_idx), _lib.ptr(table.scale_w),
              _lib.ptr(table.log_scale0), _lib.ptr(table.norm), _lib.ptr(groups), G, _lib.ptr(group_lp), _lib.ptr(elem_lp),
              _lib.ptr(mask), _lib.ptr(n_masked))
    return group_lp, elem_lp, mask, n_masked


SITE_MAX_DRAWS = 1 << 24          # the most draws arp_site_prior_draws takes


def site_prior_draws(table, draws, seed=0, draw_offset=0, device=None, out=None):
    """(x, undrawn) of `arp_site_prior_draws`: `draws` ancestral draws from the prior a DeviceSiteTable describes, x
    [draws, D] float32 -- as x[None] a centred trace of one step and `draws` chains, which predictive_check, site_logprior
    and element_order take in place -- and undrawn [draws] uint8, non-zero for a draw one of whose log-Gamma elements ran
    out of attempts (its element is NaN; 32 rejections in a row: not expected to be seen).  Draw r is a function of (seed,
    draw_offset + r) alone.  device: the table's when None; a table on another device is refused.  out: an optional
    float32 [draws, >= D] device matrix with unit column stride, written in place in its first D columns (the others are
    not touched).  Refused here, before any call: what the kernel refuses."""
    who = "site_prior_draws"
    if not isinstance(table, DeviceSiteTable):
        raise ValueError("%s: a DeviceSiteTable is required (upload_site_table)" % who)
    D, R = int(table.D), int(draws)
    if not 1 <= D <= LOGLIK_MAX_D:
        raise ValueError("%s: 1 <= D <= %d elements are required" % (who, LOGLIK_MAX_D))
    if not 1 <= R <= SITE_MAX_DRAWS:
        raise ValueError("%s: 1 <= draws <= 2^24 is required" % who)
    if int(draw_offset) < 0:
        raise ValueError("%s: draw_offset >= 0 is required" % who)
    dev = table.form.device
    if dev.type != "cuda":
        raise ValueError("%s: the table must be on the GPU (there is no CPU fallback)" % who)
    if device is not None and torch.device(device) != dev and torch.device(device) != torch.device(dev.type):
        raise ValueError("%s: the table is on %s, not on %s" % (who, dev, device))
    if out is None:
        x, stride = torch.empty(R, D, dtype=torch.float32, device=dev), D
    else:
        x, stride = _rows_out(out, R, D, who, "out")
        if x.device != dev:
            raise ValueError("%s: out must be on the table's device" % who)
    undrawn = torch.empty(R, dtype=torch.uint8, device=dev)
    _lib.call(dev, _lib.lib().arp_site_prior_draws, D, _lib.ptr(table.form), _lib.ptr(table.loc_idx), _lib.ptr(table.loc_w),
              _lib.ptr(table.loc0), _lib.ptr(table.scale_idx), _lib.ptr(table.scale_w), _lib.ptr(table.log_scale0), R,
              int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw_offset), _lib.ptr(x), stride, _lib.ptr(undrawn))
    return x, undrawn


def site_redraw(trace, table, redraw, seed=0, draw_offset=0, out=None):
    """(x, undrawn) of `arp_site_redraw` for a recorded CENTRED [S, C, D] float32 trace on the GPU, a DeviceSiteTable and
    `redraw`, [D] flags (anything numpy reads, or a uint8 device tensor): x [S C, D] float32, row s C + c the recorded draw
    (s, c) with every flagged element drawn anew from its conditional prior given the rest of the row -- exactly as
    site_prior_draws draws it, its parents read from the row being built -- and every other element as recorded, bit for
    bit; as x[None] a centred trace of one step and S C chains, which predictive_check takes in place.  undrawn [S C] uint8
    as site_prior_draws'.  Row r is a function of (seed, draw_offset + r), the flags and its own recorded row alone:
    `draw_offset` is the global number of this trace's first draw.  A block of chains of a wider trace is read in place,
    as pointwise_loglik reads it.  out: as site_prior_draws'.  WHICH elements may be flagged is `redraw_selection`'s rule,
    not checked here.  Refused here, before any call: what the kernel refuses."""
    who = "site_redraw"
    if not isinstance(table, DeviceSiteTable):
        raise ValueError("%s: a DeviceSiteTable is required (upload_site_table)" % who)
    D = int(table.D)
    if not 1 <= D <= LOGLIK_MAX_D:
        raise ValueError("%s: 1 <= D <= %d elements are required" % (who, LOGLIK_MAX_D))
    if int(draw_offset) < 0:
        raise ValueError("%s: draw_offset >= 0 is required" % who)
    flags = redraw if torch.is_tensor(redraw) else np.asarray(redraw)
    if tuple(flags.shape) != (D,) or (torch.is_tensor(flags) and flags.dtype != torch.uint8) or \
            (not torch.is_tensor(flags) and flags.dtype.kind not in "biu"):
        raise ValueError("%s: redraw must be [%d] flags (bool or integers; a tensor: uint8)" % (who, D))
    x, S, Cn, Dx, row_stride = _lib.trace_view(trace, who)
    R = S * Cn
    if R == 0 or Dx == 0:
        raise ValueError("%s: an empty trace" % who)
    if Dx != D:
        raise ValueError("%s: the trace has %d elements, the table %d" % (who, Dx, D))
    if R > SITE_MAX_DRAWS:
        raise ValueError("%s: at most 2^24 draws (S C) are taken" % who)
    dev = x.device
    if table.form.device != dev:
        raise ValueError("%s: the table must be on the trace's device" % who)
    if torch.is_tensor(flags):
        flags = flags.to(dev).contiguous()
    else:
        flags = torch.as_tensor(np.ascontiguousarray(flags != 0, np.uint8), device=dev)
    if out is None:
        rows, stride = torch.empty(R, D, dtype=torch.float32, device=dev), D
    else:
        rows, stride = _rows_out(out, R, D, who, "out")
        if rows.device != dev:
            raise ValueError("%s: out must be on the trace's device" % who)
        if rows.data_ptr() == x.data_ptr():
            raise ValueError("%s: out must not be the trace (the rows are rebuilt from the recorded ones)" % who)
    undrawn = torch.empty(R, dtype=torch.uint8, device=dev)
    _lib.call(dev, _lib.lib().arp_site_redraw, _lib.ptr(x), S, Cn, D, row_stride, _lib.ptr(table.form), _lib.ptr(table.loc_idx),
              _lib.ptr(table.loc_w), _lib.ptr(table.loc0), _lib.ptr(table.scale_idx), _lib.ptr(table.scale_w),
              _lib.ptr(table.log_scale0), _lib.ptr(flags), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw_offset), _lib.ptr(rows), stride,
              _lib.ptr(undrawn))
    return rows, undrawn


REDRAW_FLAG = "--predictive_checks_redraw"


def redraw_selection(site_table, part_names, names):
    """The [D] uint8 flags site_redraw takes for the latent parts `names` of a model: 1 for every element of a named part.
    The ONE place where the rule of a mixed predictive check's selection is defined; pure numpy.  site_table: a
    models.SiteTable (or the host copy of an uploaded one); part_names: the model's, which site_table.part indexes.
    Raises ValueError, naming the flag and the model's parts, for an empty name, a duplicate, a name that is no part --
    and for a selection that is not closed under descent: if an element that stays as recorded has a term of non-zero
    weight (in its loc or its log-scale; the log-Gamma form does not read its loc terms) at a flagged element, it was drawn
    GIVEN the recorded value of what is now redrawn, and the row is a draw from no distribution the model defines
    (mua redrawn, the m drawn from it kept).  The message names the parts that would have to be added (the closure)."""
    parts = [str(p) for p in part_names]
    names = [str(n) for n in names]
    tail = "; the model's parts: %s" % ", ".join(parts)
    if not names or "" in names:
        raise ValueError("%s: an empty name in %r%s" % (REDRAW_FLAG, ",".join(names), tail))
    if len(set(names)) != len(names):
        raise ValueError("%s: %s is named twice%s" % (REDRAW_FLAG, ", ".join(sorted({n for n in names if names.count(n) > 1})), tail))
    unknown = [n for n in names if n not in parts]
    if unknown:
        raise ValueError("%s: %s is no latent part of the model%s" % (REDRAW_FLAG, ", ".join(unknown), tail))
    part = np.asarray(site_table.part, np.int64).reshape(-1)
    form = np.asarray(site_table.form, np.int64).reshape(-1)
    D = part.size
    chosen = np.zeros(len(parts), bool)
    chosen[[parts.index(n) for n in names]] = True
    closed = chosen.copy()
    columns = ((np.asarray(site_table.loc_idx), np.asarray(site_table.loc_w), form != 2),
               (np.asarray(site_table.scale_idx), np.asarray(site_table.scale_w), np.ones(D, bool)))
    while True:                                  # the parts of every element that descends from a flagged one
        flagged = closed[part]
        hangs = np.zeros(D, bool)
        for idx, w, read in columns:
            at = np.clip(np.asarray(idx, np.int64), 0, D - 1)
            hangs |= read & np.any((np.asarray(w) != 0) & flagged[at], axis=1)
        more = np.zeros(len(parts), bool)
        more[part[hangs & ~flagged]] = True
        if not more.any():
            break
        closed |= more
    missing = [p for k, p in enumerate(parts) if closed[k] and not chosen[k]]
    if missing:
        raise ValueError("%s: %s would stay as recorded although drawn from what is redrawn (%s) -- such a row is a draw from "
                         "no distribution the model defines; add %s%s" % (
                             REDRAW_FLAG, ", ".join(missing), ", ".join(n for n in parts if n in names), ",".join(missing), tail))
    return chosen[part].astype(np.uint8)


# ---- prior predictive checks: what the prior says before it has seen data, and how far the data moved it ----
PRIOR_QUANTILES = (0.05, 0.5, 0.95)
PRIOR_Z90 = 1.6448536269514722    # the standard normal's 95 % point: (q95 - q05) / (2 z) is the sd of a normal
# prior_predictive_summary.  draws_used, draws_left_out: ints.  quantiles: a dict over PPC_STATISTICS[:4] of the (5 %, 50 %,
# 95 %) order statistics of the replicated statistic over the draws used, or None where it is not defined (no draw used; sd,
# min and max of Bernoulli data).
PriorPredictiveSummary = collections.namedtuple("PriorPredictiveSummary", ["draws_used", "draws_left_out", "quantiles"])
# prior_contraction_summary.  prior_sd_robust, contraction, z_score: [D] float64, NaN for an element left out;
# left_out: how many there are.
PriorContractionSummary = collections.namedtuple("PriorContractionSummary", ["prior_sd_robust", "contraction", "z_score",
                                                                           "left_out"])


def order_statistic_index(p, n):
    """The 0-based index of the order statistic x_(ceil(p n)) among n sorted values (the inverse of the empirical
    distribution function), clamped into [0, n)."""
    return int(min(max(math.ceil(float(p) * int(n)) - 1, 0), int(n) - 1))


def prior_predictive_summary(draw_stats, y, kind, mask=None):
    """What data the prior alone generates, on the scale of y -> PriorPredictiveSummary; pure numpy float64.  draw_stats
    [R, 8] over ALL N observations (PPC_DRAW_COLUMNS) of replicated data sets drawn at PRIOR draws, y [N], kind 0 (Normal)
    or 1 (Bernoulli-logit), mask [R] (non-zero: the draw is left out).  Per statistic of mean, sd, min, max of a replicated
    data set (ppc_counts' definitions, one helper) the order statistics x_(ceil(p R')) at p = 5 %, 50 %, 95 % over the R'
    draws used; a NaN (a replicated data set with an infinite value has no sd) sorts last, as +inf would.  sd, min and max
    are None for Bernoulli data and sd for a single observation, as in ppc_from_counts.  The p-values next to these are
    ppc_summary's, on the same draw_stats: nothing is defined twice."""
    c = _lib.host64(draw_stats).reshape(-1, len(PPC_DRAW_COLUMNS))
    y = np.asarray(_lib.host64(y), np.float64).reshape(-1)
    N = y.size
    if N < 1:
        raise ValueError("prior_predictive_summary: at least one observation is required")
    used = np.ones(c.shape[0], bool) if mask is None else (_lib.host64(mask).reshape(-1) == 0)
    if used.size != c.shape[0]:
        raise ValueError("prior_predictive_summary: mask must have one entry per draw")
    c = c[used]
    n = int(c.shape[0])
    normal = int(kind) == 0
    defined = {"mean": True, "sd": normal and N > 1, "min": normal, "max": normal}
    at = [order_statistic_index(p, n) for p in PRIOR_QUANTILES] if n else []
    quantiles = {}
    for name, rep in zip(PPC_STATISTICS[:4], _ppc_replicated(c, N)):
        s = np.sort(rep)
        quantiles[name] = tuple(float(s[i]) for i in at) if defined[name] and n else None
    return PriorPredictiveSummary(n, int(used.size) - n, quantiles)


def prior_contraction_summary(q05, q50, q95, post_mean, post_sd):
    """How far every marginal has contracted from prior to posterior (Betancourt's posterior contraction and z-score;
    Schad, Betancourt, Vasishth 2021) -> PriorContractionSummary; pure numpy float64, [D] each: the prior's 5 %, 50 % and
    95 % points and the posterior's mean and sd.
      prior_sd_robust = (q95 - q05) / (2 * 1.6448536269514722),  the sd of the normal with that 90 % interval
      contraction     = 1 - (post_sd / prior_sd_robust)^2        near 1: the data decided; near 0: the prior did; below 0:
                                                                 the posterior is WIDER than the prior's central part
      z_score         = (post_mean - q50) / prior_sd_robust      where the posterior sits in the prior, in prior sds
    The prior's scale is quantile-based ON PURPOSE: under log_sigma ~ N(0, 10) the marginal prior variance of a group effect
    is of the order e^200 and its sample variance means nothing, while the central 90 % interval is well defined and
    well estimated.  The posterior's scale is a moment (the sd split R-hat already pooled): the two are the same thing for a
    normal marginal only, so a heavy-tailed prior marginal reads as more contracted than a moment scale would say.  An
    element whose prior interval is empty (a constant element) or not finite is NaN in all three and counted."""
    q05, q50, q95, m, sd = (np.asarray(_lib.host64(v), np.float64).reshape(-1) for v in (q05, q50, q95, post_mean, post_sd))
    if not all(v.size == q05.size for v in (q50, q95, m, sd)):
        raise ValueError("prior_contraction_summary: five vectors of one length are required")
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        scale = (q95 - q05) / (2.0 * PRIOR_Z90)
        ok = np.isfinite(scale) & (scale > 0) & np.isfinite(q50)
        scale = np.where(ok, scale, np.nan)
        contraction = 1.0 - (sd / scale) ** 2
        z = (m - q50) / scale
    return PriorContractionSummary(scale, contraction, z, int(np.sum(~ok)))


def powerscale_lw(log_prior, log_likelihood, left_out=None):
    """(out, lw) for the power-scaled prior and likelihood of R draws: log_prior, log_likelihood [R] float64 device tensors
    (additive constants cancel), left_out an optional [R] bool or uint8 device tensor.  The four rows PSENS_ROWS[:4] are
    the log ratios (alpha - 1) * component at alpha = 1 / (1 + PSENS_DELTA) and 1 + PSENS_DELTA; psis_weights takes the
    NEGATED log ratio as float32 (about its mean over the draws kept, which cancels too, so that float32 resolves the
    ratios and not the component's size).  out [4, 8] float64: PSIS_COLUMNS per row, out[:, 1] the k-hat; lw [5, R] float64:
    the smoothed log weights of the four rows and PSENS_ROWS[4], 0 for a draw kept; -inf throughout for a draw left out."""
    if not (torch.is_tensor(log_prior) and log_prior.is_cuda and log_prior.dim() == 1 and log_prior.numel() > 0
            and torch.is_tensor(log_likelihood) and log_likelihood.shape == log_prior.shape):
        raise ValueError("powerscale_lw: log_prior and log_likelihood of one shape [R] on the GPU are required")
    R = int(log_prior.numel())
    dev = log_prior.device
    mask = torch.zeros(R, dtype=torch.uint8, device=dev) if left_out is None else left_out.to(torch.uint8).contiguous()
    kept = mask == 0
    rows = []
    for component in (log_prior, log_likelihood):
        c = component.to(torch.float64)
        centre = torch.where(kept, c, torch.zeros_like(c)).sum() / kept.sum().clamp(min=1)
        c = torch.where(kept, c - centre, torch.zeros_like(c))
        for alpha in (1.0 / (1.0 + PSENS_DELTA), 1.0 + PSENS_DELTA):
            rows.append((-(alpha - 1.0) * c).to(torch.float32))
    out, lw4 = psis_weights(torch.stack(rows).contiguous(), mask)
    base = torch.where(kept, torch.zeros(R, dtype=torch.float64, device=dev),
                       torch.full((R,), float("-inf"), dtype=torch.float64, device=dev))
    return out, torch.cat([lw4, base[None]], dim=0).contiguous()


def _cjs_distance(s):
    """The cumulative Jensen-Shannon distance of one weight row from its [D, 8] sums; NaN for a constant element."""
    a_pq, a_qp, i_p, i_q = s[:, 4], s[:, 5], s[:, 6], s[:, 7]
    ln4 = 2.0 * np.log(2.0)
    cjs_pq = np.maximum(0.0, a_pq + (i_q - i_p) / ln4)
    cjs_qp = np.maximum(0.0, a_qp + (i_p - i_q) / ln4)
    return np.sqrt((cjs_pq + cjs_qp) / (i_p + i_q))


def psens_summary(sums):
    """Power-scaling sensitivity, the single place where its statistics are defined -> PsensSummary; pure numpy float64.
    sums [5, D, 8]: cjs_sums of the rows PSENS_ROWS.  Per row
      cjs_pq = max(0, A_pq + (I_q - I_p) / (2 ln 2)),  cjs_qp = max(0, A_qp + (I_p - I_q) / (2 ln 2)),
      dist = sqrt((cjs_pq + cjs_qp) / (I_p + I_q))                  (NaN for a constant element: 0 / 0)
    and sensitivity = (dist_lower + dist_upper) / (2 log2(1 + PSENS_DELTA)), for the prior and for the likelihood.  With
    the pooled mean and sd from the unweighted row, mean = sum W u / sum W, sd = sqrt(sum W u^2 / sum W - mean^2):
    mean_shift = (mean_upper - mean_pooled) / sd_pooled, sd_ratio = sd_upper / sd_pooled.  Diagnosis against
    PSENS_THRESHOLD: prior above and likelihood above -- prior-data conflict; prior above only -- weak likelihood (or a
    strong prior); a NaN is above nothing."""
    s = np.asarray(_lib.host64(sums), np.float64)
    if s.ndim != 3 or s.shape[0] != len(PSENS_ROWS) or s.shape[2] != len(CJS_COLUMNS):
        raise ValueError("psens_summary: sums must be [5, D, 8] (PSENS_ROWS, CJS_COLUMNS)")
    with np.errstate(divide="ignore", invalid="ignore"):
        dist = [_cjs_distance(s[k]) for k in range(4)]
        scale = 2.0 * np.log2(1.0 + PSENS_DELTA)
        prior, likelihood = (dist[0] + dist[1]) / scale, (dist[2] + dist[3]) / scale
        mean = s[:, :, 2] / s[:, :, 1]
        sd = np.sqrt(np.maximum(s[:, :, 3] / s[:, :, 1] - mean * mean, 0.0))
        shift = [np.where(sd[4] > 0, (mean[k] - mean[4]) / sd[4], np.nan) for k in (1, 3)]
        ratio = [np.where(sd[4] > 0, sd[k] / sd[4], np.nan) for k in (1, 3)]
        above_p, above_l = prior > PSENS_THRESHOLD, likelihood > PSENS_THRESHOLD
    return PsensSummary(prior, likelihood, shift[0], shift[1], ratio[0], ratio[1],
                        int(np.sum(np.isnan(prior) | np.isnan(likelihood))),
                        np.flatnonzero(above_p & above_l), np.flatnonzero(above_p & ~above_l))


# ---- simulation-based calibration: where the truths sit among the refits' draws (csrc/sbc.hip) ----
SBC_MAX_Q = 256                   # the most quantities arp_sbc_fold takes (csrc/sbc.hip: kSbcMaxQ)
SBC_MAX_DRAWS = 1 << 24           # the most draws per replicate
SBC_MAX_REPLICATES = 1 << 20      # the most replicates
# sbc_summary.  replications: N', the replicates not left out; left_out: how many were; draws: L; names: the quantities.
# Per replicate and quantity, [N, Q] float64 with NaN rows for a replicate left out: u (the rank value), post_bias
# (posterior mean - truth), post_sd, post_z.  Per quantity, [Q] float64 (NaN where N' is too small): ks, ks_p, rank_mean_z,
# rank_var_ratio, rank_var_z, post_z_mean, post_z_sd; constant [Q] bool: every draw of every kept replicate equals its truth.
SbcSummary = collections.namedtuple("SbcSummary", ["replications", "left_out", "draws", "names", "u", "post_bias", "post_sd",
                                                   "post_z", "ks", "ks_p", "rank_mean_z", "rank_var_ratio", "rank_var_z",
                                                   "post_z_mean", "post_z_sd", "constant"])


def sbc_fold(draws, truth):
    """(counts, sums, left_out, n_left_out) of `arp_sbc_fold` for draws [N, L, Q] and truth [N, Q], float32 device
    tensors: counts [N, Q, 2] int32 = (#{x < t}, #{x == t}) and sums [N, Q, 2] float64 = (sum (x - t), sum (x - t)^2) over
    the L draws x of replicate r's quantity q against its truth t; left_out [N] uint8, 1 for a replicate whose truth or
    any of whose draws is not finite (its counts and sums are 0); n_left_out: their count, an int64 device scalar.  An
    inner block of a wider buffer -- draws[:, :l, :q] of [N, L', Q'], truth[:, :q] -- is read in place, through its
    strides; any other layout is copied.  Refused here, before any call: what the kernel refuses."""
    who = "sbc_fold"
    if not (torch.is_tensor(draws) and torch.is_tensor(truth) and draws.is_cuda and truth.is_cuda
            and draws.dtype == torch.float32 and truth.dtype == torch.float32 and draws.dim() == 3 and truth.dim() == 2):
        raise ValueError("%s: float32 draws [N, L, Q] and truth [N, Q] on the GPU are required (there is no CPU fallback)" % who)
    N, L, Q = (int(v) for v in draws.shape)
    if tuple(truth.shape) != (N, Q) or truth.device != draws.device:
        raise ValueError("%s: truth must be [%d, %d] on the draws' device" % (who, N, Q))
    if not 1 <= Q <= SBC_MAX_Q:
        raise ValueError("%s: 1 <= Q <= %d quantities are required" % (who, SBC_MAX_Q))
    if not 1 <= L <= SBC_MAX_DRAWS:
        raise ValueError("%s: 1 <= L <= 2^24 draws per replicate are required" % who)
    if not 1 <= N <= SBC_MAX_REPLICATES:
        raise ValueError("%s: 1 <= N <= 2^20 replicates are required" % who)
    # (the stride of an axis of length 1 means nothing)
    row = int(draws.stride(1)) if L > 1 else Q
    rep = int(draws.stride(0)) if N > 1 else L * row
    if not ((draws.stride(2) == 1 or Q == 1) and row >= Q and rep >= L * row):
        draws = draws.contiguous()
        row, rep = Q, L * Q
    t_stride = int(truth.stride(0)) if N > 1 else Q
    if not ((truth.stride(1) == 1 or Q == 1) and t_stride >= Q):
        truth, t_stride = truth.contiguous(), Q
    dev = draws.device
    counts = torch.empty(N, Q, 2, dtype=torch.int32, device=dev)
    sums = torch.empty(N, Q, 2, dtype=torch.float64, device=dev)
    left_out = torch.empty(N, dtype=torch.uint8, device=dev)
    n_left_out = torch.zeros((), dtype=torch.int64, device=dev)
    _lib.call(dev, _lib.lib().arp_sbc_fold, _lib.ptr(draws), N, L, Q, rep, row, _lib.ptr(truth), t_stride, _lib.ptr(counts),
              _lib.ptr(sums), _lib.ptr(left_out), _lib.ptr(n_left_out))
    return counts, sums, left_out, n_left_out


def kolmogorov_p_value(ks, n):
    """The asymptotic p-value of a Kolmogorov distance `ks` of n values, in Stephens' (1970) form:
    lambda = (sqrt n + 0.12 + 0.11 / sqrt n) ks,  p = 2 sum_{j >= 1} (-1)^(j - 1) exp(-2 j^2 lambda^2), clipped to [0, 1];
    1 for lambda < 0.3 (the alternating series has not settled there, and the value is 1 to nine digits); NaN for n < 1."""
    if n < 1 or not np.isfinite(ks):
        return float("nan")
    root = math.sqrt(n)
    lam = (root + 0.12 + 0.11 / root) * float(ks)
    if lam < 0.3:
        return 1.0
    j = np.arange(1, 101, dtype=np.float64)
    p = 2.0 * float(np.sum((-1.0) ** (j - 1.0) * np.exp(-2.0 * j * j * lam * lam)))
    return min(max(p, 0.0), 1.0)


def sbc_summary(counts, sums, n_draws, left_out=None, names=None):
    """Simulation-based calibration, the single place where its statistics are defined -> SbcSummary; pure numpy
    float64.  counts, sums [N, Q, 2] as sbc_fold returns them, n_draws = L, left_out [N] (non-zero: the replicate enters
    nothing), names [Q].  Over the N' replicates kept, per quantity:
      u = (less + equal / 2 + 1 / 2) / (L + 1)          the mid-rank on (0, 1): deterministic, ties split evenly
      ks, ks_p                                          kolmogorov_distance of the u from uniform, kolmogorov_p_value
      rank_mean_z = (mean u - 1/2) sqrt(12 N')          its sign: on which side of the truth the posterior sits
      rank_var_ratio = 12 s^2,  rank_var_z = (s^2 - 1/12) sqrt(180 N')     s^2 the sample variance of u; Var(s^2) is about
                                                        (mu_4 - sigma^4) / N' = (1/80 - 1/144) / N' = 1 / (180 N').  A ratio
                                                        above 1 is a U-shaped histogram, a posterior too narrow; below 1
                                                        one too wide
      post_bias = s1 / L,  post_sd = sqrt((s2 - s1^2 / L) / (L - 1)) (NaN for L = 1),  post_z = post_bias / post_sd;
      post_z_mean, post_z_sd: mean and sd of the finite post_z over the replicates -- near 0 and 1
    A constant column (every draw equal to its truth) has u = 1/2 everywhere and is flagged in `constant`."""
    c = np.asarray(counts.cpu() if torch.is_tensor(counts) else counts).astype(np.float64)
    s = _lib.host64(sums)
    if c.ndim != 3 or c.shape[2] != 2 or s.shape != c.shape:
        raise ValueError("sbc_summary: counts and sums of one [N, Q, 2] shape are required")
    N, Q = c.shape[:2]
    L = int(n_draws)
    if L < 1:
        raise ValueError("sbc_summary: n_draws >= 1 is required")
    kept = np.ones(N, bool) if left_out is None else (_lib.host64(left_out).reshape(-1) == 0)
    if kept.size != N:
        raise ValueError("sbc_summary: left_out must have one entry per replicate")
    names = list(names) if names is not None else ["q%d" % q for q in range(Q)]
    if len(names) != Q:
        raise ValueError("sbc_summary: names must have one entry per quantity")
    n = int(kept.sum())
    nan_q = np.full(Q, np.nan)
    u = np.full((N, Q), np.nan)
    u[kept] = (c[kept, :, 0] + 0.5 * c[kept, :, 1] + 0.5) / (L + 1.0)
    bias, sd, z = np.full((N, Q), np.nan), np.full((N, Q), np.nan), np.full((N, Q), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        bias[kept] = s[kept, :, 0] / L
        if L > 1:
            sd[kept] = np.sqrt(np.maximum(s[kept, :, 1] - s[kept, :, 0] ** 2 / L, 0.0) / (L - 1.0))
        z[kept] = bias[kept] / sd[kept]
    ks, ks_p, mean_z, var_ratio, var_z, z_mean, z_sd = (nan_q.copy() for _ in range(7))
    uk = u[kept]
    for q in range(Q):
        if n >= 1:
            ks[q] = kolmogorov_distance(uk[:, q])
            ks_p[q] = kolmogorov_p_value(ks[q], n)
            mean_z[q] = (uk[:, q].mean() - 0.5) * math.sqrt(12.0 * n)
        if n >= 2:
            s2 = float(np.var(uk[:, q], ddof=1))
            var_ratio[q] = 12.0 * s2
            var_z[q] = (s2 - 1.0 / 12.0) * math.sqrt(180.0 * n)
        zq = z[kept, q]
        zq = zq[np.isfinite(zq)]
        if zq.size >= 1:
            z_mean[q] = zq.mean()
        if zq.size >= 2:
            z_sd[q] = zq.std(ddof=1)
    constant = np.all(c[kept, :, 1] == L, axis=0) if n else np.zeros(Q, bool)
    return SbcSummary(n, N - n, L, names, u, bias, sd, z, ks, ks_p, mean_z, var_ratio, var_z, z_mean, z_sd, constant)
