"""What the reports of main.py and the stand-alone modes (sbc.py) share: formatting, the step and tile rules, the seed rule,
the null path and the walks over draws and tiles.  A leaf: it imports neither of them; diagnostics.<name> is looked up per call."""
import json
import os
from collections import OrderedDict

import numpy as np

from . import diagnostics, util

LOO_CHUNK_BYTES = 256 << 20          # a tile's [observations, draws] float32 log-likelihoods stay below this


def _finite_or_none(x):
    """A JSON number, or None (written as null) for NaN / inf: `nan` is not JSON and never equals itself."""
    x = float(x)
    return x if np.isfinite(x) else None


def _nan_max(x):
    """(largest finite entry, its index), or (nan, -1) when there is none."""
    x = np.asarray(x, np.float64)
    ok = np.flatnonzero(np.isfinite(x))
    if not ok.size:
        return float("nan"), -1
    at = int(ok[x[ok].argmax()])
    return float(x[at]), at


def _fmt(v):
    return "n/a" if v is None else "{:.4g}".format(v)


def _shown(items, limit):
    """The first `limit` of `items`, comma separated, then `, ...` when there are more: how a warning names what it found."""
    return ", ".join(str(v) for v in items[:limit]) + (", ..." if len(items) > limit else "")


def _above(k, threshold, present=None):
    """[len(k)] bool: Pareto k-hat above `threshold`; where the threshold is not finite (None: written as null), not
    fitted -- not finite -- among the rows that are `present` (all; an empty group's row is NaN and absent)."""
    k = np.asarray(k, np.float64)
    with np.errstate(invalid="ignore"):
        if threshold is not None and np.isfinite(threshold):
            return k > threshold
        return ~np.isfinite(k) if present is None else present & ~np.isfinite(k)


def grouped_head(part, names, group_of, sizes):
    """The arrays a grouped side file opens with: the part, its groups' names, every observation's group, the groups' sizes."""
    return [("part", np.asarray(part)), ("groups", np.asarray(names)), ("group_of", np.asarray(group_of, np.int32)),
            ("n_obs", np.asarray(sizes, np.int64))]


def data_tail(y, spec):
    """The pair a side file closes with: the observations themselves and the model's name."""
    return [("y", np.asarray(y, np.float32)), ("model", np.asarray(spec.name))]


def element_names(spec):
    """One name per element of the flat state, in trace order: `tau` for a scalar part, `m[17]`, `z[2,3]` otherwise."""
    names = []
    for name, shape in zip(spec.part_names, spec.part_shapes):
        if not len(shape):
            names.append(name)
        else:
            names.extend("%s[%s]" % (name, ",".join(str(int(i)) for i in idx)) for idx in np.ndindex(*shape))
    return names


def _write_json_atomic(file_path, obj):
    """A reader (another rank at the top of its next phase, a later run) sees the old file or the new one, never a
    half-written one: write next to it, then rename over it."""
    tmp = "%s.tmp.%d" % (file_path, os.getpid())
    with open(tmp, "w") as f:
        json.dump(obj, f)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, file_path)


def _null_keys(title, why, keys):
    """Every key of `keys` as null, with the one message that says why the report `title` was not computed."""
    util.print_("    {}: not computed, {}".format(title, why))
    return OrderedDict((key, None) for key in keys)


def derived_seed(seed, constant):
    """A report's own 64-bit seed, from --seed and the report's seed constant."""
    return (int(seed) * 0x9E3779B97F4A7C15 + constant) & 0xFFFFFFFFFFFFFFFF


def next_seed(seed):
    """The seed after `seed`: a second stream that does not repeat the first's Philox words."""
    return (seed + 1) & 0xFFFFFFFFFFFFFFFF


def probe_steps(S, R):
    """The recorded steps an energy probe visits: R evenly spaced of S, the first and the last among them; all S if S < R."""
    S, R = int(S), int(R)
    if S <= 0 or R <= 0:
        return []
    return sorted({int(round(v)) for v in np.linspace(0, S - 1, min(S, R))})


def loo_steps(S, k, draws):
    """The recorded steps the predictive report takes its draws from: clamp(draws // k, 1, S) evenly spaced of S, the last
    one among them (probe_steps, the rule of --energy_probe_steps, counted from the end: a single step is the last), and
    no more than arp_psis_loo takes draws of."""
    k, S = max(int(k), 1), int(S)
    want = max(1, min(S, int(draws) // k))
    return sorted(S - 1 - s for s in probe_steps(S, min(want, diagnostics.PSIS_MAX_DRAWS // k)))


def rows_within(count, bytes_per_row, budget=None, workspace_bytes=None, cap=None):
    """The one budget rule of the reports: clamp(budget // bytes_per_row, 1, count) rows (at most `cap`), then halved,
    (rows + 1) // 2, while `workspace_bytes(rows)` -- whatever more a call of that many rows takes -- is over `budget`
    bytes (LOO_CHUNK_BYTES); at least one."""
    budget = LOO_CHUNK_BYTES if budget is None else int(budget)
    rows = max(1, min(max(int(count), 1), budget // max(1, int(bytes_per_row))))
    rows = int(rows if cap is None else min(rows, cap))
    while workspace_bytes is not None and rows > 1 and workspace_bytes(rows) > budget:
        rows = (rows + 1) // 2
    return rows


def loo_tile_rows(N, R, budget=None):
    """Observations per tile of the predictive report: rows of R float32 within `budget` bytes (LOO_CHUNK_BYTES); at
    least one."""
    return rows_within(N, 4 * int(R), budget)


def ppc_tile_rows(N, R, workspace_bytes, budget=None):
    """Observations per tile of the predictive checks: loo_tile_rows, halved until `workspace_bytes(rows, R)` -- the
    kernel's partial sums, the only [observations, draws]-sized memory this report takes -- is within the budget too; at
    least one."""
    return rows_within(N, 4 * int(R), budget, lambda rows: workspace_bytes(rows, R))


def select_draws(trace, k, k_steps, flags):
    """(why, steps, draws) of the LOO, PPC and sensitivity reports: the leading `k` chains of the device trace [S, C, D] at
    loo_steps(S, k_steps, --loo_draws), k_steps being k or the job-wide count of a sharded PPC.  `why`: None, or why there is
    no report.  `draws` [len(steps), k, D]: a copy, D floats a draw; None for k = 0, the idle rank of a sharded PPC."""
    import torch
    S, _, D = (int(v) for v in trace.shape)
    if S <= 0 or int(k_steps) <= 0:
        return "no chain has its trace on the device", None, None
    if D > diagnostics.LOGLIK_MAX_D:
        return "the model has more than {} elements".format(diagnostics.LOGLIK_MAX_D), None, None
    steps = loo_steps(S, k_steps, getattr(flags, "loo_draws", 65536))
    if not steps:
        return "more than {} chains".format(diagnostics.PSIS_MAX_DRAWS), None, None
    return None, steps, trace[torch.as_tensor(steps, device=trace.device), :int(k)].contiguous() if int(k) > 0 else None


def replicate_tiles(draws, table, seed, draw_offset=0, y_rep_out=None, budget=None):
    """(draw_stats [S C, 8], obs_sums [N, 4], mask [S C]) on the device: one replicated data set per draw of `draws`
    [S, C, D] (diagnostics.predictive_check), in ascending ppc_tile_rows tiles (within `budget`) of the observations, combined by
    diagnostics.combine_draw_stats.  `y_rep_out` [N, S C] float32 on the device: takes the replicated values themselves."""
    import torch
    rows = ppc_tile_rows(table.N, int(draws.shape[0]) * int(draws.shape[1]), diagnostics.predictive_workspace_bytes, budget)
    stats, sums, mask = None, [], None
    for n0 in range(0, table.N, rows):
        n1 = min(table.N, n0 + rows)
        part, obs, y_rep, mask, _ = diagnostics.predictive_check(draws, table, n0, n1, seed=seed, draw_offset=draw_offset,
                                                                 want_y_rep=y_rep_out is not None)
        stats = part if stats is None else diagnostics.combine_draw_stats(stats, part)
        sums.append(obs)
        if y_rep_out is not None:
            y_rep_out[n0:n1] = y_rep
    return stats, torch.cat(sums, dim=0), mask


def group_range_size(G, R, budget=None):
    """Groups per call of the grouped predictive check: [groups, R, 8] float64 statistics within `budget` bytes
    (LOO_CHUNK_BYTES); at least one."""
    return rows_within(G, 64 * int(R), budget)


def logo_range_size(G, R, forms, workspace_bytes, budget=None):
    """Groups per call of leave-one-group-out: `forms` (1: conditional, 2: and marginal) [groups, R] float32 matrices and
    the PSIS workspace `workspace_bytes(groups, R)` of one of them within `budget` bytes (LOO_CHUNK_BYTES) -- group_range_size
    with this report's rows, halved as ppc_tile_rows halves until the workspace fits too; at least one."""
    row = 4 * int(forms) * int(R)
    return rows_within(G, row, budget, lambda per: row * per + workspace_bytes(per, R))


MM_MAX_BATCH = 4095                 # arp_weighted_moments takes 4096 rows of weights: a batch's and one for the unweighted moments


def mm_batch_size(T, R, D, budget=None):
    """Targets per call of moment matching: the mapped draws [targets, R, D] float32 of diagnostics.affine_rows within
    `budget` bytes (LOO_CHUNK_BYTES); at least one, at most T and at most MM_MAX_BATCH."""
    return rows_within(T, 4 * int(R) * int(D), budget, cap=MM_MAX_BATCH)


def replicate_groups(draws, table, groups, y, group_of, seed, draw_offset=0, left_out=None, budget=None):
    """(counts [G, PPC_COUNTS] float64 numpy, mask [S C] on the device): the data replicated per draw of `draws` [S, C, D]
    and folded per group (diagnostics.group_predictive_check), in ascending ranges of groups whose [groups, S C, 8]
    statistics stay within `budget` (group_range_size); every range is brought to the host and counted by
    diagnostics.ppc_group_counts before the next is launched -- a group's row does not depend on the range it came in.
    left_out: further draws to leave out, [S C] bool on the device (the mixed check's undrawn rows), or-ed to the mask."""
    R = int(draws.shape[0]) * int(draws.shape[1])
    per = group_range_size(groups.G, R, budget)
    counts, left = [], None
    for g0 in range(0, groups.G, per):
        stats, mask, _ = diagnostics.group_predictive_check(draws, table, groups, g0, min(groups.G, g0 + per), seed=seed,
                                                            draw_offset=draw_offset)
        if left is None:
            left = (mask != 0) if left_out is None else ((mask != 0) | left_out)
        counts.append(diagnostics.ppc_group_counts(stats, y, group_of, left, g0))
    return np.concatenate(counts, axis=0), left


def joint_loglik(draws, table, out, tile_rows):
    """(total [S C] float64, mask [S C]): the joint log-likelihood of the table's data at every draw of `draws` [S, C, D], in
    ascending tiles (diagnostics.pointwise_loglik into `out`, loglik_total): the float64 sums compose bit for bit."""
    import torch
    total = torch.zeros(int(draws.shape[0]) * int(draws.shape[1]), dtype=torch.float64, device=draws.device)
    mask = None
    for n0 in range(0, table.N, tile_rows):
        ll, mask, _ = diagnostics.pointwise_loglik(draws, table, n0, min(table.N, n0 + tile_rows), out=out)
        diagnostics.loglik_total(ll, total)
    return total, mask
