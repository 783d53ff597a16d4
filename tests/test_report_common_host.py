"""CPU: what the reports share (autoreparam_amd/report_common.py) and the table of side reports in main.py.  The seed
rule, the one budget rule, the k-hat threshold test and the grouped-file builders against the expressions they replace; the
draw selection's refusals, their order and its draws; the two tile walks on recording stand-ins of the device functions; the
no-trace branch of main._convergence_report for every combination of the
flags; _save_diagnostics on one array per tag; and that neither report_common nor sbc drags main in."""
import itertools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seeds_are_the_spelled_out_expression():
    from autoreparam_amd import main, report_common as rc, sbc
    constants = (main.VI_CHECK_SEED, 0x454E5247, 0x54524A50, main.PPC_SEED, main.PRIOR_SEED, sbc.SBC_SEED)
    assert len(set(constants)) == 6
    for s in (0, 3, 2 ** 63 - 1):
        for c in constants:
            literal = (int(s) * 0x9E3779B97F4A7C15 + c) & 0xFFFFFFFFFFFFFFFF
            assert rc.derived_seed(s, c) == literal and 0 <= literal < 2 ** 64
            assert rc.next_seed(literal) == (literal + 1) & 0xFFFFFFFFFFFFFFFF
    assert rc.next_seed(2 ** 64 - 1) == 0 and rc.next_seed(0) == 1


def test_main_names_are_the_shared_objects(monkeypatch):
    from autoreparam_amd import main, report_common as rc
    for name in ("_finite_or_none", "_nan_max", "_fmt", "probe_steps", "loo_steps", "ppc_tile_rows", "LOO_CHUNK_BYTES",
                 "element_names", "_write_json_atomic", "_above", "_shown", "grouped_head", "data_tail"):
        assert getattr(main, name) is getattr(rc, name), name
    # main.loo_tile_rows is the shared rule within main's own budget, which the tile tests shrink there
    for N, R in ((11566, 65536), (8, 65536), (5, 1 << 30), (1000, 256)):
        assert main.loo_tile_rows(N, R) == rc.loo_tile_rows(N, R) and main.loo_tile_rows(N, R, 4096) == rc.loo_tile_rows(N, R, 4096)
    monkeypatch.setattr(main, "LOO_CHUNK_BYTES", 100 * 4 * 256)
    assert main.loo_tile_rows(1000, 256) == 100 and rc.loo_tile_rows(1000, 256) == 1000


def test_rows_within_is_each_of_the_five_spelled_out_rules():
    """The five sizing rules as they stood before rows_within, spelled out, against the names that now call it."""
    from autoreparam_amd import report_common as rc
    assert rc.LOO_CHUNK_BYTES == 256 << 20 and rc.MM_MAX_BATCH == 4095
    halved = 0
    for count, R, D in itertools.product((0, 1, 7, 4096, 5000), (1, 64, 65536, 1 << 24), (1, 255)):
        for budget in (1, 4 * R, 256 << 20):
            loo = int(max(1, min(max(int(count), 1), budget // max(1, 4 * int(R)))))
            assert rc.loo_tile_rows(count, R, budget) == loo == rc.rows_within(count, 4 * R, budget)
            assert rc.group_range_size(count, R, budget) == int(max(1, min(max(int(count), 1), budget // max(1, 64 * int(R)))))
            assert rc.mm_batch_size(count, R, D, budget) == int(
                max(1, min(max(int(count), 1), rc.MM_MAX_BATCH, budget // max(1, 4 * int(R) * int(D)))))
            if budget == 256 << 20:                                                            # the default budget
                assert rc.loo_tile_rows(count, R) == loo and rc.group_range_size(count, R) == rc.group_range_size(count, R, budget)
                assert rc.mm_batch_size(count, R, D) == rc.mm_batch_size(count, R, D, budget)
            # a workspace that is nothing, linear in the rows, and over the budget whatever the rows
            for workspace in (lambda rows, R: 0, lambda rows, R: 8 * rows * R, lambda rows, R: budget + 1):
                rows = loo
                while rows > 1 and workspace(rows, R) > budget:
                    rows = (rows + 1) // 2
                halved += rows != loo
                assert rc.ppc_tile_rows(count, R, workspace, budget) == rows
                for forms in (1, 2):
                    per = int(max(1, min(max(int(count), 1), budget // max(1, 4 * int(forms) * int(R)))))
                    while per > 1 and 4 * int(forms) * int(R) * per + workspace(per, R) > budget:
                        per = (per + 1) // 2
                    assert rc.logo_range_size(count, R, forms, workspace, budget) == per
                if workspace(1, R) > budget:
                    assert rows == per == 1                                                    # at least one
    assert halved > 0


def test_above_is_each_of_the_six_spelled_out_tests():
    """k-hat above the threshold, or not fitted when there is no threshold: the six expressions _above replaced, on a column
    with finite values on both sides of the threshold, +inf, a NaN and an empty group's all-NaN row."""
    import warnings
    from autoreparam_amd import report_common as rc
    columns = np.array([[0.0, 0.2], [-1.0, 0.9], [-2.0, np.inf], [-3.0, np.nan], [np.nan, np.nan], [-4.0, 0.7]])
    sizes = np.array([3, 2, 1, 4, 0, 5])
    k_all = columns[:, 1]
    filled = ~np.all(np.isnan(columns), axis=1)
    k = np.where(filled, k_all, np.nan)
    same = lambda a, b: a.dtype == bool and b.dtype == bool and np.array_equal(a, b)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                                         # (the guard is _above's)
        for threshold in (0.7, float("nan")):
            with np.errstate(invalid="ignore"):
                loo = int(np.sum(k_all > threshold)) if np.isfinite(threshold) else int(np.sum(~np.isfinite(k_all)))
                form = int(np.sum(k > threshold)) if np.isfinite(threshold) else int(np.sum(filled & ~np.isfinite(k)))
                key = rc._finite_or_none(threshold)                                             # what _logo_report reads back
                warned = (k > key) if key is not None else (sizes > 0) & ~np.isfinite(k)
                select = (k > threshold) if np.isfinite(threshold) else np.isposinf(k)
                keys = (k > threshold) if np.isfinite(threshold) else (filled & ~np.isfinite(k))
            assert int(np.sum(rc._above(k_all, threshold))) == loo == (2 if np.isfinite(threshold) else 3)       # loo_keys
            assert int(np.sum(rc._above(k, threshold, filled))) == form == (2 if np.isfinite(threshold) else 2)  # _logo_form_keys
            assert same(rc._above(k, key, sizes > 0), warned)                                   # _logo_report's warning
            assert same(rc._above(k, threshold, ~np.isnan(k)), select)                          # mm_select, _mm_run's warning
            assert same(rc._above(k, threshold, filled), keys)                                  # mm_keys
        assert list(rc._above(k, 0.7)) == [False, True, True, False, False, False]
        assert list(rc._above(k, None)) == [False, False, True, True, True, False]
        assert list(rc._above(k, None, ~np.isnan(k))) == [False, False, True, False, False, False]


def test_shown_names_the_first_and_says_when_there_are_more():
    from autoreparam_amd import main, report_common as rc
    assert main.LOGO_SHOWN == main.MM_SHOWN == main.PPC_GROUP_SHOWN == main.PPC_MIXED_SHOWN == 8
    for limit in (1, 8):
        for n in (0, limit - 1, limit, limit + 1):
            names = ["m[%d]" % i for i in range(n)]
            assert rc._shown(names, limit) == ", ".join(names[:limit]) + (", ..." if len(names) > limit else "")
            at = np.arange(n) * 3                                                              # indices, as flatnonzero gives them
            assert rc._shown(at, limit) == ", ".join(str(i) for i in at[:limit]) + (", ..." if at.size > limit else "")
            assert rc._shown([int(i) for i in at], limit) == rc._shown(at, limit)
    assert rc._shown(["a", "b", "c"], 2) == "a, b, ..." and rc._shown(["a", "b"], 2) == "a, b" and rc._shown(["a"], 2) == "a"


def test_grouped_file_builders_keep_names_dtypes_and_order(tmp_path):
    """The arrays a grouped side file opens and closes with, as _logo_report and _ppc_group_report spelled them."""
    from autoreparam_amd import report_common as rc
    part, names, group_of, sizes = "m", ["m[0]", "m[1]", "m[2]"], np.array([0, -1, 2, 2]), [1, 0, 2]
    y, spec = np.array([0.5, 1.5, -2.0, 3.0]), types.SimpleNamespace(name="radon")
    want = ([("part", np.asarray(part)), ("groups", np.asarray(names)), ("group_of", np.asarray(group_of, np.int32)),
             ("n_obs", np.asarray(sizes, np.int64))],
            [("y", np.asarray(y, np.float32)), ("model", np.asarray(spec.name))])
    for got, expected in zip((rc.grouped_head(part, names, group_of, sizes), rc.data_tail(y, spec)), want):
        assert [n for n, _ in got] == [n for n, _ in expected]
        for (_, a), (_, b) in zip(got, expected):
            assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    head, tail = rc.grouped_head(part, names, group_of, sizes), rc.data_tail(y, spec)
    assert [a.dtype for _, a in head] == [np.dtype("<U1"), np.dtype("<U4"), np.dtype(np.int32), np.dtype(np.int64)]
    assert tail[0][1].dtype == np.float32 and tail[1][1].shape == () and str(tail[1][1]) == "radon"
    y32 = np.asarray(y, np.float32)
    assert rc.data_tail(y32, spec)[0][1] is y32                                                # float32 as uploaded: no copy
    path = str(tmp_path / "grouped.npz")
    np.savez(path, **dict(head + [("elpd_logo_g", np.zeros(3))] + tail))
    assert np.load(path).files == ["part", "groups", "group_of", "n_obs", "elpd_logo_g", "y", "model"]


FLAGS = types.SimpleNamespace(loo_draws=6)


def test_select_draws_refuses_in_order_before_it_slices():
    from autoreparam_amd import diagnostics, report_common as rc
    none = "no chain has its trace on the device"
    assert rc.select_draws(torch.zeros(4, 0, 5), 0, 0, FLAGS) == (none, None, None)
    assert rc.select_draws(torch.zeros(4, 2, 5), 0, 0, FLAGS) == (none, None, None)
    assert rc.select_draws(torch.zeros(0, 2, 5), 2, 2, FLAGS) == (none, None, None)
    assert rc.select_draws(torch.zeros(0, 2, 300), 2, 2, FLAGS) == (none, None, None)           # the first refusal wins
    assert rc.select_draws(torch.zeros(4, 2, 300), 2, 2, FLAGS) == ("the model has more than 255 elements", None, None)
    many = diagnostics.PSIS_MAX_DRAWS + 1
    assert many == 2 ** 24 + 1
    # a [4, 2, 5] tensor has no 2^24 + 1 chains to slice: the refusal comes first
    assert rc.select_draws(torch.zeros(4, 2, 5), many, many, FLAGS) == ("more than 16777216 chains", None, None)
    assert rc.select_draws(torch.zeros(4, 2, 300), many, many, FLAGS)[0] == "the model has more than 255 elements"


def test_select_draws_takes_the_leading_chains_at_loo_steps():
    from autoreparam_amd import report_common as rc
    trace = torch.arange(7 * 5 * 4, dtype=torch.float32).reshape(7, 5, 4)
    why, steps, draws = rc.select_draws(trace, 3, 3, FLAGS)
    assert why is None and steps == rc.loo_steps(7, 3, 6) == [0, 6]
    assert draws.is_contiguous() and tuple(draws.shape) == (2, 3, 4) and torch.equal(draws, trace[steps, :3])
    draws[0, 0, 0] = -1.0
    assert trace[0, 0, 0] == 0.0                                                            # a copy
    why, steps, draws = rc.select_draws(trace, 0, 3, FLAGS)                                  # the idle rank of a sharded PPC
    assert why is None and draws is None and steps == rc.loo_steps(7, 3, 6)
    assert rc.select_draws(trace, 5, 5, types.SimpleNamespace())[1] == rc.loo_steps(7, 5, 65536)    # the flag's default


N_OBS = 8


@pytest.fixture(params=(1, 3, 8))
def tile_rows(request, monkeypatch):
    """Tiles of 1, 3 and 8 of the 8 observations, for R = 2 draws: the budget is rows x R float32."""
    from autoreparam_amd import diagnostics, report_common as rc
    monkeypatch.setattr(rc, "LOO_CHUNK_BYTES", 4 * 2 * request.param)
    monkeypatch.setattr(diagnostics, "predictive_workspace_bytes", lambda rows, R: 0)
    assert rc.loo_tile_rows(N_OBS, 2) == request.param
    return request.param


def covers_once_ascending(ranges, rows):
    assert ranges == [(n0, min(N_OBS, n0 + rows)) for n0 in range(0, N_OBS, rows)]
    assert [n for n0, n1 in ranges for n in range(n0, n1)] == list(range(N_OBS))


@pytest.mark.parametrize("want_y_rep", (False, True))
def test_replicate_tiles_walks_every_observation_once(tile_rows, want_y_rep, monkeypatch):
    from autoreparam_amd import diagnostics, report_common as rc
    calls, combined = [], []
    draws, table, mask = torch.zeros(1, 2, 3), types.SimpleNamespace(N=N_OBS), torch.zeros(2, dtype=torch.uint8)

    def predictive_check(trace, tab, n0, n1, seed=None, draw_offset=None, want_y_rep=None):
        assert trace is draws and tab is table
        calls.append((n0, n1, seed, draw_offset, want_y_rep))
        rows = torch.arange(n0, n1, dtype=torch.float64)
        y_rep = (rows[:, None] + torch.tensor([0.0, 0.5])).to(torch.float32) if want_y_rep else None
        return torch.ones(2, 8, dtype=torch.float64), rows[:, None].repeat(1, 4), y_rep, mask, None

    def combine_draw_stats(a, b):
        combined.append(1)
        return a + b
    monkeypatch.setattr(diagnostics, "predictive_check", predictive_check)
    monkeypatch.setattr(diagnostics, "combine_draw_stats", combine_draw_stats)
    y_out = torch.full((N_OBS, 2), -1.0) if want_y_rep else None
    stats, obs, got_mask = rc.replicate_tiles(draws, table, 12345, draw_offset=77, y_rep_out=y_out)
    covers_once_ascending([c[:2] for c in calls], tile_rows)
    assert {c[2:] for c in calls} == {(12345, 77, want_y_rep)}
    assert len(combined) == len(calls) - 1 and torch.equal(stats, torch.full((2, 8), float(len(calls)), dtype=torch.float64))
    assert tuple(obs.shape) == (N_OBS, 4) and torch.equal(obs[:, 0], torch.arange(N_OBS, dtype=torch.float64))
    assert got_mask is mask
    if want_y_rep:
        assert torch.equal(y_out, torch.arange(N_OBS, dtype=torch.float32)[:, None] + torch.tensor([0.0, 0.5]))
    calls.clear()
    rc.replicate_tiles(draws, table, 5)                                                     # the defaults of the prior checks
    assert {c[2:] for c in calls} == {(5, 0, False)}
    calls.clear()
    rc.replicate_tiles(draws, table, 5, budget=4 * 2 * 2)                                    # a caller's own budget: tiles of 2
    covers_once_ascending([c[:2] for c in calls], 2)


@pytest.mark.parametrize("rows", (1, 3, 8))
def test_joint_loglik_adds_ascending_tiles(rows, monkeypatch):
    from autoreparam_amd import diagnostics, report_common as rc
    calls, folds = [], []
    draws, table = torch.zeros(1, 2, 3), types.SimpleNamespace(N=N_OBS)
    buffer, mask = torch.zeros(rows, 2), torch.zeros(2, dtype=torch.uint8)

    def pointwise_loglik(trace, tab, n0, n1, out=None):
        assert trace is draws and tab is table and out is buffer
        calls.append((n0, n1))
        out[:n1 - n0] = torch.arange(n0, n1, dtype=torch.float32)[:, None]
        return out[:n1 - n0], mask, None

    def loglik_total(ll, total):
        folds.append(len(calls))
        total += ll.to(torch.float64).sum(dim=0)
    monkeypatch.setattr(diagnostics, "pointwise_loglik", pointwise_loglik)
    monkeypatch.setattr(diagnostics, "loglik_total", loglik_total)
    total, got_mask = rc.joint_loglik(draws, table, buffer, rows)
    covers_once_ascending(calls, rows)
    assert folds == list(range(1, len(calls) + 1))                                          # every tile folded before the next
    assert total.dtype == torch.float64 and torch.equal(total, torch.full((2,), 28.0, dtype=torch.float64)) and got_mask is mask


PARENTS = ("predictive_diagnostics", "predictive_checks", "sensitivity_diagnostics", "prior_predictive_checks")


def flag_sets():
    """All 16 subsets of the four reports with a null path, each with and without --loo_predictive and
    --sensitivity_prior_parts wherever their parent is set."""
    for on in itertools.product((False, True), repeat=4):
        asked = [name for name, v in zip(PARENTS, on) if v]
        children = [c for c, parent in (("--loo_predictive", PARENTS[0]), ("--sensitivity_prior_parts=mu", PARENTS[2]))
                    if parent in asked]
        for n in range(len(children) + 1):
            for chosen in itertools.combinations(children, n):
                yield asked, list(chosen)


def test_side_report_table_is_well_formed():
    from autoreparam_amd import main
    tags = [row.tag for row in main.SIDE_REPORTS]
    assert len(set(tags)) == len(tags) == 9 and all(tag.endswith("/") for tag in tags)
    assert tags == [main.ENERGY_ARRAYS, main.TRAJECTORY_ARRAYS, main.GEOMETRY_ARRAYS, main.LOO_ARRAYS, main.LOO_PRED_ARRAYS,
                    main.PPC_ARRAYS, main.PSENS_ARRAYS, main.PSENS_SITES_ARRAYS, main.PRIOR_ARRAYS]
    assert all(callable(row.save) for row in main.SIDE_REPORTS)
    assert [row.flag for row in main.SIDE_REPORTS if row.null is not None] == list(PARENTS)
    assert [row.tag for row in main.SIDE_REPORTS if row.report is None] == [main.LOO_PRED_ARRAYS, main.PSENS_SITES_ARRAYS]
    assert len(list(flag_sets())) == 36 and len({tuple(a) for a, _ in flag_sets()}) == 16


def test_no_trace_writes_the_null_keys_of_what_was_asked(capsys):
    from autoreparam_amd import main, models
    from autoreparam_amd.flags import FlagValues

    class Results(object):
        trace = None
    cfg = type("Cfg", (), {"model": models._spec_eight_schools()})()
    for asked, children in flag_sets():
        f = FlagValues()
        f.parse(["--" + name for name in asked] + children)
        capsys.readouterr()
        keys, arrays = main._convergence_report(Results(), cfg, f, None)
        lines = [l for l in capsys.readouterr().out.splitlines() if "not computed" in l]
        expected = ()
        for name, own, child, more in ((PARENTS[0], main.LOO_KEYS, "--loo_predictive", main.LOO_PRED_KEYS),
                                       (PARENTS[1], main.PPC_KEYS, None, ()),
                                       (PARENTS[2], main.PSENS_KEYS, "--sensitivity_prior_parts=mu", main.PSENS_SITE_KEYS),
                                       (PARENTS[3], main.PRIOR_KEYS, None, ())):
            if name in asked:
                expected += own + (more if child in children else ())
        assert tuple(keys) == expected, (asked, children)
        assert all(v is None for v in keys.values()) and arrays is None
        assert len(lines) == len(asked) and all("no chain has its trace on the device" in l for l in lines), (asked, lines)
        if not asked:
            assert (keys, arrays) == ({}, None)
        f.parse(["--noconvergence_diagnostics"])
        assert main._convergence_report(Results(), cfg, f, None) == ({}, None) and capsys.readouterr().out == ""


def test_save_diagnostics_writes_one_file_per_tag(tmp_path):
    from autoreparam_amd import main
    arrays = {"split_rhat/mu": np.zeros(1)}
    for i, row in enumerate(main.SIDE_REPORTS):
        arrays[row.tag] = {"a": np.full(1, float(i))}
    main._save_diagnostics(str(tmp_path / "CP"), arrays)
    names = ("rhat", "energy", "trajectory", "geometry", "loo", "loopred", "ppc", "psens", "psens_sites", "prior")
    assert sorted(os.listdir(str(tmp_path))) == sorted("CP_%s.npz" % n for n in names)
    assert np.load(str(tmp_path / "CP_rhat.npz")).files == ["split_rhat/mu"]
    for i, n in enumerate(names[1:]):
        z = np.load(str(tmp_path / ("CP_%s.npz" % n)))
        assert z.files == ["a"] and z["a"][0] == i, n
    main._save_diagnostics(str(tmp_path / "none"), None)
    assert len(os.listdir(str(tmp_path))) == 10


def test_neither_report_common_nor_sbc_imports_main():
    script = ("import sys\n"
              "import autoreparam_amd.report_common\n"
              "assert 'autoreparam_amd.main' not in sys.modules and 'autoreparam_amd.sbc' not in sys.modules\n"
              "import autoreparam_amd.sbc\n"
              "assert 'autoreparam_amd.main' not in sys.modules\n")
    r = subprocess.run([sys.executable, "-c", script], cwd=ROOT, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
