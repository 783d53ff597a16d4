"""CPU: the host half of the rank-normalised R-hat (flags, main._convergence_report's sharded-job rule, the ABI lists) and
the float64 yardstick tests/rank_rhat_ref.py itself.  The kernels' half is tests/test_gpu_rank.py."""
import os
import re
import types

import numpy as np
import pytest
import torch

import rank_rhat_ref
import rhat_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK_KEYS = ("rank_rhat_max", "rank_rhat_bulk_max", "rank_rhat_tail_max", "rank_rhat_chains", "rank_rhat_time_sec")


def test_flag_defaults_off_and_parses_both_ways():
    from autoreparam_amd.flags import FlagValues
    f = FlagValues()
    assert f.rank_normalized_rhat is False
    f.parse(["--rank_normalized_rhat"]); assert f.rank_normalized_rhat is True
    f.parse(["--norank_normalized_rhat"]); assert f.rank_normalized_rhat is False


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_yardstick_sees_what_the_classic_statistic_cannot(seed):
    """64 chains x 400 draws: the classic split R-hat calls all three elements converged; the folded statistic sees the
    16 chains at 3 x the scale, the rank-normalised one the 16 shifted Cauchy chains."""
    x = rank_rhat_ref.table_input(seed)
    classic = rhat_ref.rhat(x, True)[0]
    r = rank_rhat_ref.rank_rhat(x)
    print("seed %d: classic %s bulk %s tail %s" % (seed, classic, r["bulk"], r["tail"]))
    assert (classic < 1.01).all()
    assert r["tail"][1] > 1.04 and r["bulk"][2] > 1.04 and r["rhat"][0] < 1.01


def test_yardstick_ranks_ties_zeros_and_quantiles():
    x = np.array([3.0, -0.0, 0.0, 3.0, 3.0, -1.0, 1e-45, -1e-45], np.float32).reshape(4, 2, 1)
    # sorted: -1, -1e-45, (-0, +0), 1e-45, 3, 3, 3
    want = np.array([5 + 8, 2 + 4, 2 + 4, 5 + 8, 5 + 8, 0 + 1, 4 + 5, 1 + 2], np.uint32)
    assert np.array_equal(rank_rhat_ref.rank2(x).reshape(-1), want)
    # rank2 = 2 (average rank) - 1: scipy's own ranks
    from scipy.stats import rankdata
    assert np.array_equal(2 * rankdata(x.reshape(-1), method="average") - 1, want)
    assert rank_rhat_ref.median(x)[0] == np.float32(0.5) * (np.float32(0.0) + np.float32(1e-45))
    q = rank_rhat_ref.quantiles(x, (0.0, 0.05, 0.5, 0.95, 1.0))[:, 0]
    assert list(q) == [-1.0, -1.0, 0.0, 3.0, 3.0]
    z = rank_rhat_ref.z_scores(rank_rhat_ref.rank2(x), 8)
    assert z[0, 1, 0] == z[1, 0, 0] and z[2, 1, 0] == -rank_rhat_ref.z_scores(np.array([15]), 8)[0]   # the zeros tie; symmetric
    assert rank_rhat_ref.z_scores(np.array([8]), 8)[0] == 0.0                                          # the middle rank


def test_sharded_job_writes_null_keys_without_touching_the_device_function(monkeypatch):
    """World size 2: the five keys are there, null, rank_rhat_chains == 0, and neither rank_rhat nor rank_normalize runs."""
    from autoreparam_amd import diagnostics, main as cli, models, parallel
    from autoreparam_amd.flags import FlagValues
    cfg = models.get_model_by_name("8schools", "")
    D = cfg.model.D
    S, Cn = 20, 4
    x = np.random.RandomState(0).randn(S, Cn, D).astype(np.float32)

    def moments(trace, split=True):
        m, v = rhat_ref.moments(trace.numpy(), split)
        return torch.as_tensor(m), torch.as_tensor(v)

    def fold(mean, var):
        m, v = mean.reshape(-1, D).numpy().astype(np.float64), var.reshape(-1, D).numpy().astype(np.float64)
        ok = np.isfinite(v)
        z = lambda a: np.where(ok, a, 0.0).sum(axis=0)
        return torch.as_tensor(np.stack([ok.sum(axis=0) * 1.0, z(m), z(m * m), z(v), (ok & (v == 0)).sum(axis=0) * 1.0]))

    def never(*a, **kw):
        raise AssertionError("the device function was called")

    monkeypatch.setattr(diagnostics, "split_moments", moments)
    monkeypatch.setattr(diagnostics, "fold", fold)
    monkeypatch.setattr(diagnostics, "rank_rhat", never)
    monkeypatch.setattr(diagnostics, "rank_normalize", never)
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    monkeypatch.setattr(parallel, "all_reduce_sum", lambda value, device=None: torch.as_tensor(np.asarray(value)))
    kr = types.SimpleNamespace(trace=torch.as_tensor(x), ess_info=None, moments=None)
    f = FlagValues()
    base_keys, base_arrays = cli._convergence_report(kr, cfg, f, None)
    assert not set(RANK_KEYS) & set(base_keys)
    f.rank_normalized_rhat = True
    keys, arrays = cli._convergence_report(kr, cfg, f, None)
    assert set(keys) == set(base_keys) | set(RANK_KEYS)
    assert keys["rank_rhat_chains"] == 0
    assert all(keys[k] is None for k in RANK_KEYS if k != "rank_rhat_chains")
    assert sorted(arrays) == sorted(base_arrays)
    assert keys["split_rhat_max"] == base_keys["split_rhat_max"]


def test_header_declares_and_binding_lists_the_two_symbols():
    from autoreparam_amd import _lib
    src = open(os.path.join(ROOT, "include", "autoreparam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("arp_rank_workspace_bytes", "arp_rank_normalize"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SYMBOLS, name
    assert "#define ARP_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "autoreparam.h")).read()
