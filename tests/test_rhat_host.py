"""CPU: the host half of the convergence diagnostics (autoreparam_amd/diagnostics.py, main._convergence_report) against
the float64 restatement in tests/rhat_ref.py.  The kernels' half is tests/test_gpu_rhat.py."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import rhat_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KEYS = ("split_rhat_max", "split_rhat_chains", "rhat_max_all_chains", "diagnostics_time_sec")


def numpy_sums(trace, split):
    """What arp_moments_fold returns, formed in numpy from the reference's per-row moments: [5, D]."""
    mean, var = rhat_ref.moments(trace, split)
    D = mean.shape[-1]
    mean, var = mean.reshape(-1, D), var.reshape(-1, D)
    ok = np.isfinite(var)
    z = lambda a: np.where(ok, a, 0.0).sum(axis=0)
    return np.stack([ok.sum(axis=0).astype(np.float64), z(mean), z(mean * mean), z(var), (ok & (var == 0)).sum(axis=0) * 1.0])


def _trace(S, C, D, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(S, C, D) * (1.0 + np.arange(D)) + 0.3 * rs.randn(1, C, D) + 2.0 * np.arange(D)
    return x.astype(np.float32)


def _check(x, split):
    from autoreparam_amd import diagnostics
    n = x.shape[0] // 2 if split else x.shape[0]
    got = diagnostics.rhat_from_sums(numpy_sums(x, split), n)
    want = rhat_ref.rhat(x, split)
    np.testing.assert_allclose(got.rhat, want[0], rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(got.mean, want[1], rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(got.sd, want[2], rtol=1e-12, equal_nan=True)
    assert np.array_equal(got.constant_rows, want[3])
    return got


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("S,C", [(200, 16), (201, 7), (51, 2), (40, 1), (7, 5)])
def test_rhat_from_sums_equals_the_reference(S, C, split):
    got = _check(_trace(S, C, 6, seed=S + C), split)
    m = C * (2 if split else 1)
    assert np.array_equal(got.rows, np.full(6, m))
    assert np.isfinite(got.rhat).all() == (m >= 2)          # one row: NaN, not an exception


def test_constant_chains():
    x = _trace(120, 6, 4, seed=1)
    x[:, 2, :] = x[0, 2, :]                                  # one chain never moved: it counts, with variance 0
    for split in (False, True):
        got = _check(x, split)
        assert np.isfinite(got.rhat).all() and np.array_equal(got.constant_rows, np.full(4, 2 if split else 1))
    x[:] = x[:1]                                             # none moved: W = 0 -> NaN
    for split in (False, True):
        got = _check(x, split)
        assert np.isnan(got.rhat).all() and np.array_equal(got.constant_rows, got.rows)


def test_tiny_runs_end_in_nan():
    from autoreparam_amd import diagnostics
    for S in (1, 2, 3):
        x = _trace(S, 4, 3, seed=S)
        got = _check(x, True)                                # halves of 0 or 1 draws: no finite variance anywhere
        assert np.isnan(got.rhat).all() and np.array_equal(got.rows, np.zeros(3))
    assert np.isnan(diagnostics.rhat_from_sums(np.zeros((5, 3)), 0).rhat).all()      # a job without chains


def test_sums_are_additive_over_chain_blocks():
    x = _trace(90, 11, 5, seed=4)
    for split in (False, True):
        whole = numpy_sums(x, split)
        np.testing.assert_allclose(numpy_sums(x[:, :4], split) + numpy_sums(x[:, 4:], split), whole, rtol=1e-12)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _rank(rank, ws, port, out_dir):
    from autoreparam_amd import parallel
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    x = _trace(90, 11, 5, seed=4)
    lo, hi = parallel.shard_bounds(x.shape[1], rank, ws)
    total = parallel.all_reduce_sum(torch.as_tensor(numpy_sums(x[:, lo:hi], True))).numpy()
    np.save(os.path.join(out_dir, "sums%d.npy" % rank), total)
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_sums(tmp_path):
    from autoreparam_amd import diagnostics
    mp.spawn(_rank, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = (np.load(os.path.join(str(tmp_path), "sums%d.npy" % r)) for r in range(2))
    assert np.array_equal(a, b)
    x = _trace(90, 11, 5, seed=4)
    np.testing.assert_allclose(a, numpy_sums(x, True), rtol=1e-12)
    np.testing.assert_allclose(diagnostics.rhat_from_sums(a, 45).rhat, rhat_ref.rhat(x, True)[0], rtol=1e-10)


@pytest.mark.parametrize("delta", [0.5, 1.0, 2.0])
def test_known_answer_for_shifted_chains(delta):
    """m chains of n i.i.d. N(0, 1) draws, half of them shifted by delta:  W -> 1 and B/n -> 1/n + delta^2/4 m/(m-1), so
    rhat^2 -> (n-1)/n + 1/n + delta^2/4 m/(m-1).  Sampling error of the statistic for THIS n and m (delta method, W and
    B independent for normal draws):  sd(W) = sqrt(2 / ((n-1) m));  B/n is the sample variance of m row means with
    fixed offsets a_i (sum a_i^2 = m delta^2/4) and noise of variance 1/n, so
    var(B/n) = 4 sum a_i^2 / (n (m-1)^2) + 2 / (n^2 (m-1));  sd(rhat^2) = sqrt(var(B/n) + E[B/n]^2 sd(W)^2).
    Allowed: 5 of those standard deviations (n = 200, m = 400: 0.010 / 0.019 / 0.038 at delta = 0.5 / 1 / 2, against
    effects of 0.06 / 0.25 / 1.0), seed 11."""
    from autoreparam_amd import diagnostics
    n, m = 200, 400
    rs = np.random.RandomState(11)
    x = rs.randn(n, m, 1).astype(np.float32)
    x[:, : m // 2] += np.float32(delta)
    expect_b = 1.0 / n + delta ** 2 / 4.0 * m / (m - 1.0)
    expect = (n - 1.0) / n + expect_b
    sd_w = np.sqrt(2.0 / ((n - 1.0) * m))
    var_b = m * delta ** 2 / (n * (m - 1.0) ** 2) + 2.0 / (n ** 2 * (m - 1.0))
    allowed = 5.0 * np.sqrt(var_b + (expect_b * sd_w) ** 2)
    got = diagnostics.rhat_from_sums(numpy_sums(x, False), n).rhat[0] ** 2
    print("delta %.1f: rhat^2 %.5f, expected %.5f, allowed deviation %.5f" % (delta, got, expect, allowed))
    assert abs(got - expect) < allowed
    assert abs(rhat_ref.rhat(x, False)[0][0] ** 2 - expect) < allowed        # (the yardstick meets it too)


def test_header_declares_and_binding_lists_the_three_symbols():
    from autoreparam_amd import _lib
    src = open(os.path.join(ROOT, "include", "autoreparam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("arp_moments_workspace_bytes", "arp_split_moments", "arp_moments_fold"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SYMBOLS, name
    assert "#define ARP_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "autoreparam.h")).read()


def test_kernel_results_keep_their_positional_form():
    from autoreparam_amd import inference
    kr = inference.KernelResults(inference.HmcInnerResults(None), 1.0, 3, None)
    assert kr.moments is None and kr.trace is None and kr._fields[-1] == "trace"
    ikr = inference.InterleavedKernelResults(kr, kr, ess_info=None)
    assert ikr.moments is None and ikr.trace is None


@pytest.mark.parametrize("case", ["no_trace", "flag_off"])
@pytest.mark.parametrize("method", ["CP", "i"])
def test_no_trace_or_flag_off_adds_no_key_and_no_file(tmp_path, monkeypatch, case, method):
    """Kernel results that carry no device trace (every stand-in engine of tests/test_distributed.py), or
    --noconvergence_diagnostics with a trace at hand: the record handed to save_hmc_results has none of the new keys
    and no _rhat.npz appears."""
    from test_distributed import _fake_engine
    from autoreparam_amd import inference, main as cli
    from autoreparam_amd.flags import FLAGS
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    for name in ("find_best_learning_rate", "hmc", "hmc_interleaved"):
        monkeypatch.setattr(inference, name, getattr(inference, name))       # restored after _fake_engine replaces them
    _fake_engine(None)
    if case == "flag_off":
        fake_hmc, fake_inter = inference.hmc, inference.hmc_interleaved

        def with_trace(kr, flags, n):
            return kr._replace(trace=torch.zeros(int(flags.num_samples), n, 10))

        def hmc(*a, **kw):
            r = fake_hmc(*a, **kw)
            return (r[0], with_trace(r[1], kw["flags"], len(r[3][0]))) + tuple(r[2:])

        def inter(*a, **kw):
            r = fake_inter(*a, **kw)
            return (r[0], with_trace(r[1], kw["flags"], len(r[2][0]))) + tuple(r[2:])
        monkeypatch.setattr(inference, "hmc", hmc)
        monkeypatch.setattr(inference, "hmc_interleaved", inter)
    records = []
    real_save = cli.save_hmc_results
    monkeypatch.setattr(cli, "save_hmc_results", lambda file_path, **rec: (records.append(rec), real_save(file_path, **rec)))
    d = str(tmp_path)
    base = ["--model=8schools", "--results_dir=" + d, "--num_chains=5", "--num_samples=12", "--num_burnin_steps=4",
            "--num_adaptation_steps=3", "--num_chains_to_save=2"]
    if case == "flag_off":
        base.append("--noconvergence_diagnostics")
    for m in ("CP", "NCP"):
        cli.main(base + ["--inference=VI", "--method=" + m], flags=FLAGS.copy())
        cli.main(base + ["--inference=HMCtuning", "--method=" + m, "--num_leapfrog_steps=2"], flags=FLAGS.copy())
    records.clear()
    cli.main(base + ["--inference=HMC", "--method=" + method], flags=FLAGS.copy())
    assert len(records) == 1 and "ess_min" in records[0]
    assert not set(NEW_KEYS) & set(records[0])
    assert not [f for f in os.listdir(d) if f.endswith("_rhat.npz")]
    assert [f for f in os.listdir(d) if f.endswith("_ess.npz")]


def test_flag_defaults_on_and_parses_both_ways():
    from autoreparam_amd.flags import FlagValues
    f = FlagValues()
    assert f.convergence_diagnostics is True
    f.parse(["--noconvergence_diagnostics"]); assert f.convergence_diagnostics is False
    f.parse(["--convergence_diagnostics"]); assert f.convergence_diagnostics is True


@pytest.mark.parametrize("name", ["split_moments", "rank_normalize", "ess_multichain"])
def test_wrappers_refuse_what_is_not_a_float32_device_trace(name):
    """Every wrapper of a diagnostics kernel names itself when it refuses a trace: one on the CPU, of another type, or not
    [S, C, D] -- before anything is allocated or the library is loaded."""
    from autoreparam_amd import diagnostics
    message = re.escape(name + ": a float32 [S, C, D] trace on the GPU is required (there is no CPU fallback)")
    for bad in (torch.zeros(4, 2, 3), torch.zeros(4, 2, 3, dtype=torch.float64), torch.zeros(4, 6)):
        with pytest.raises(ValueError, match="^" + message + "$"):
            getattr(diagnostics, name)(bad)
