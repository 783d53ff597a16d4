"""GPU: the convergence diagnostics' kernels (csrc/diag.hip: arp_split_moments, arp_moments_fold) and their way up to
the CLI, against the float64 restatement in tests/rhat_ref.py applied to the same float32 trace.

Tolerance of the moments (check_moments): a float32 numpy emulation of the kernel's chunked arithmetic (`emulate`: shifted
sums per chunk of 256 rows, means carried as offsets from the part's first row, chunks merged pairwise, left to right) measures on each input what the arithmetic itself
loses against float64; the kernel is allowed 4 x that (fma contraction, nothing else differs) and never more than the
project's rtol = 1e-3.  The variance's error is relative, the mean's is in units of the series' standard deviation.
Measured (emulation / MI355X), see DESIGN.md section 6."""
import json
import os
import shutil

import numpy as np
import pytest

import rhat_ref

pytestmark = pytest.mark.gpu

CHUNK = 256
CAP = 1e-3
NEW_KEYS = ("split_rhat_max", "split_rhat_chains", "rhat_max_all_chains", "diagnostics_time_sec")


def emulate(x, split):
    """float32 numpy emulation of arp_split_moments' arithmetic on x [S, N] float32 -> (mean, var) [P, N] float32."""
    f = np.float32
    S, N = x.shape
    P, n = (2, S // 2) if split else (1, S)
    mean, var = np.full((P, N), np.nan, f), np.full((P, N), np.nan, f)
    for p, start in enumerate((0, S - n)[:P]):
        if n == 0:
            continue
        na, ref0 = f(0), x[start]
        for r0 in range(0, n, CHUNK):
            rows = x[start + r0: start + min(r0 + CHUNK, n)]
            ref, s1, s2 = rows[0], np.zeros(N, f), np.zeros(N, f)
            for r in rows[1:]:
                d = r - ref
                s1 = s1 + d
                s2 = s2 + d * d
            c = f(len(rows))
            a = s1 / c
            mb, m2b = (ref - ref0) + a, np.maximum(s2 - s1 * a, f(0))
            if r0 == 0:
                m, m2 = mb, m2b
            else:
                tot = na + c
                delta, w = mb - m, c / tot
                m = m + delta * w
                m2 = (m2 + m2b) + (delta * delta) * (na * w)
            na = na + c
        mean[p] = ref0 + m
        if n > 1:
            var[p] = m2 / f(n - 1)
    return mean, var


def errors(mean, var, x, split):
    """(max |mean - mean64| / sd64, max |var - var64| / var64) over EVERY series of x [S, N]; parts of one row (var NaN on
    both sides) count through their mean, in units of |mean64| + 1."""
    m64, v64 = rhat_ref.moments(x, split)
    mean, var = np.asarray(mean, np.float64).reshape(m64.shape), np.asarray(var, np.float64).reshape(v64.shape)
    assert np.array_equal(np.isnan(v64), np.isnan(var)) and np.array_equal(np.isnan(m64), np.isnan(mean))
    if not np.isfinite(v64).any():
        return (np.nanmax(np.abs(mean - m64) / (np.abs(m64) + 1)) if np.isfinite(m64).any() else 0.0), 0.0
    assert (v64 > 0).all()
    return np.max(np.abs(mean - m64) / np.sqrt(v64)), np.max(np.abs(var - v64) / v64)


def check_moments(x, split, got, label):
    """x [S, C, D] float32 (numpy); got = (mean, var) tensors from the kernel.  Prints every figure, then asserts."""
    S = x.shape[0]
    flat = x.reshape(S, -1)
    emu = errors(*emulate(flat, split), flat, split)
    gpu = errors(got[0].cpu().numpy(), got[1].cpu().numpy(), flat, split)
    tol = tuple(min(4.0 * e, CAP) for e in emu)
    print("%s split=%d: mean err (sd) emulation %.3g gpu %.3g allowed %.3g | var err (rel) emulation %.3g gpu %.3g allowed %.3g"
          % (label, split, emu[0], gpu[0], tol[0], emu[1], gpu[1], tol[1]))
    assert gpu[0] <= tol[0] and gpu[1] <= tol[1], (label, split, emu, gpu)
    return emu, gpu


def ar1_family(S, Cn, D, seed):
    """The ESS tests' scaled and offset AR(1) family (tests/test_gpu_edges.py)."""
    from oracle import ess_ref
    rho = np.array([0.0, 0.3, 0.6, 0.9, -0.4])[:D]
    scale, offset = np.array([1.0, 10.0, 0.1, 3.0, 1.0])[:D], np.array([0.0, 100.0, -5.0, 1e3, 0.0])[:D]
    return (ess_ref.ar1(S, (Cn, D), rho, seed=seed) * scale + offset).astype(np.float32)


def test_split_moments_ar1_family_and_adversarial_element(gpu):
    import torch
    from autoreparam_amd import diagnostics
    for S in (600, 601):                                     # even, odd (the middle row is dropped)
        x = ar1_family(S, 37, 5, seed=5)
        x[:, :, 4] = (1e3 + 0.1 * np.random.RandomState(S).randn(S, 37)).astype(np.float32)   # mean 10^3, sd 0.1
        xd = torch.as_tensor(x, device=gpu)
        for split in (True, False):
            got = diagnostics.split_moments(xd, split)
            assert got[0].shape == ((2 if split else 1), 37, 5)
            check_moments(x, split, got, "ar1 [%d, 37, 5]" % S)
            again = diagnostics.split_moments(xd, split)
            assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])       # bitwise reproducible


@pytest.mark.parametrize("S", [1, 2, 3])
def test_split_moments_tiny_runs(gpu, S):
    """A part of one row has var = NaN (and its mean = the row); an empty part (S = 1, split) is NaN altogether; no error."""
    import torch
    from autoreparam_amd import diagnostics
    x = ar1_family(S, 6, 5, seed=S)
    xd = torch.as_tensor(x, device=gpu)
    for split in (True, False):
        mean, var = diagnostics.split_moments(xd, split)
        n = S // 2 if split else S
        assert bool(torch.isnan(var).all()) == (n < 2)
        if n == 1:
            assert np.array_equal(mean.cpu().numpy(), rhat_ref.moments(x, split)[0].astype(np.float32))
        check_moments(x, split, (mean, var), "tiny S=%d" % S)


def test_constant_series_have_variance_zero_exactly(gpu):
    import torch
    from autoreparam_amd import diagnostics
    x = ar1_family(700, 9, 5, seed=2)
    x[:, 4, :] = x[0, 4, :]                                  # a chain that never moved, offsets up to 10^3
    x[350:, 7, 3] = x[350, 7, 3]                              # one that stopped half-way: constant second half only
    xd = torch.as_tensor(x, device=gpu)
    mean, var = diagnostics.split_moments(xd, True)
    assert (var[:, 4] == 0).all() and torch.equal(mean[0, 4], xd[0, 4]) and torch.equal(mean[1, 4], xd[0, 4])
    assert var[1, 7, 3] == 0 and var[0, 7, 3] > 0
    mean, var = diagnostics.split_moments(xd, False)
    assert (var[0, 4] == 0).all() and var[0, 7, 3] > 0


@pytest.mark.parametrize("Cn,D", [(37, 5), (40, 6)])
def test_chain_sub_range_view_is_bitwise_the_full_result(gpu, Cn, D):
    """xd[:, 3:11, :] is taken in place (rows stay rows, the pointer moves): the same rows of the full result bit for bit,
    whether a column is reached by a 16-byte or a 4-byte load ([.., 40, 6]: the full trace qualifies for 16 B, the view,
    18 floats in, does not)."""
    import torch
    from autoreparam_amd import diagnostics
    x = np.random.RandomState(3).randn(600, Cn, D).astype(np.float32) * 3 + 50
    xd = torch.as_tensor(x, device=gpu)
    for split in (True, False):
        full = diagnostics.split_moments(xd, split)
        view = diagnostics.split_moments(xd[:, 3:11, :], split)
        assert torch.equal(view[0], full[0][:, 3:11]) and torch.equal(view[1], full[1][:, 3:11])
        lead = diagnostics.split_moments(xd[:, :8, :], split)
        assert torch.equal(lead[0], full[0][:, :8]) and torch.equal(lead[1], full[1][:, :8])


def test_long_trace_takes_the_two_launch_route(gpu):
    import torch
    from autoreparam_amd import _lib, diagnostics
    S, Cn, D = 50000, 16, 125                                # 2 000 series of 50 000 rows
    assert _lib.lib().arp_moments_workspace_bytes(S, Cn * D, 1) > 0
    rs = np.random.default_rng(8)
    x = rs.standard_normal((S, Cn, D), dtype=np.float32) * (0.1 + np.arange(D, dtype=np.float32) % 7) + \
        (np.arange(D, dtype=np.float32) * 8 - 200)
    x[:, :, 3] = 1e3 + 0.1 * rs.standard_normal((S, Cn), dtype=np.float32)
    xd = torch.as_tensor(x, device=gpu)
    for split in (True, False):
        check_moments(x, split, diagnostics.split_moments(xd, split), "long [50000, 16, 125]")


def test_wide_trace_takes_one_launch(gpu):
    import torch
    from autoreparam_amd import _lib, diagnostics
    S, Cn, D = 24, 8192, 128                                 # 1 048 576 series
    assert _lib.lib().arp_moments_workspace_bytes(S, Cn * D, 1) == 0
    assert _lib.lib().arp_moments_workspace_bytes(1000, 65536 * 85, 1) == 0       # the sampler's own trace
    rs = np.random.default_rng(9)
    x = rs.standard_normal((S, Cn, D), dtype=np.float32) * 2 + (np.arange(D, dtype=np.float32) - 60)
    xd = torch.as_tensor(x, device=gpu)
    for split in (True, False):
        check_moments(x, split, diagnostics.split_moments(xd, split), "wide [24, 8192, 128]")


@pytest.mark.parametrize("Cn,D", [(1024, 85), (333, 7)])
def test_both_routes_forced_on_one_input_agree_bitwise(gpu, monkeypatch, Cn, D):
    """ARP_MOMENTS_ROUTE (an ARP_DEBUG switch) overrides the library's choice: the one-launch and the two-launch route
    give every series the same bits (same chunks, same merge order), and both meet the tolerance."""
    import torch
    from autoreparam_amd import _lib, diagnostics
    S = 1500
    rs = np.random.default_rng(10)
    x = rs.standard_normal((S, Cn, D), dtype=np.float32) * 0.5 + 30
    xd = torch.as_tensor(x, device=gpu)
    monkeypatch.setenv("ARP_DEBUG", "1")
    out = {}
    for route in ("wide", "long"):
        monkeypatch.setenv("ARP_MOMENTS_ROUTE", route)
        assert (_lib.lib().arp_moments_workspace_bytes(S, Cn * D, 1) > 0) == (route == "long")
        for split in (True, False):
            out[route, split] = diagnostics.split_moments(xd, split)
            check_moments(x, split, out[route, split], "forced %s [1500, %d, %d]" % (route, Cn, D))
    for split in (True, False):
        assert torch.equal(out["wide", split][0], out["long", split][0])
        assert torch.equal(out["wide", split][1], out["long", split][1])


@pytest.mark.parametrize("D", [1, 10, 85, 125])
@pytest.mark.parametrize("Cn", [1, 63, 4096, 65536])
def test_fold_against_numpy(gpu, Cn, D):
    import torch
    from autoreparam_amd import diagnostics
    rs = np.random.RandomState(Cn + D)
    mean = (rs.randn(Cn, D) * 3 + 100).astype(np.float32)
    var = (rs.rand(Cn, D) + 0.1).astype(np.float32)
    var[rs.rand(Cn, D) < 0.05] = np.nan
    var[rs.rand(Cn, D) < 0.05] = 0.0
    var[rs.rand(Cn, D) < 0.01] = np.inf
    md, vd = torch.as_tensor(mean, device=gpu), torch.as_tensor(var, device=gpu)
    got = diagnostics.fold(md, vd)
    assert got.dtype == torch.float64 and got.shape == (5, D)
    ok = np.isfinite(var)
    m64, v64 = mean.astype(np.float64), var.astype(np.float64)
    z = lambda a: np.where(ok, a, 0.0).sum(axis=0)
    g = got.cpu().numpy()
    assert np.array_equal(g[0], ok.sum(axis=0)) and np.array_equal(g[4], (var == 0).sum(axis=0))
    for k, want in ((1, z(m64)), (2, z(m64 * m64)), (3, z(v64))):
        np.testing.assert_allclose(g[k], want, rtol=1e-12, atol=0)
    assert torch.equal(got, diagnostics.fold(md, vd))                                    # two runs, the same bits
    assert torch.equal(got, diagnostics.fold(md.reshape(1, Cn, D), vd.reshape(1, Cn, D)))
    assert (diagnostics.fold(md[:0], vd[:0]) == 0).all()                                 # a rank without chains


def rhat_allowance(trace, split, eps_mean, eps_var):
    """What errors of at most eps_mean [rows, D] on the rows' means and eps_var [rows, D] on their variances can do to
    (rhat, pooled mean, pooled sd), element by element, from the float64 moments of `trace` [S, C, D]:
    dW <= mean(eps_var);  with a_c = mean_c - centre and e = max_c eps_mean (every centred mean moves by at most 2 e),
    d(B/n) <= (4 e sum |a_c| + 4 m e^2) / (m - 1);  var+ = (n-1)/n W + B/n, rhat^2 = var+ / W."""
    mean, var = rhat_ref.moments(trace, split)
    n = rhat_ref.parts(trace, split).shape[1]
    D = mean.shape[-1]
    mean, var = mean.reshape(-1, D), var.reshape(-1, D)
    m = mean.shape[0]
    w = var.mean(axis=0)
    a = mean - mean.mean(axis=0)
    b_n = (a * a).sum(axis=0) / (m - 1)
    d_w = eps_var.mean(axis=0)
    e = eps_mean.max(axis=0)
    d_b = (4 * e * np.abs(a).sum(axis=0) + 4 * m * e * e) / (m - 1)
    plus = (n - 1.0) / n * w + b_n
    d_plus = d_w + d_b
    r2_hi, r2_lo = (plus + d_plus) / (w - d_w), np.maximum(plus - d_plus, 0) / (w + d_w)
    r = np.sqrt(plus / w)
    d_sd = np.maximum(np.sqrt(plus + d_plus) - np.sqrt(plus), np.sqrt(plus) - np.sqrt(np.maximum(plus - d_plus, 0)))
    return np.maximum(np.sqrt(r2_hi) - r, r - np.sqrt(r2_lo)), e, d_sd, d_w / w


def test_both_routes_on_one_sampler_run(gpu):
    """A radon MN run through inference.hmc with the whole trace and again streaming (same seed, same samples:
    test_gpu_cli.test_streaming_trace_mode_equals_whole_trace).  Whole trace: split R-hat through the kernels, allowed
    what the moments' own tolerance (CAP: 1e-3 sd on a mean, 1e-3 relative on a variance) implies.  Streaming: the
    un-split R-hat of every chain from the in-kernel statistics planes against the reference on the whole trace, allowed
    what the planes' documented accuracy -- 2e-6 (max|x| + 1) on a mean, 2e-6 (max|x| + 1)^2 on a variance
    (tests/test_gpu_hmc.py) -- plus the float32 rounding of the values handed to arp_moments_fold implies through W and
    B; that bound on W stays below 10 % of every W.  No element is left out."""
    from autoreparam_amd import diagnostics, flags as flags_mod, graphs, inference, models
    cfg = models.get_model_by_name("radon", "MN")
    sp = cfg.model
    f = flags_mod.FlagValues()
    f.num_chains, f.num_samples, f.num_burnin_steps, f.num_adaptation_steps, f.num_leapfrog_steps = 96, 400, 100, 80, 4
    target, *_ = graphs.make_cp_graph(cfg, flags=f)
    rs = np.random.RandomState(0)
    init = [0.1 * rs.randn(96, *s).astype(np.float32) for s in sp.part_shapes]
    step = [0.15] * 3 + [np.full(85, 0.3)]
    _, kr_a, _, _ = inference.hmc(target, cfg, step, init, "CP", flags=f)
    assert kr_a.trace is not None and tuple(kr_a.trace.shape) == (400, 96, sp.D) and kr_a.moments is None
    x = kr_a.trace.cpu().numpy()
    # whole trace -> split R-hat
    got = diagnostics.rhat_from_sums(diagnostics.fold(*diagnostics.split_moments(kr_a.trace, True)), 200)
    want = rhat_ref.rhat(x, True)
    _, v64 = rhat_ref.moments(x, True)
    v64 = v64.reshape(-1, sp.D)
    allow = rhat_allowance(x, True, CAP * np.sqrt(v64), CAP * v64)
    print("whole trace: split rhat max %.5f; largest |error| %.3g, allowed there %.3g" % (
        np.nanmax(want[0]), np.abs(got.rhat - want[0]).max(), allow[0][np.abs(got.rhat - want[0]).argmax()]))
    assert (np.abs(got.rhat - want[0]) <= allow[0]).all()
    assert (np.abs(got.mean - want[1]) <= allow[1]).all() and (np.abs(got.sd - want[2]) <= allow[2]).all()
    # streaming -> un-split R-hat of all chains from the statistics planes
    f2 = f.copy(); f2.trace_chunk_rows = 96; f2.ess_chains = 70; f2.num_chains_to_save = 5
    _, kr_b, _, _ = inference.hmc(target, cfg, step, init, "CP", flags=f2)
    assert kr_b.moments is not None and tuple(kr_b.trace.shape) == (400, 70, sp.D) and kr_b.ess_info.chains == 70
    assert np.array_equal(kr_b.trace.cpu().numpy(), x[:, :70])
    got = diagnostics.rhat_from_sums(diagnostics.from_stats(*kr_b.moments), 400)
    want = rhat_ref.rhat(x, False)
    m64, v64 = (a[0] for a in rhat_ref.moments(x, False))
    scale = np.abs(x).max(axis=0).astype(np.float64) + 1
    allow = rhat_allowance(x, False, 2e-6 * scale + 2.0 ** -24 * np.abs(m64), 2e-6 * scale * scale + 2.0 ** -24 * v64)
    print("streaming: rhat max %.5f; largest |error| %.3g, allowed there %.3g; bound on W / W at most %.3g" % (
        np.nanmax(want[0]), np.abs(got.rhat - want[0]).max(), allow[0][np.abs(got.rhat - want[0]).argmax()], allow[3].max()))
    assert allow[3].max() < 0.10
    assert (np.abs(got.rhat - want[0]) <= allow[0]).all()
    assert (np.abs(got.mean - want[1]) <= allow[1]).all() and (np.abs(got.sd - want[2]) <= allow[2]).all()
    assert np.array_equal(got.rows, np.full(sp.D, 96))
    # and the kept chains' split R-hat is that of the same chains of the whole trace, bit for bit (same kernel, same rows)
    import torch
    a = diagnostics.split_moments(kr_a.trace[:, :70], True)
    b = diagnostics.split_moments(kr_b.trace[:, :70], True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _run(args, out=None):
    from autoreparam_amd import flags as flags_mod
    from autoreparam_amd import main as cli
    return cli.main(args, flags=flags_mod.FlagValues(), out=out)


CHAINS, SAMPLES = 64, 400


@pytest.fixture(scope="module")
def cli_run(gpu, tmp_path_factory):
    """8 schools (non-centred: it mixes) through the CLI: VI, one tuning run, then the sampling run with and (in a copy of the directory made
    before it) without the diagnostics; every chain's trace saved."""
    d = str(tmp_path_factory.mktemp("rhat_cli"))
    on, off = os.path.join(d, "on"), os.path.join(d, "off")
    common = ["--model=8schools", "--method=NCP", "--num_chains=%d" % CHAINS, "--seed=4"]
    hm = ["--num_samples=%d" % SAMPLES, "--num_burnin_steps=600", "--num_adaptation_steps=400"]
    _run(common + ["--results_dir=" + on, "--inference=VI", "--num_optimization_steps=600"])
    _run(common + ["--results_dir=" + on, "--inference=HMCtuning", "--num_leapfrog_steps=4"] + hm)
    shutil.copytree(on, off)
    _run(common + ["--results_dir=" + on, "--inference=HMC", "--num_chains_to_save=%d" % CHAINS] + hm)
    _run(common + ["--results_dir=" + off, "--inference=HMC", "--num_chains_to_save=%d" % CHAINS,
                   "--noconvergence_diagnostics"] + hm)
    return on, off


def _packed_trace(d):
    from autoreparam_amd import models
    sp = models.get_model_by_name("8schools", "").model
    tr = np.load(os.path.join(d, "NCP_tied_traces.npz"))
    return sp, np.concatenate([tr[n].reshape(SAMPLES, CHAINS, -1) for n in sp.part_names], axis=2)


def test_cli_end_to_end(cli_run):
    """split_rhat_max and every array of _rhat.npz against the reference evaluated on _traces.npz (all chains saved);
    allowed: what the moments' own tolerance (CAP) implies through the formulas (rhat_allowance)."""
    on, off = cli_run
    r = json.load(open(os.path.join(on, "NCP_tied.json")))
    r_off = json.load(open(os.path.join(off, "NCP_tied.json")))
    for k in NEW_KEYS:
        assert isinstance(r[k], list) and len(r[k]) == 1 == len(r["ess_min"]), k
        assert k not in r["tuning_runs"][0] and k not in r_off
    assert set(r["tuning_runs"][0]) == {"num_leapfrog_steps", "ess_min", "sem_min", "acceptance_rate", "mcmc_time",
                                        "num_samples", "num_burnin_steps"}
    # without the diagnostics: exactly the keys the CLI wrote before they existed
    assert set(r_off) == {"elbo", "variational_fit_time_secs", "actual_num_variational_steps", "estimated_elbo_std",
                          "learning_rate", "initial_step_size", "learned_reparam", "learned_variational_params",
                          "tuning_runs", "ess_min", "sem_min", "acceptance_rate", "mcmc_time_sec", "ess_estimator",
                          "ess_min_batch_means", "sem_min_batch_means", "batch_means_batch", "ess_constant_chains",
                          "ess_chains"}
    assert set(r) == set(r_off) | set(NEW_KEYS)
    assert not os.path.exists(os.path.join(off, "NCP_tied_rhat.npz"))
    assert r["split_rhat_chains"] == [CHAINS] and r["rhat_max_all_chains"] == [None]
    assert 0 < r["diagnostics_time_sec"][0] < 60
    sp, x = _packed_trace(on)
    want = rhat_ref.rhat(x, True)
    v64 = rhat_ref.moments(x, True)[1].reshape(-1, sp.D)
    allow = rhat_allowance(x, True, CAP * np.sqrt(v64), CAP * v64)
    z = np.load(os.path.join(on, "NCP_tied_rhat.npz"))
    assert sorted(z.files) == sorted("%s/%s" % (k, n) for k in ("split_rhat", "posterior_mean", "posterior_sd")
                                     for n in sp.part_names)
    for key, ref, tol in (("split_rhat", want[0], allow[0]), ("posterior_mean", want[1], allow[1]),
                          ("posterior_sd", want[2], allow[2])):
        parts = [z["%s/%s" % (key, n)] for n in sp.part_names]
        assert [p.shape for p in parts] == [tuple(s) for s in sp.part_shapes]
        got = np.concatenate([p.reshape(-1) for p in parts])
        print("%s: largest |error| %.3g (allowed there %.3g)" % (key, np.abs(got - ref).max(), tol[np.abs(got - ref).argmax()]))
        assert (np.abs(got - ref) <= tol).all(), key
    at = int(np.argmax(want[0]))
    assert abs(r["split_rhat_max"][0] - want[0][at]) <= allow[0][at]
    assert r["split_rhat_max"][0] > np.sqrt((SAMPLES // 2 - 1.0) / (SAMPLES // 2)) - 1e-3       # rhat^2 >= (n - 1) / n


def test_sees_what_ess_cannot(gpu, cli_run):
    """A quarter of the chains sit 2 pooled sd away in one element: the maximum moves to that element, with the value the
    reference gives, while arp_ess of those very series is unchanged to its own test tolerance (rtol 1e-3,
    tests/test_gpu_edges.py) -- a shift does not touch autocorrelations."""
    import torch
    from autoreparam_amd import diagnostics, util
    sp, x = _packed_trace(cli_run[0])
    e = 0
    sd = rhat_ref.rhat(x, True)[2][e]
    y = x.copy()
    y[:, : CHAINS // 4, e] += np.float32(2 * sd)
    xd, yd = torch.as_tensor(x, device=gpu), torch.as_tensor(y, device=gpu)
    got = diagnostics.rhat_from_sums(diagnostics.fold(*diagnostics.split_moments(yd, True)), SAMPLES // 2)
    want = rhat_ref.rhat(y, True)
    v64 = rhat_ref.moments(y, True)[1].reshape(-1, sp.D)
    allow = rhat_allowance(y, True, CAP * np.sqrt(v64), CAP * v64)
    print("shifted element %d: rhat %.4f (reference %.4f), before the shift %.4f" % (e, got.rhat[e], want[0][e],
                                                                                    rhat_ref.rhat(x, True)[0][e]))
    assert int(np.nanargmax(got.rhat)) == e == int(np.nanargmax(want[0])) and got.rhat[e] > 1.2
    assert (np.abs(got.rhat - want[0]) <= allow[0]).all()
    ess_x, ess_y = util.effective_sample_size(xd).cpu().numpy(), util.effective_sample_size(yd).cpu().numpy()
    np.testing.assert_allclose(ess_y, ess_x, rtol=1e-3)
