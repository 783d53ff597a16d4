"""Nested R-hat on the device (arp_moments_fold_nested, arp_nested_step_sums, diagnostics.nested_*, --superchain_size)
against the float64 yardstick tests/nested_rhat_ref.py.

Tolerances.  The kernels take float32 inputs (exact in float64) and work in float64 throughout, so the sums are held to
multiples of 2^-52, not to a float32 figure.  With A = the largest |value| of the column and per superchain g, b, w:
  counts (rows 0 and 5)  exact
  sum g, sum w           a mean of M terms and a sum of K of them: (M + K) 2^-52 sum |g|
  sum g^2                twice the relative error of g: 2 (M + K) 2^-52 sum g^2
  sum b                  M2 of a lane is s2 - s1^2 / n about one of its own draws, at most ~ 5 sd from the mean, so
                         s2 <= 26 M2, summed over at most M terms: 13 M 2^-52 b, allowed 16 M; the pairwise merges subtract
                         means known to 2^-53 A each, over at most 10 levels: 2 sqrt(b) 10 2^-53 A, allowed 16 A sqrt(b)
The statistic: the bound of nested.hip, 2^-52 K gbar^2 / ((K - 1) B) on B, allowed 8 x, plus the sums' own share.
"""
import ctypes as C
import functools
import json
import os
import shutil

import numpy as np
import pytest

import nested_rhat_ref as ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def make_trace(S, Cn, M, D, seed):
    """float32 [S, Cn, D]: noise about superchain offsets of sd 0.5; columns at 100 sd, at scale 1e-3 and (D >= 4) one that
    is constant inside every chain."""
    rs = np.random.RandomState(seed)
    x = rs.randn(S, Cn, D) + np.repeat(0.5 * rs.randn(Cn // M, D), M, axis=0)[None]
    x[:, :, 0] += 100.0
    if D >= 3:
        x[:, :, 2] *= 1e-3
    if D >= 4:
        x[:, :, 3] = x[0, :, 3]
    return x.astype(np.float32)


def allowances(mean, var, M):
    """[5, ...] absolute allowances for rows 1 - 4 of the sums (and a zero row 0) of per-chain moments [C, ...]."""
    ok, g, b, w = ref.groups(mean, var, M)
    K = ok.shape[0]
    z = lambda a: np.where(ok, a, 0.0).sum(axis=0)
    A = np.where(np.isfinite(mean), np.abs(mean), 0.0).max(axis=0)
    with np.errstate(invalid="ignore"):
        return np.stack([np.zeros_like(A), (M + K) * EPS * z(np.abs(g)), 2 * (M + K) * EPS * z(g * g),
                         EPS * (16 * M * z(b) + 16 * A * z(np.sqrt(b))), (M + K) * EPS * z(np.abs(w))])


def check_sums(got, want, allow, label):
    assert got.shape == want.shape, label
    assert np.array_equal(got[0], want[0]), (label, "count")
    worst = 0.0
    for i, name in ((1, "sum g"), (2, "sum g^2"), (3, "sum b"), (4, "sum w"))[:4 if want.shape[0] == 6 else 3]:
        err = np.abs(got[i] - want[i])
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(allow[i] > 0, err / allow[i], 0.0))))
        assert (err <= allow[i]).all(), (label, name, float(err.max()), float(allow[i].min()))
    if want.shape[0] == 6:
        assert np.array_equal(got[5], want[5]), (label, "left out")
    print("%s: largest error %.3f of its allowance" % (label, worst))


def statistic_allowance(want, K):
    """Relative, on nested R-hat - and on B / W: the raw-sums bound on B, and 1e-12 for everything else."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return 8.0 * EPS * K * want["gbar"] ** 2 / ((K - 1) * want["B"]) + 1e-12


# ---- the fold

FOLD_SHAPES = [(4, 2, 1), (6, 3, 3), (2 * 513, 513, 2), (2050, 2, 71), (192, 64, 129)]


@functools.lru_cache(maxsize=None)
def fold_case(shape):
    rows, M, D = shape
    x = make_trace(6, rows, M, D, seed=rows + D)
    mean, var = ref.chain_moments(x)
    mean, var = mean.astype(np.float32), var.astype(np.float32)
    for a in (mean, var):
        a.setflags(write=False)
    return mean, var


def run_fold(gpu, mean, var, M):
    import torch
    from autoreparam_amd import diagnostics
    m = torch.as_tensor(np.array(mean), device=gpu)
    v = None if var is None else torch.as_tensor(np.array(var), device=gpu)
    out = diagnostics.nested_fold(m, v, M)
    assert out.shape == (6, mean.shape[-1]) and out.dtype == torch.float64 and out.is_cuda
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", FOLD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fold_against_the_yardstick(gpu, shape):
    from autoreparam_amd import diagnostics
    rows, M, D = shape
    mean, var = fold_case(shape)
    got = run_fold(gpu, mean, var, M)
    check_sums(got, ref.sums(mean, var, M), allowances(mean, var, M), "fold %s" % (shape,))
    assert run_fold(gpu, mean, var, M).tobytes() == got.tobytes()                    # repeatable
    # one draw per chain
    one = run_fold(gpu, mean, None, M)
    check_sums(one, ref.sums(mean, None, M), allowances(mean, None, M), "fold %s, var=None" % (shape,))
    assert (one[4] == 0).all()
    # the statistic
    want = ref.from_moments(mean, var, M)
    res = diagnostics.nested_rhat_from_sums(got)
    K = rows // M
    ok, g, _, _ = ref.groups(mean, var, M)
    tol = statistic_allowance({"gbar": g.mean(axis=0), "B": want.between}, K)
    if K >= 2:
        assert (np.abs(res.rhat / want.rhat - 1.0) <= tol).all(), (shape, res.rhat, want.rhat)
        assert (np.abs(res.excess / want.excess - 1.0) <= tol).all()
    else:
        assert np.isnan(res.rhat).all()


def test_fold_leaves_out_whole_superchains_and_counts_them(gpu):
    shape = (192, 64, 129)
    rows, M, D = shape
    mean, var = (np.array(a) for a in fold_case(shape))
    clean = run_fold(gpu, mean, var, M)
    var[3, 5] = np.nan                       # superchain 0, column 5
    var[64 + 63, 5] = np.inf                 # superchain 1, column 5 (its last row)
    var[130, 7] = -np.inf                    # superchain 2, column 7
    mean[0, 128] = np.nan                    # superchain 0, the last column
    var[70, 9] = 0.0                         # a chain that never moved counts
    var[64:128, 11] = 0.0                    # a superchain of them too
    got = run_fold(gpu, mean, var, M)
    check_sums(got, ref.sums(mean, var, M), allowances(mean, var, M), "fold with non-finite rows")
    assert got[0, 5] == 1 and got[5, 5] == 2 and got[0, 7] == 2 and got[5, 7] == 1 and got[0, 128] == 2 and got[5, 128] == 1
    assert got[0, 9] == 3 and got[0, 11] == 3
    untouched = [d for d in range(D) if d not in (5, 7, 9, 11, 128)]
    assert got[:, untouched].tobytes() == clean[:, untouched].tobytes()
    # a left-out superchain is as if it were not there: the other two, alone
    alone = run_fold(gpu, mean[64:], var[64:], M)
    assert np.array_equal(alone[:5, 128], got[:5, 128])
    # var = None tests the means only
    one = run_fold(gpu, mean, None, M)
    assert one[0, 5] == 3 and one[0, 128] == 2 and one[5, 128] == 1


def test_fold_of_no_rows_is_zero(gpu):
    import torch
    from autoreparam_amd import diagnostics
    none = torch.empty(0, 5, device=gpu)
    assert (diagnostics.nested_fold(none, none, 4).cpu().numpy() == 0).all()


# ---- the step kernel

STEP_SHAPES = [(1, 4, 2, 1), (3, 12, 3, 5), (2, 130, 65, 71), (2, 1024, 2, 129), (2, 2048, 1024, 3), (5, 64, 8, 300)]


@functools.lru_cache(maxsize=None)
def step_case(shape):
    S, Cn, M, D = shape
    x = make_trace(S, Cn, M, D, seed=Cn + D)
    x.setflags(write=False)
    return x


def step_allowances(x, M):
    return np.stack([allowances(row.astype(np.float64), None, M)[:4] for row in x], axis=1)


def run_step(gpu, x, M):
    import torch
    from autoreparam_amd import diagnostics
    xd = x if torch.is_tensor(x) else torch.as_tensor(np.array(x), device=gpu)
    out = diagnostics.nested_step_sums(xd, M)
    assert out.shape == (4, xd.shape[0], xd.shape[2]) and out.dtype == torch.float64 and out.is_cuda
    return out.cpu().numpy()


def check_profile(got, x, M, label):
    from autoreparam_amd import diagnostics
    K = x.shape[1] // M
    res = diagnostics.nested_rhat_by_step(got)
    want = ref.by_step(x, M)
    assert res.shape == want.shape
    if K < 2:
        assert np.isnan(res).all()
        return
    for s in range(x.shape[0]):
        ok, g, b, _ = ref.groups(x[s].astype(np.float64), None, M)
        k = ok.sum(axis=0)
        with np.errstate(all="ignore"):
            gbar = np.where(ok, g, 0.0).sum(axis=0) / k
            B = np.where(ok, (g - gbar) ** 2, 0.0).sum(axis=0) / (k - 1)
        tol = statistic_allowance({"gbar": gbar, "B": B}, K)
        both = np.isfinite(want[s])
        assert np.array_equal(np.isfinite(res[s]), both), (label, s)
        assert (np.abs(res[s][both] / want[s][both] - 1.0) <= tol[both]).all(), (label, s)


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_sums_against_the_yardstick(gpu, shape):
    S, Cn, M, D = shape
    x = step_case(shape)
    got = run_step(gpu, x, M)
    check_sums(got, ref.step_sums(x, M), step_allowances(x, M), "step %s" % (shape,))
    assert (got[0] == Cn // M).all()
    check_profile(got, x, M, shape)
    assert run_step(gpu, x, M).tobytes() == got.tobytes()                            # repeatable


def test_step_sums_cut_over_workgroups(gpu):
    """One row of many superchains is cut over workgroups whose sums a second launch adds (the workspace route)."""
    from autoreparam_amd import diagnostics
    shape = (2, 8192, 4, 33)
    S, Cn, M, D = shape
    assert diagnostics.nested_step_workspace_bytes(S, Cn, D, M) > 0
    assert diagnostics.nested_step_workspace_bytes(*STEP_SHAPES[1][:2], STEP_SHAPES[1][3], STEP_SHAPES[1][2]) == 0
    x = step_case(shape)
    got = run_step(gpu, x, M)
    check_sums(got, ref.step_sums(x, M), step_allowances(x, M), "step %s" % (shape,))
    check_profile(got, x, M, shape)
    assert run_step(gpu, x, M).tobytes() == got.tobytes()


def test_step_sums_of_an_inner_block_of_chains(gpu):
    import torch
    shape = (3, 12, 3, 5)
    M = shape[2]
    wide = make_trace(3, 12 + 11, 1, 5, seed=3)
    wide[:, 5:17] = step_case(shape)
    wd = torch.as_tensor(wide, device=gpu)
    view = wd[:, 5:17]
    assert not view.is_contiguous()
    a = run_step(gpu, view, M)
    assert a.tobytes() == run_step(gpu, view.contiguous(), M).tobytes() == run_step(gpu, step_case(shape), M).tobytes()
    lead = run_step(gpu, wd[:, :21], M)                       # a leading block: 7 superchains of other values
    check_sums(lead, ref.step_sums(wide[:, :21], M), step_allowances(wide[:, :21], M), "leading block")


def test_step_sums_drop_only_the_cell_with_a_non_finite_draw(gpu):
    shape = (5, 64, 8, 300)
    S, Cn, M, D = shape
    x = np.array(step_case(shape))
    clean = run_step(gpu, x, M)
    x[1, 2 * M + 3, 7] = np.nan
    x[4, 7 * M + 7, 299] = np.inf
    x[0, 0, 0] = -np.inf
    got = run_step(gpu, x, M)
    check_sums(got, ref.step_sums(x, M), step_allowances(x, M), "step with non-finite draws")
    hit = np.zeros((S, D), bool)
    hit[1, 7] = hit[4, 299] = hit[0, 0] = True
    assert (got[0][hit] == Cn // M - 1).all() and (got[0][~hit] == Cn // M).all()
    assert got[:, ~hit].tobytes() == clean[:, ~hit].tobytes()
    assert np.isfinite(got).all()
    check_profile(got, x, M, "non-finite draws")


# ---- arguments

def test_argument_errors_launch_nothing(gpu):
    import torch
    from autoreparam_amd import _lib, diagnostics
    L = _lib.lib()
    S, Cn, M, D = 3, 12, 3, 5
    x = torch.zeros(S, Cn, D, device=gpu)
    mean = torch.zeros(Cn, D, device=gpu)
    sums4 = torch.full((4, S, D), 7.0, dtype=torch.float64, device=gpu)
    sums6 = torch.full((6, D), 7.0, dtype=torch.float64, device=gpu)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)

    def step(trace=p(x), c=Cn, m=M, out=p(sums4), stride=Cn * D):
        return L.arp_nested_step_sums(trace, S, c, D, stride, m, out, null, 0, st)

    def fold(mu=p(mean), rows=Cn, m=M, out=p(sums6)):
        return L.arp_moments_fold_nested(mu, null, rows, D, m, out, st)

    for what, call, word in (("trace", lambda: step(trace=null), "trace and sums"), ("sums", lambda: step(out=null), "trace and sums"),
                             ("M = 1", lambda: step(m=1), "M >= 2"), ("M = 0", lambda: step(m=0), "M >= 2"),
                             ("C % M", lambda: step(m=5), "divides n_chains"), ("stride", lambda: step(stride=Cn * D - 1), "row_stride")):
        rc = call()
        msg = L.arp_last_error().decode()
        print("%s -> %d: %s" % (what, rc, msg))
        assert rc == 1 and "arp_nested_step_sums" in msg and word in msg
    for what, call, word in (("mean", lambda: fold(mu=null), "mean"), ("sums", lambda: fold(out=null), "sums"),
                             ("M = 1", lambda: fold(m=1), "M >= 2"), ("rows % M", lambda: fold(rows=Cn - 1), "divides n_rows")):
        rc = call()
        msg = L.arp_last_error().decode()
        print("%s -> %d: %s" % (what, rc, msg))
        assert rc == 1 and "arp_moments_fold_nested" in msg and word in msg
    # a row cut over workgroups needs its workspace
    big = (2, 8192, 33, 4)
    need = int(L.arp_nested_step_workspace_bytes(*big))
    assert need > 0 and need % 256 == 0 and int(L.arp_nested_step_workspace_bytes(2, 8192, 33, 3)) == 0
    xb = torch.zeros(2, 8192, 33, device=gpu)
    sb = torch.full((4, 2, 33), 7.0, dtype=torch.float64, device=gpu)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=gpu)
    for what, args in (("too small", (p(ws), need - 1)), ("too small", (null, need)), ("aligned", (C.c_void_p(ws.data_ptr() + 8), need))):
        rc = L.arp_nested_step_sums(p(xb), 2, 8192, 33, 8192 * 33, 4, p(sb), args[0], args[1], st)
        msg = L.arp_last_error().decode()
        assert rc == 1 and "arp_nested_step_sums" in msg and what in msg, msg
    # the Python layer: a CPU tensor, a size that does not divide
    with pytest.raises(ValueError, match="on the GPU"):
        diagnostics.nested_step_sums(torch.zeros(S, Cn, D), M)
    with pytest.raises(ValueError, match="on the GPU"):
        diagnostics.nested_fold(torch.zeros(Cn, D), None, M)
    with pytest.raises(RuntimeError, match="divides n_rows"):
        diagnostics.nested_fold(mean, mean, 5)
    with pytest.raises(RuntimeError, match="divides n_chains"):
        diagnostics.nested_step_sums(x, 5)
    torch.cuda.synchronize()
    for t in (sums4, sums6, sb):
        assert (t.cpu().numpy() == 7.0).all()                  # nothing was launched
    assert step() == 0 and fold() == 0
    torch.cuda.synchronize()
    assert (sums4.cpu().numpy()[0] == Cn // M).all() and (sums6.cpu().numpy()[0] == Cn // M).all()


# ---- the command line

CHAINS, SAMPLES, SIZE = 64, 400, 8
KEYS = ("nested_rhat_max", "nested_rhat_superchains", "nested_rhat_superchain_size", "nested_rhat_chains", "nested_rhat_floor",
        "nested_rhat_left_out", "nested_rhat_first_step_max", "nested_rhat_last_step_max", "nested_rhat_time_sec")


def _cli(args):
    from autoreparam_amd import flags as flags_mod
    from autoreparam_amd import main as cli
    return cli.main(args, flags=flags_mod.FlagValues())


@pytest.fixture(scope="module")
def cli_run(gpu, tmp_path_factory):
    """The small run of test_gpu_mcess.py (8 schools, non-centred, 64 chains of 400 samples, every trace saved): the
    sampling run with --superchain_size=8 and, in a copy of the directory made before it, without."""
    d = str(tmp_path_factory.mktemp("nested_cli"))
    on, off = os.path.join(d, "on"), os.path.join(d, "off")
    common = ["--model=8schools", "--method=NCP", "--num_chains=%d" % CHAINS, "--seed=4"]
    hm = ["--num_samples=%d" % SAMPLES, "--num_burnin_steps=600", "--num_adaptation_steps=400"]
    _cli(common + ["--results_dir=" + on, "--inference=VI", "--num_optimization_steps=600"])
    _cli(common + ["--results_dir=" + on, "--inference=HMCtuning", "--num_leapfrog_steps=4"] + hm)
    shutil.copytree(on, off)
    sample = ["--inference=HMC", "--num_chains_to_save=%d" % CHAINS] + hm
    _cli(common + ["--results_dir=" + on, "--superchain_size=%d" % SIZE] + sample)
    _cli(common + ["--results_dir=" + off] + sample)
    return on, off


def test_cli_end_to_end(gpu, cli_run):
    import torch
    from autoreparam_amd import analyze, diagnostics, models
    on, off = cli_run
    r = json.load(open(os.path.join(on, "NCP_tied.json")))
    r_off = json.load(open(os.path.join(off, "NCP_tied.json")))
    assert set(r) == set(r_off) | set(KEYS) and not set(KEYS) & set(r_off)
    for k in KEYS:
        assert isinstance(r[k], list) and len(r[k]) == 1 and k not in r["tuning_runs"][0], k
    assert r["nested_rhat_superchains"] == [CHAINS // SIZE] == [8] and r["nested_rhat_superchain_size"] == [SIZE]
    assert r["nested_rhat_chains"] == [CHAINS] and r["nested_rhat_left_out"] == [0]
    assert r["nested_rhat_floor"] == [float(np.sqrt(1.0 + 1.0 / SIZE))]
    assert 0 < r["nested_rhat_time_sec"][0] < 60
    sp = models.get_model_by_name("8schools", "").model
    z, z_off = np.load(os.path.join(on, "NCP_tied_rhat.npz")), np.load(os.path.join(off, "NCP_tied_rhat.npz"))
    new = ["nested_rhat/%s" % n for n in sp.part_names] + ["nested_rhat_by_step", "nested_rhat_by_step_element"]
    assert sorted(z.files) == sorted(z_off.files + new)
    tr = np.load(os.path.join(on, "NCP_tied_traces.npz"))
    x = np.concatenate([tr[n].reshape(SAMPLES, CHAINS, -1) for n in sp.part_names], axis=2).astype(np.float32)
    # the chains of a superchain started from one point and then parted ways
    assert all(np.unique(x[-1, k * SIZE:(k + 1) * SIZE, 0]).size > 1 for k in range(CHAINS // SIZE))
    xd = torch.as_tensor(x, device=gpu)
    mean, var = diagnostics.split_moments(xd, split=False)
    want = diagnostics.nested_rhat_from_sums(diagnostics.nested_fold(mean[0], var[0], SIZE))
    parts = [z["nested_rhat/%s" % n] for n in sp.part_names]
    assert [p.shape for p in parts] == [tuple(s) for s in sp.part_shapes]
    assert np.array_equal(np.concatenate([p.reshape(-1) for p in parts]), want.rhat, equal_nan=True)
    assert r["nested_rhat_max"][0] == np.nanmax(want.rhat)
    steps = diagnostics.nested_rhat_by_step(diagnostics.nested_step_sums(xd, SIZE))
    assert z["nested_rhat_by_step"].shape == (SAMPLES,) and z["nested_rhat_by_step_element"].shape == (SAMPLES,)
    assert np.array_equal(z["nested_rhat_by_step"], steps.max(axis=1))
    assert np.array_equal(z["nested_rhat_by_step_element"], steps.argmax(axis=1))
    assert r["nested_rhat_first_step_max"][0] == steps[0].max() and r["nested_rhat_last_step_max"][0] == steps[-1].max()
    # the yardstick on the same traces
    ref_all = ref.nested(x, SIZE)
    assert np.allclose(want.rhat, ref_all.rhat, rtol=1e-5)             # (the moments are float32: test_gpu_rhat.py holds them)
    assert np.allclose(steps, ref.by_step(x, SIZE), rtol=1e-9)
    lines = analyze.report_rhat({"NCP_tied": r}, on, "")
    assert sum("nested R-hat" in line for line in lines) == 1
    assert not any("nested" in line for line in analyze.report_rhat({"NCP_tied": r_off}, off, ""))
