"""GPU: the posterior geometry report -- arp_gram_sums (csrc/gram.hip: the cross moments of a trace on
v_mfma_f32_32x32x2_f32), diagnostics.gram_sums / geometry_from_sums / scale_coupling / coupling_from_sums and
--geometry_diagnostics -- against the float64 yardstick of tests/geometry_ref.py: exact on integer data, within twice the
header's bound on normal data, rows left out, reproducibility, refusals, the funnel, and the CLI end to end.

Measured on an MI355X (largest deviation / allowance of the parity test): DESIGN.md section 6."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

import geometry_ref as gr
import helpers

pytestmark = pytest.mark.gpu

DS = (1, 2, 31, 32, 33, 64, 71, 125, 250, 512)


def _W():
    from autoreparam_amd import diagnostics
    assert diagnostics.GRAM_WINDOW == gr.W and diagnostics.GRAM_WINDOW <= 256
    return diagnostics.GRAM_WINDOW


def _row_counts(W):
    # ..., and 2 W + 37: three workgroups (one window each) with a ragged last tile at every tile height (16, 32, 64)
    return (1, 2, 3, W - 1, W, W + 1, 3 * W + 5, 2 * W + 37)


def _sums(gpu, x, shift=None):
    from autoreparam_amd import diagnostics
    xd = torch.as_tensor(np.ascontiguousarray(x, np.float32), device=gpu)
    sd = None if shift is None else torch.as_tensor(np.ascontiguousarray(shift, np.float32), device=gpu)
    return diagnostics.gram_sums(xd, sd).cpu().numpy()


def _normal(rows, D, seed):
    """(x, shift): columns N(1000, 1) as float32, and a shift within one sd of every column's mean."""
    rs = np.random.RandomState(seed)
    x = (1000.0 + rs.randn(rows, D)).astype(np.float32)
    shift = (1000.0 + rs.uniform(-1.0, 1.0, D)).astype(np.float32)
    return x, shift


def _check_within(got, x, shift, what):
    """got against gram_ref(x, shift): G within gram_allowance (twice the header's bound), row D within 1e-12 of the sum
    of |u| (a float64 sum of n terms in any order is good to n 2^-53 of that; n <= 2^13 here), the counts exactly.
    Returns the largest deviation / allowance of G."""
    ref, allow = gr.gram_ref(x, shift), gr.gram_allowance(x, shift)
    D = ref.shape[1]
    assert np.isfinite(got).all(), what
    dev = np.abs(got[:D] - ref[:D])
    assert (dev <= allow).all(), (what, float((dev - allow).max()))
    u, keep = gr.u_rows(x, shift)
    abs_sum = np.abs(u[keep].astype(np.float64)).sum(axis=0)
    assert (np.abs(got[D] - ref[D]) <= 1e-12 * abs_sum).all(), what
    assert np.array_equal(got[D + 1], ref[D + 1]), what
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(allow > 0, dev / allow, 0.0)
    return float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------------------
# 1. exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", DS)
def test_integer_data_is_exact(gpu, D):
    """Integers in [-64, 64] as float32, NULL shift: every product is at most 2^12 and every window sum at most 2^20, so
    all float32 arithmetic is exact and `sums` must EQUAL the integer reference (formed in float64, where sums below 2^53
    are exact) -- no tolerance, so any layout, padding or tail error shows.  G is asymmetric in its inputs (random columns),
    which also catches a swapped row / column map of the accumulator."""
    W = _W()
    rs = np.random.RandomState(D)
    for rows in _row_counts(W):
        x = rs.randint(-64, 65, size=(rows, D)).astype(np.float32)
        got = _sums(gpu, x)
        assert np.array_equal(got, gr.gram_ref(x)), (D, rows)


@pytest.mark.parametrize("D,rows", [(33, 2 * 1024 * 256 + 300), (512, 2 * 113 * 256 + 300)])
def test_integer_data_is_exact_with_chunks_of_several_windows(gpu, D, rows):
    """More windows than the grid has workgroups for, so a workgroup's chunk holds several windows (three here) and its
    float64 registers are added into more than once; the last chunk is short and its last tile ragged."""
    rs = np.random.RandomState(D)
    x = rs.randint(-64, 65, size=(rows, D)).astype(np.float32)
    assert np.array_equal(_sums(gpu, x), gr.gram_ref(x))


# ---------------------------------------------------------------------------
# 2. parity within the bound
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", (1, 33, 71, 125, 250, 512))
def test_normal_data_within_twice_the_bound(gpu, D):
    """Columns N(1000, 1), a shift within one sd of the mean: G within 2 (W + 1) 2^-24 sum |u_i u_j| per entry (twice the
    header's bound; the doubling covers its second-order terms), row D to 1e-12 relative, the counts exact.  The same data
    with a NULL shift within its own, much larger allowance (u = x ~ 1000), and bitwise the result of explicit zeros."""
    W = _W()
    worst = 0.0
    for rows in (3, W + 1, 3 * W + 5, 2 * W + 37):
        x, shift = _normal(rows, D, 100 * D + rows)
        worst = max(worst, _check_within(_sums(gpu, x, shift), x, shift, (D, rows, "shift")))
        plain = _sums(gpu, x)
        _check_within(plain, x, None, (D, rows, "null shift"))
        assert np.array_equal(plain, _sums(gpu, x, np.zeros(D, np.float32))), (D, rows)
    print("gram sums D=%d: largest deviation / allowance %.4f" % (D, worst))


# ---------------------------------------------------------------------------
# 3. rows left out
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", (1, 33, 71, 250, 512))
def test_rows_with_a_non_finite_element_are_left_out(gpu, D):
    """NaN, +inf and -inf planted in the first and the last column, in the first and the last row, and in a column of every
    32-block: the counts are exact, G and row D are those of the remaining rows (test 2's allowance), and no entry of
    `sums` is non-finite.  Then every row spoiled: zeros and a count of 0."""
    W = _W()
    rows = 3 * W + 5
    x, shift = _normal(rows, D, 7 * D)
    bad = [np.nan, np.inf, -np.inf]
    plant = [(0, 0), (rows - 1, D - 1), (1, D - 1), (rows - 2, 0), (W - 1, 0), (W, D - 1), (W + 1, D // 2)]
    plant += [(17 + 31 * b, min(32 * b + 5, D - 1)) for b in range((D + 31) // 32)]
    for i, (r, d) in enumerate(plant):
        x[r, d] = bad[i % 3]
    n_bad = len({r for r, _ in plant})
    got = _sums(gpu, x, shift)
    assert got[D + 1, 0] == rows - n_bad
    if D > 1:
        assert got[D + 1, 1] == n_bad
    _check_within(got, x, shift, (D, "planted"))
    x[:, D - 1] = np.nan
    x[::2, D - 1] = np.inf
    got = _sums(gpu, x, shift)
    want = np.zeros((D + 2, D))
    if D > 1:
        want[D + 1, 1] = rows
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------
# 4. reproducibility
# ---------------------------------------------------------------------------
def test_reproducible_symmetric_and_in_place(gpu):
    """Two calls are bitwise equal; G is bitwise symmetric; a block of chains read in place (row_stride > n_chains * D, at
    a chain offset of 3 * 71 = 213 floats, no multiple of 32) equals its contiguous copy bitwise; the sums of two halves of
    the rows, added, agree with the whole within the allowance."""
    from autoreparam_amd import _lib, diagnostics
    S, K, D, off, cn = 37, 29, 71, 3, 19
    rs = np.random.RandomState(4)
    wide = torch.as_tensor((1000.0 + rs.randn(S, K, D)).astype(np.float32), device=gpu)
    shift = torch.as_tensor((1000.0 + rs.uniform(-1, 1, D)).astype(np.float32), device=gpu)
    block = wide[:, off:off + cn]
    view = _lib.trace_view(block, "test")
    assert view[0].data_ptr() == block.data_ptr() and view[4] == K * D > cn * D and (off * D) % 32 != 0
    a = diagnostics.gram_sums(block, shift)
    b = diagnostics.gram_sums(block, shift)
    c = diagnostics.gram_sums(block.contiguous(), shift)
    d = diagnostics.gram_sums(block.contiguous().reshape(S * cn, D), shift)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    g = a[:D].cpu().numpy()
    assert np.array_equal(g, g.T)
    x = block.contiguous().reshape(S * cn, D).cpu().numpy()
    _check_within(a.cpu().numpy(), x, shift.cpu().numpy(), "block")
    h = (S // 2) * cn
    halves = (diagnostics.gram_sums(block[:S // 2], shift) + diagnostics.gram_sums(block[S // 2:], shift)).cpu().numpy()
    assert h % 256 != 0                                                      # (the halves are cut inside a window)
    _check_within(halves, x, shift.cpu().numpy(), "halves")


# ---------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------
def test_refusals(gpu):
    """Every refusal of the header: rc 1 before any launch, a message that names the function, nothing written."""
    from autoreparam_amd import _lib
    L = _lib.lib()
    S, Cn, D = 6, 5, 7
    x = torch.zeros(S, Cn, D, device=gpu)
    sums = torch.full((D + 2, D), 7.0, dtype=torch.float64, device=gpu)
    need = int(L.arp_gram_workspace_bytes(S, Cn, D))
    assert need > 0 and need % 256 == 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=gpu)
    assert ws.data_ptr() % 256 == 0
    null = C.c_void_p(0)
    good = dict(x=_lib.ptr(x), S=S, Cn=Cn, D=D, stride=Cn * D, sums=_lib.ptr(sums), ws=_lib.ptr(ws), bytes=need)
    bad = [dict(x=null), dict(sums=null), dict(D=0), dict(D=-1), dict(D=513), dict(S=0), dict(S=-2), dict(Cn=0), dict(Cn=-1),
           dict(S=1 << 16, Cn=1 << 15, stride=(1 << 15) * D), dict(stride=Cn * D - 1), dict(ws=null), dict(ws=null, bytes=0),
           dict(bytes=need - 1), dict(bytes=0), dict(ws=C.c_void_p(ws.data_ptr() + 8))]
    with torch.cuda.device(gpu):
        for change in bad:
            k = dict(good, **change)
            rc = L.arp_gram_sums(k["x"], k["S"], k["Cn"], k["D"], k["stride"], null, k["sums"], k["ws"], k["bytes"], _lib.stream())
            assert rc == 1 and b"arp_gram_sums" in L.arp_last_error(), change
        torch.cuda.synchronize()
        assert bool((sums == 7.0).all())
        for S_, Cn_, D_ in ((0, 5, 7), (6, 0, 7), (6, 5, 0), (6, 5, 513), (1 << 16, 1 << 15, 7)):
            assert L.arp_gram_workspace_bytes(S_, Cn_, D_) == 0
        k = good
        assert L.arp_gram_sums(k["x"], k["S"], k["Cn"], k["D"], k["stride"], null, k["sums"], k["ws"], k["bytes"], _lib.stream()) == 0
        torch.cuda.synchronize()
    want = np.zeros((D + 2, D))
    want[D + 1, 0] = S * Cn
    assert np.array_equal(sums.cpu().numpy(), want)


# ---------------------------------------------------------------------------
# 6. the funnel
# ---------------------------------------------------------------------------
N_FUNNEL = 1 << 17


def _draws(kind):
    rs = np.random.RandomState(0)
    if kind == "funnel":
        y = 3.0 * rs.randn(N_FUNNEL)
        x = np.exp(0.5 * y)[:, None] * rs.randn(N_FUNNEL, 9)
        return np.concatenate([y[:, None], x], axis=1).astype(np.float32)
    return rs.randn(N_FUNNEL, 10).astype(np.float32)


def _eigen_allowance(x, ref):
    """What twice the header's bound on G allows the eigenvalues of R to move (Weyl: at most the spectral norm of the
    change of R, itself at most its Frobenius norm).  With a = allowance / ((n - 1) sd_i sd_j), to first order
    |dR_ij| <= a_ij + |R_ij| (a_ii + a_jj) / 2: the entry's own covariance and the two variances it is scaled by."""
    n = x.shape[0]
    a = gr.gram_allowance(x) / ((n - 1.0) * np.outer(ref["sd"], ref["sd"]))
    diag = np.diag(a)
    return float(np.linalg.norm(a + 0.5 * np.abs(ref["correlation"]) * (diag[:, None] + diag[None, :]))) + 1e-12


@pytest.mark.parametrize("kind", ("funnel", "normal"))
def test_the_funnel_is_seen_by_the_coupling_not_by_the_correlation(gpu, kind):
    """2^17 exact draws (numpy.random.RandomState(0), built on the CPU): the funnel y ~ N(0, 3^2), x_j ~ N(0, e^y) has a
    correlation matrix of condition number below 2 while every K[y][x_j] lies in [0.75, 0.85] (theory 0.80); ten
    independent normals give max |K| < 5 / sqrt(N).  Every figure agrees with tests/geometry_ref.py on the same draws: the
    eigenvalues within _eigen_allowance, K within 1e-4."""
    from autoreparam_amd import diagnostics
    x = _draws(kind)
    xd = torch.as_tensor(x, device=gpu)
    g = diagnostics.geometry_from_sums(diagnostics.gram_sums(xd))
    K = diagnostics.coupling_from_sums(diagnostics.scale_coupling(xd, g.mean, g.sd))
    assert g.rows == N_FUNNEL and g.rows_left_out == 0 and len(g.left_out) == 0 and K.shape == (10, 10)
    ref = gr.geometry_ref(x)
    K_ref = gr.coupling_ref(x)
    print("%s: condition number %.4f (ref %.4f); K[0][1:] %s; max |K| %.5f" % (
        kind, g.condition_number, ref["condition_number"], np.round(K[0, 1:], 4), np.abs(K).max()))
    if kind == "funnel":
        assert g.condition_number < 2.0
        assert ((K[0, 1:] >= 0.75) & (K[0, 1:] <= 0.85)).all(), K[0]
    else:
        assert np.abs(K).max() < 5.0 / np.sqrt(N_FUNNEL)
    assert np.abs(g.eigenvalues - ref["eigenvalues"]).max() <= _eigen_allowance(x, ref)
    assert np.abs(K - K_ref).max() <= 1e-4
    assert np.allclose(g.mean, ref["mean"], rtol=0, atol=1e-9 + 1e-6 * ref["sd"].max())
    assert np.allclose(g.sd, ref["sd"], rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------
# 7. end to end
# ---------------------------------------------------------------------------
def _cli(args):
    from autoreparam_amd import flags as flags_mod
    from autoreparam_amd import main as cli
    return cli.main(args, flags=flags_mod.FlagValues())


def test_report_on_a_sampler_run_equals_the_reference(gpu):
    """inference.hmc on 8 schools, NCP, 256 chains, 200 samples; main._geometry_report on it against geometry_ref applied
    to trace.cpu() (centred) and to the engine's own transform of it (the sampler's coordinates), with the run's steps."""
    from autoreparam_amd import flags as flags_mod, graphs, inference, main as cli, models
    cfg = models.get_model_by_name("8schools", "")
    sp = cfg.model
    f = flags_mod.FlagValues()
    f.num_chains, f.num_samples, f.num_burnin_steps, f.num_adaptation_steps, f.num_leapfrog_steps = 256, 200, 200, 150, 4
    f.device = str(gpu)
    target, *_ = graphs.make_ncp_graph(cfg, flags=f)
    rs = np.random.RandomState(0)
    init = [0.1 * rs.randn(256, *s).astype(np.float32) for s in sp.part_shapes]
    step = [np.full(s, 0.3) if len(s) else 0.3 for s in sp.part_shapes]
    _, kr, _, _ = inference.hmc(target, cfg, step, init, "NCP", flags=f)
    assert kr.trace is not None and tuple(kr.trace.shape) == (200, 256, sp.D) and kr.probe is not None
    xc = kr.trace.cpu().numpy().reshape(-1, sp.D)
    keys, arrays = cli._geometry_report(kr, kr.trace, 256, sp, f, None, xc.astype(np.float64).mean(axis=0))
    kn = kr.probe.kernels[0]
    xs = kr.probe.engine.transform(torch.as_tensor(xc, device=gpu), which=kn.which, to_centered=False).cpu().numpy()
    eps0 = kn.eps0.cpu().numpy() if torch.is_tensor(kn.eps0) else np.asarray(kn.eps0)
    ref_c, ref_s = gr.geometry_ref(xc), gr.geometry_ref(xs, eps0)
    K_ref = gr.coupling_ref(xs)
    assert set(keys) == set(cli.GEOMETRY_KEYS) | {"geometry_time_sec"}
    assert keys["geometry_rows"] == 200 * 256 and keys["geometry_rows_left_out"] == 0 and keys["geometry_chains"] == 256
    assert keys["geometry_elements_left_out"] == 0
    print("8 schools NCP: condition number %.4g (ref %.4g), step-scaled %.4g (ref %.4g), centred %.4g (ref %.4g)" % (
        keys["geometry_condition_number"], ref_s["condition_number"], keys["geometry_condition_number_step_scaled"],
        ref_s["step_scaled_condition_number"], keys["geometry_condition_number_centred"], ref_c["condition_number"]))
    # the shift is within a float32 rounding of the mean, so u is O(sd) and the header's bound is ~ 3e-5 of a variance:
    # 1e-3 relative on a condition number leaves room for an ill-conditioned R to amplify it
    assert keys["geometry_condition_number"] == pytest.approx(ref_s["condition_number"], rel=1e-3)
    assert keys["geometry_condition_number_step_scaled"] == pytest.approx(ref_s["step_scaled_condition_number"], rel=1e-3)
    assert keys["geometry_condition_number_centred"] == pytest.approx(ref_c["condition_number"], rel=1e-3)
    assert keys["geometry_max_abs_correlation"] == pytest.approx(ref_s["max_abs_correlation"], abs=1e-4)
    names = cli.element_names(sp)
    assert len(names) == sp.D and keys["geometry_max_correlation_pair"] == [names[i] for i in ref_s["pair"]]
    assert np.abs(arrays["correlation"] - ref_s["correlation"]).max() <= 1e-4
    assert np.abs(arrays["correlation_centred"] - ref_c["correlation"]).max() <= 1e-4
    assert np.abs(arrays["scale_coupling"] - K_ref).max() <= 1e-4
    i, j = np.unravel_index(int(np.abs(K_ref).argmax()), K_ref.shape)
    assert keys["geometry_max_scale_coupling"] == pytest.approx(abs(K_ref[i, j]), abs=1e-4)
    assert keys["geometry_max_scale_coupling_pair"] == [names[i], names[j]]
    assert np.allclose(arrays["mean"], ref_s["mean"], rtol=0, atol=1e-5 * ref_s["sd"].max() + 1e-6 * np.abs(ref_s["mean"]).max())
    assert np.allclose(arrays["sd"], ref_s["sd"], rtol=1e-4, atol=0)
    stiff = np.concatenate([np.asarray(arrays["stiffest_direction/" + n]).reshape(-1) for n in sp.part_names])
    assert abs(np.linalg.norm(stiff) - 1.0) < 1e-9
    # without a chain on the device: every key null
    none, no_arrays = cli._geometry_report(kr, kr.trace, 0, sp, f, None, np.zeros(sp.D))
    assert no_arrays is None and all(none[key] is None for key in cli.GEOMETRY_KEYS)


def test_cli_geometry_diagnostics(gpu, tmp_path):
    """8 schools NCP at 256 chains and 200 samples through main.main with --geometry_diagnostics: the keys and
    <method>_geometry.npz; the same run without the flag, in a copy of the directory made before it: neither.  Then
    --method=i on radon MN at 128 chains and 64 samples: `geometry_by_kernel` with two entries, the `_1` arrays, and
    kernel 0's correlation equal to `correlation_centred` to float rounding (CP's transform is the identity)."""
    from autoreparam_amd import analyze, main as cli
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    common = ["--model=8schools", "--num_chains=256", "--seed=3", "--num_optimization_steps=400"]
    hm = ["--num_samples=200", "--num_burnin_steps=200", "--num_adaptation_steps=150"]
    _cli(common + ["--results_dir=" + on, "--inference=VI", "--method=NCP"])
    _cli(common + ["--results_dir=" + on, "--inference=HMCtuning", "--method=NCP", "--num_leapfrog_steps=4"] + hm)
    shutil.copytree(on, off)
    _cli(common + ["--results_dir=" + on, "--inference=HMC", "--method=NCP", "--geometry_diagnostics"] + hm)
    _cli(common + ["--results_dir=" + off, "--inference=HMC", "--method=NCP"] + hm)
    path = lambda root, suffix: os.path.join(root, "NCP_tied" + suffix)
    r, plain = json.load(open(path(on, ".json"))), json.load(open(path(off, ".json")))
    assert set(r) - set(plain) == set(cli.GEOMETRY_KEYS) | {"geometry_time_sec"} and set(plain) <= set(r)
    assert not any(key.startswith("geometry") for key in plain) and not os.path.exists(path(off, "_geometry.npz"))
    for key in cli.GEOMETRY_KEYS + ("geometry_time_sec",):
        assert len(r[key]) == 1 and r[key][0] is not None, key
    assert r["geometry_rows"] == [200 * 256] and r["geometry_chains"] == [256] and r["geometry_rows_left_out"] == [0]
    assert 1.0 <= r["geometry_condition_number"][0] and r["geometry_time_sec"][0] <= r["diagnostics_time_sec"][0]
    sp = helpers.spec("8schools")
    z = np.load(path(on, "_geometry.npz"))
    D = sp.D
    assert z["correlation"].shape == (D, D) and z["scale_coupling"].shape == (D, D) and z["elements"].shape == (D,)
    for key in ("mean", "sd", "eigenvalues", "step_scaled_eigenvalues", "eigenvalues_centred"):
        assert z[key].shape == (D,) and np.isfinite(z[key]).all(), key
    for part, shape in zip(sp.part_names, sp.part_shapes):
        assert z["stiffest_direction/" + part].shape == tuple(shape) and z["softest_direction/" + part].shape == tuple(shape)
    lines = analyze.report_geometry(analyze.load(str(tmp_path), "on"), str(tmp_path), "on")
    assert len([l for l in lines if "condition number" in l]) == 1 and any("stiffest direction" in l for l in lines)
    assert analyze.report_geometry(analyze.load(str(tmp_path), "off"), str(tmp_path), "off") == []

    two = str(tmp_path / "two")
    common = ["--model=radon", "--dataset=MN", "--num_chains=128", "--seed=3", "--num_optimization_steps=400",
              "--results_dir=" + two]
    hm = ["--num_samples=64", "--num_burnin_steps=200", "--num_adaptation_steps=150"]
    for m in ("CP", "NCP"):
        _cli(common + ["--inference=VI", "--method=" + m])
        _cli(common + ["--inference=HMCtuning", "--method=" + m, "--num_leapfrog_steps=4"] + hm)
    _cli(common + ["--inference=HMC", "--method=i", "--geometry_diagnostics"] + hm)
    r = json.load(open(os.path.join(two, "i_tied.json")))
    by = r["geometry_by_kernel"][0]
    assert len(by) == 2 and all(set(d) == set(cli.GEOMETRY_KERNEL_KEYS) for d in by)
    assert by[0]["geometry_condition_number"] == r["geometry_condition_number"][0]
    z = np.load(os.path.join(two, "i_tied_geometry.npz"))
    assert "correlation_1" in z.files and "scale_coupling_1" in z.files and "stiffest_direction_1/" + helpers.spec("radon_MN").part_names[0] in z.files
    # 64 x 128 rows of D = 88 (fewer rows than a long run: R is estimated, but both are estimates from the SAME rows):
    # entries of a correlation matrix from u of O(sd) are good to ~ (W + 1) 2^-24 = 1.5e-5 each
    assert np.nanmax(np.abs(z["correlation"] - z["correlation_centred"])) <= 1e-4
