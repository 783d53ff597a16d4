"""Multi-chain ESS on the device (arp_ess_multichain, diagnostics.ess_multichain / bulk_tail_ess, --bulk_tail_ess)
against the float64 yardstick tests/mcess_ref.py.

Tolerances.  rho: 3e-5, the project's float32 element tolerance; windows of at most 128
float products flushed into double bound the error by 128 x 2^-24 ~ 8e-6 of sum |y y'| <= n Gamma(0), a 4 x margin.
The cut: an element takes part only where no pair sum E + O the loop tested lies within 6e-4 of zero (ten times what
the rho tolerance can move a pair sum); the seeds below were chosen on the CPU so that EVERY element of every shape
does, and the tests assert that -- no element is excused.  ESS: the rho tolerance carried through tau,
|ESS - ESS64| <= ESS64 (2 max_t + 3) 3e-5 / tau64 (the monotone step is an averaging and does not amplify it).
"""
import ctypes as C
import functools
import json
import os
import shutil

import numpy as np
import pytest

import mcess_ref
import rank_rhat_ref
import rhat_ref
from test_gpu_rhat import CAP          # the moments' own tolerance (relative, on the variance's scale)

pytestmark = pytest.mark.gpu

RHO_TOL = 3e-5
MARGIN = 6e-4


def trend_case(seed):
    """(40, 2, 2): element 1 is a linear trend plus noise about chain levels 20 apart -- the pooled autocorrelation stays
    positive at every lag and the loop ends at the n - 5 limit."""
    x = mcess_ref.ar1_family(40, 2, 2, seed).astype(np.float64)
    rs = np.random.RandomState(seed + 1000)
    x[:, :, 1] = 0.1 * np.arange(40)[:, None] + 20.0 * np.arange(2)[None, :] + rs.randn(40, 2)
    return x.astype(np.float32)


# (64, 3, 300): no seed gives 600 cut margins (300 elements, split 0 and 1) that all clear 6e-4, so the trace is the first
# 300 of the family's 360 elements without these 16, whose margin on the CPU was below 1.2e-3 with seed 1
WIDE_DROP = (15, 31, 46, 61, 62, 81, 99, 125, 126, 158, 177, 245, 272, 294, 335, 346)


def wide_case(seed):
    x = mcess_ref.ar1_family(64, 3, 360, seed)
    keep = [d for d in range(360) if d not in WIDE_DROP][:300]
    return np.ascontiguousarray(x[:, :, keep])


# name -> (S, C, D), seed, maker
CASES = {
    "smallest": ((64, 4, 5), 1, None),
    "odd_S_D7": ((101, 3, 7), 2, None),
    "straddle": ((64, 67, 5), 1, None),
    "D130": ((64, 4, 130), 19, None),
    "D300": ((64, 3, 300), 1, lambda seed: wide_case(seed)),   # D > 256: every lane's sums are a partial, the fold walks the chains
    "several_blocks": ((1000, 64, 5), 6, None),
    "far_lags": ((600, 4, 1), 1, lambda seed: mcess_ref.ar1_family(600, 4, 1, seed, rhos=(0.99,))),
    "limit": ((40, 2, 2), 1, trend_case),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(trace [S, C, D] float32, {split: list of mcess_ref.Ess}) -- computed once, shared, never modified."""
    shape, seed, maker = CASES[name]
    x = maker(seed) if maker else mcess_ref.ar1_family(*shape, seed)
    assert x.shape == shape and x.dtype == np.float32
    x.setflags(write=False)
    return x, {s: mcess_ref.ess(x, bool(s)) for s in (0, 1)}


def ess_allowance(ref):
    return ref.ess * (2 * ref.max_t + 3) * RHO_TOL / ref.tau


def check_against(ref, ess, max_t, rho, label):
    """Every element of one device result against the yardstick's list `ref`; rho may be None."""
    worst_rho = 0.0
    for d, r in enumerate(ref):
        if np.isnan(r.ess):
            assert np.isnan(ess[d]) and max_t[d] == 0, (label, d)
            continue
        assert r.cut_margin >= MARGIN, "%s element %d: cut margin %.3g (pick another seed)" % (label, d, r.cut_margin)
        assert max_t[d] == r.max_t, (label, d, int(max_t[d]), r.max_t)
        if rho is not None:
            k = min(r.max_t + 2, rho.shape[0])
            err = np.abs(rho[:k, d].astype(np.float64) - r.rho[:k]).max()
            worst_rho = max(worst_rho, err)
            assert err <= RHO_TOL, (label, d, err)
            assert np.isnan(rho[r.max_t + 2:, d]).all(), (label, d)
        assert abs(ess[d] - r.ess) <= ess_allowance(r), (label, d, float(ess[d]), r.ess, ess_allowance(r))
    print("%s: largest |rho error| %.3g (allowed %.3g); cut lags %d .. %d" % (
        label, worst_rho, RHO_TOL, min(r.max_t for r in ref), max(r.max_t for r in ref)))


def run(gpu, x, split, threshold=None, n_rho=0):
    import torch
    from autoreparam_amd import diagnostics
    xd = x if torch.is_tensor(x) else torch.as_tensor(np.array(x, np.float32), device=gpu)
    thr = None if threshold is None else torch.as_tensor(np.asarray(threshold, np.float32), device=gpu)
    ess, max_t, rho = diagnostics.ess_multichain(xd, split=bool(split), threshold=thr, n_rho=n_rho)
    return ess.cpu().numpy(), max_t.cpu().numpy(), None if rho is None else rho.cpu().numpy()


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_shapes_against_the_yardstick(gpu, name, split):
    x, ref = case(name)
    n = x.shape[0] // 2 if split else x.shape[0]
    ess, max_t, rho = run(gpu, x, split, n_rho=n)
    check_against(ref[split], ess, max_t, rho, "%s split=%d" % (name, split))
    if name == "limit":
        assert ref[split][1].max_t >= n - 5            # the loop ran into its limit, not into a negative pair
    if name == "several_blocks":
        cuts = [r.max_t for r in ref[split]]
        assert max(cuts) >= 48 and min(cuts) <= 10     # one element spans several lag blocks, its wave-mates finished early
    if name == "far_lags":
        assert ref[split][0].max_t >= 32
    if name == "D300":
        # elements leave after block 0, 1, ... while others go on: a closed lane's stale partials must not be read
        last_block = sorted(set(r.max_t // 16 for r in ref[split]))
        assert len(last_block) >= 2 and last_block[0] == 0, last_block


def test_threshold_mode_is_the_indicator_trace(gpu):
    """x <= thr[d] inside the sweep: the yardstick on the materialised 0/1 trace, and bitwise the device run on it."""
    x, _ = case("odd_S_D7")
    thr = np.quantile(x.reshape(-1, x.shape[2]), 0.3, axis=0).astype(np.float32)
    ind = (x <= thr[None, None, :]).astype(np.float32)
    for split in (0, 1):
        ref = mcess_ref.ess(ind, bool(split))
        n = x.shape[0] // 2 if split else x.shape[0]
        got = run(gpu, x, split, threshold=thr, n_rho=n)
        check_against(ref, *got, "indicator split=%d" % split)
        mat = run(gpu, ind, split, n_rho=n)
        for a, b in zip(got, mat):
            assert a.tobytes() == b.tobytes()


def test_chain_sub_range_view_and_repeats_are_bitwise_equal(gpu):
    import torch
    x, _ = case("straddle")
    wide = torch.as_tensor(np.array(x, np.float32), device=gpu)
    lo, hi = 5, 42
    view = wide[:, lo:hi]
    assert not view.is_contiguous()
    n = x.shape[0] // 2
    a = run(gpu, view, 1, n_rho=n)
    b = run(gpu, view.contiguous(), 1, n_rho=n)
    c = run(gpu, view, 1, n_rho=n)
    for u, v, w in zip(a, b, c):
        assert u.tobytes() == v.tobytes() == w.tobytes()
    check_against(mcess_ref.ess(x[:, lo:hi], True), *a, "chains [5, 42)")


def test_degenerate_inputs(gpu):
    x, _ = case("smallest")
    # an element constant everywhere: NaN; the others are untouched
    y = x.copy()
    y[:, :, 2] = 1.5
    for split in (0, 1):
        ess, max_t, _ = run(gpu, y, split)
        assert np.isnan(ess[2]) and max_t[2] == 0
        check_against(mcess_ref.ess(y, bool(split)), ess, max_t, None, "constant element split=%d" % split)
    # one constant chain among moving ones: finite, the yardstick's value
    y = x.copy()
    y[:, 1, 3] = y[0, 1, 3]
    for split in (0, 1):
        ess, max_t, _ = run(gpu, y, split)
        assert np.isfinite(ess[3])
        check_against(mcess_ref.ess(y, bool(split)), ess, max_t, None, "constant chain split=%d" % split)
    # one chain
    y = np.ascontiguousarray(x[:, :1])
    for split in (0, 1):
        ess, max_t, _ = run(gpu, y, split)
        check_against(mcess_ref.ess(y, bool(split)), ess, max_t, None, "C=1 split=%d" % split)
    # fewer than four draws per row: NaN, never an error
    for S in (1, 2, 3, 7):
        for split in (0, 1):
            ess, max_t, rho = run(gpu, np.ascontiguousarray(x[:S]), split, n_rho=3)
            n = S // 2 if split else S
            if n < 4:
                assert np.isnan(ess).all() and (max_t == 0).all() and np.isnan(rho).all()
            else:
                check_against(mcess_ref.ess(x[:S], bool(split)), ess, max_t, None, "S=%d split=%d" % (S, split))


def test_nan_and_inf_leave_the_other_elements_alone(gpu):
    x, ref = case("smallest")
    y = x.copy()
    y[7, 1, 0] = np.nan
    y[9, 2, 0] = np.inf
    for split in (0, 1):
        ess, max_t, rho = run(gpu, y, split, n_rho=8)       # (run raises on a non-zero return)
        good = [mcess_ref.Ess(np.nan, 0, np.nan, np.zeros(0), np.inf, np.nan)] + ref[split][1:]
        e2, m2 = ess.copy(), max_t.copy()
        e2[0], m2[0] = np.nan, 0                               # (element 0: unspecified)
        check_against(good, e2, m2, None, "NaN / inf in element 0, split=%d" % split)


def test_argument_errors(gpu):
    import torch
    from autoreparam_amd import _lib
    L = _lib.lib()
    S, Cn, D = 64, 4, 5
    x = torch.zeros(S, Cn, D, device=gpu)
    ess = torch.full((D,), 7.0, device=gpu)
    need = int(L.arp_ess_multichain_workspace_bytes(S, Cn, D, 1))
    assert need > 0 and need % 256 == 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=gpu)
    assert ws.data_ptr() % 256 == 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ess_ptr, ws_ptr, ws_bytes, s=S, c=Cn):
        return L.arp_ess_multichain(C.c_void_p(x.data_ptr()), s, c, D, c * D, 1, C.c_void_p(0), C.c_void_p(ess_ptr),
                                    C.c_void_p(0), C.c_void_p(0), 0, C.c_void_p(ws_ptr), ws_bytes, st)

    for what, args in (("ess", (0, ws.data_ptr(), need)),
                       ("too small", (ess.data_ptr(), ws.data_ptr(), need - 1)),
                       ("aligned", (ess.data_ptr(), ws.data_ptr() + 4, need)),
                       ("2^31", (ess.data_ptr(), ws.data_ptr(), need, 1 << 20, 1 << 11)),
                       ("2^20 draws per row", (ess.data_ptr(), ws.data_ptr(), need, (1 << 21) + 2, 1))):
        rc = call(*args)
        msg = L.arp_last_error().decode()
        print("%s -> %d: %s" % (what, rc, msg))
        assert rc == 1 and "arp_ess_multichain" in msg and what in msg
    assert int(L.arp_ess_multichain_workspace_bytes(1 << 20, 1 << 11, D, 1)) == 0
    assert int(L.arp_ess_multichain_workspace_bytes((1 << 21) + 2, 1, D, 1)) == 0
    assert int(L.arp_ess_multichain_workspace_bytes(1 << 21, 1, D, 1)) > 0
    torch.cuda.synchronize()
    assert (ess.cpu().numpy() == 7.0).all()                    # nothing was launched
    assert call(ess.data_ptr(), ws.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert np.isnan(ess.cpu().numpy()).all()                   # (a trace of zeros never moved)


BT_SHAPE, BT_SEED = (200, 8, 6), 2


def test_bulk_tail_ess_against_the_yardstick(gpu):
    """bulk: the yardstick on the device's own z trace (z itself is held by test_gpu_rank.py); tail: on 1[x <= q] with
    the yardstick's order statistics; mean: on the draws; mcse_mean = sd / sqrt(ess_mean) with rhat_ref's pooled sd --
    the sd is allowed the moments' own tolerance (test_gpu_rhat.CAP), the ESS half its allowance (square root)."""
    import torch
    from autoreparam_amd import diagnostics
    x = mcess_ref.ar1_family(*BT_SHAPE, BT_SEED)
    D = x.shape[2]
    xd = torch.as_tensor(x, device=gpu)
    got = diagnostics.bulk_tail_ess(xd)
    assert all(v.shape == (D,) and v.dtype == np.float64 for v in got)
    z = diagnostics.rank_normalize(xd, fold=False)[0].cpu().numpy()
    q = rank_rhat_ref.quantiles(x, (0.05, 0.95))
    want_sd = rhat_ref.rhat(x, True)[2]
    bulk, mean = mcess_ref.ess(z, True), mcess_ref.ess(x, True)
    tails = [mcess_ref.ess((x <= q[i][None, None, :]).astype(np.float32), True) for i in (0, 1)]
    for d in range(D):
        for label, r, value in (("bulk", bulk[d], got.bulk[d]), ("mean", mean[d], got.mean[d])):
            assert r.cut_margin >= MARGIN, (label, d, r.cut_margin)
            assert abs(value - r.ess) <= ess_allowance(r), (label, d, value, r.ess)
        lo, hi = tails[0][d], tails[1][d]
        assert min(lo.cut_margin, hi.cut_margin) >= MARGIN, ("tail", d)
        assert abs(got.tail[d] - min(lo.ess, hi.ess)) <= max(ess_allowance(lo), ess_allowance(hi)), ("tail", d)
        assert abs(got.sd[d] - want_sd[d]) <= CAP * want_sd[d]
        want = want_sd[d] / np.sqrt(mean[d].ess)
        assert abs(got.mcse_mean[d] - want) <= want * (CAP + 0.5 * ess_allowance(mean[d]) / mean[d].ess), ("mcse", d)
    print("bulk %s\ntail %s\nmean %s" % (got.bulk, got.tail, got.mean))


def test_sees_what_the_per_chain_ess_cannot(gpu):
    """White noise about chain offsets of sd 3 (the input of tests/test_mcess_host.py): the multi-chain ESS of the mean is
    a few per cent of N while arp_ess, summed over the chains, calls the draws independent."""
    import torch
    from autoreparam_amd import diagnostics, util
    rs = np.random.RandomState(11)
    S, Cn = 400, 16
    x = (rs.randn(S, Cn, 1) + 3.0 * rs.randn(1, Cn, 1)).astype(np.float32)
    xd = torch.as_tensor(x, device=gpu)
    N = S * Cn
    ess_mean = float(diagnostics.ess_multichain(xd, split=True)[0].cpu()[0])
    per_chain = float(util.effective_sample_size(xd).sum().cpu())
    print("multi-chain %.1f, per-chain summed %.0f, N = %d" % (ess_mean, per_chain, N))
    assert ess_mean < 0.05 * N
    assert per_chain > 0.5 * N


CHAINS, SAMPLES = 64, 400
KEYS = ("ess_bulk_min", "ess_tail_min", "ess_mean_min", "mcse_mean_over_sd_max", "bulk_tail_ess_chains",
        "bulk_tail_ess_time_sec")
FAMILIES = ("ess_bulk", "ess_tail", "ess_mean", "mcse_mean")


def _cli(args):
    from autoreparam_amd import flags as flags_mod
    from autoreparam_amd import main as cli
    return cli.main(args, flags=flags_mod.FlagValues())


@pytest.fixture(scope="module")
def cli_run(gpu, tmp_path_factory):
    """The small run of test_gpu_rhat.py (8 schools, non-centred, 64 chains of 400 samples, every trace saved): the
    sampling run with --bulk_tail_ess and, in a copy of the directory made before it, without."""
    d = str(tmp_path_factory.mktemp("mcess_cli"))
    on, off = os.path.join(d, "on"), os.path.join(d, "off")
    common = ["--model=8schools", "--method=NCP", "--num_chains=%d" % CHAINS, "--seed=4"]
    hm = ["--num_samples=%d" % SAMPLES, "--num_burnin_steps=600", "--num_adaptation_steps=400"]
    _cli(common + ["--results_dir=" + on, "--inference=VI", "--num_optimization_steps=600"])
    _cli(common + ["--results_dir=" + on, "--inference=HMCtuning", "--num_leapfrog_steps=4"] + hm)
    shutil.copytree(on, off)
    sample = ["--inference=HMC", "--num_chains_to_save=%d" % CHAINS] + hm
    _cli(common + ["--results_dir=" + on, "--bulk_tail_ess"] + sample)
    _cli(common + ["--results_dir=" + off] + sample)
    return on, off


def test_cli_end_to_end(gpu, cli_run):
    import torch
    from autoreparam_amd import analyze, diagnostics, models
    on, off = cli_run
    r = json.load(open(os.path.join(on, "NCP_tied.json")))
    r_off = json.load(open(os.path.join(off, "NCP_tied.json")))
    assert set(r) == set(r_off) | set(KEYS) and not set(KEYS) & set(r_off)
    for k in r_off:                                            # every key it had before, unchanged (clocks aside)
        if not k.endswith(("time_sec", "time_secs")):
            assert r[k] == r_off[k], k
    for k in KEYS:
        assert isinstance(r[k], list) and len(r[k]) == 1 and k not in r["tuning_runs"][0], k
    assert r["bulk_tail_ess_chains"] == [CHAINS] and 0 < r["bulk_tail_ess_time_sec"][0] < 60
    sp = models.get_model_by_name("8schools", "").model
    z, z_off = np.load(os.path.join(on, "NCP_tied_rhat.npz")), np.load(os.path.join(off, "NCP_tied_rhat.npz"))
    new = ["%s/%s" % (f, n) for f in FAMILIES for n in sp.part_names]
    assert sorted(z.files) == sorted(z_off.files + new)
    for k in z_off.files:
        assert z[k].tobytes() == z_off[k].tobytes(), k
    tr = np.load(os.path.join(on, "NCP_tied_traces.npz"))
    x = np.concatenate([tr[n].reshape(SAMPLES, CHAINS, -1) for n in sp.part_names], axis=2).astype(np.float32)
    want = diagnostics.bulk_tail_ess(torch.as_tensor(x, device=gpu))
    for f, ref in zip(FAMILIES, (want.bulk, want.tail, want.mean, want.mcse_mean)):
        parts = [z["%s/%s" % (f, n)] for n in sp.part_names]
        assert [p.shape for p in parts] == [tuple(s) for s in sp.part_shapes]
        assert np.array_equal(np.concatenate([p.reshape(-1) for p in parts]), ref, equal_nan=True), f
    assert r["ess_bulk_min"][0] == np.nanmin(want.bulk) and r["ess_tail_min"][0] == np.nanmin(want.tail)
    assert r["ess_mean_min"][0] == np.nanmin(want.mean)
    assert r["mcse_mean_over_sd_max"][0] == np.nanmax(want.mcse_mean / want.sd)
    N = SAMPLES * CHAINS                                       # (tau >= 1 / log10 N)
    assert 0 < r["ess_bulk_min"][0] <= np.float32(N * np.log10(N)) and 0 < r["ess_tail_min"][0] <= np.float32(N * np.log10(N))
    lines = analyze.report_rhat({"NCP_tied": r}, on, "")
    assert any("multi-chain ESS min" in line for line in lines)
    assert not any("multi-chain ESS" in line for line in analyze.report_rhat({"NCP_tied": r_off}, off, ""))
