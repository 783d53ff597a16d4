"""GPU: the two kernels of csrc/mmatch.hip through diagnostics.weighted_moments / affine_rows, and diagnostics.moment_match,
against the numpy restatement of tests/mmatch_ref.py.

1. arp_weighted_moments against float64 numpy (sums in np.longdouble) within the header's bound (R' + 32) 2^-52 sum w |t|,
   nothing added: rows {1, 2, 63, 64, 65, 257, 4099} x columns {1, 2, 63, 64, 65, 255} x targets {1, 3, 17}, a view into a
   wider matrix, log weights spread over +-1e4, -inf entries, a target with nothing kept, one NaN, a centre far from the
   data; lw_max and the count exact; two calls bitwise equal; a target's row bitwise the same alone and among 17.
2. arp_affine_rows bit for bit against the float32 restatement: the same rows and columns, 1 and 5 targets, parity -1, 0, 1,
   NaN and inf rows among the copied ones, a strided x; forward then inverse (the host's parameters for it: m' = u,
   s' = 1 / s, u' = m) returns x within 4 units in the last place of max(|x|, |m|, |u|) -- at s = 1, where that bound is
   three roundings each way in one unit; at another scale u weighs |u| / s in x's units and the bound is not that one.
3. Every documented refusal through the C ABI: an error, its message, and outputs that keep their pattern.
4. diagnostics.moment_match on the closed-form case with torch float64 closures: the maps, S, U, k-hat and elpd of the
   restatement, the repair itself on the device's numbers, and batches of 1 and 3 bitwise equal."""
import ctypes as C

import numpy as np
import pytest
import torch

import mmatch_cases as mc
import mmatch_ref as mr
import psis_ref as pr
from test_gpu_psis import ELPD_MEASURED, FACTOR, K_MEASURED

pytestmark = pytest.mark.gpu

WORST = {"share": 0.0}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def strided(gpu, x, pad):
    """x on the device as a view into a matrix `pad` columns wider, the padding NaN (it is never read)."""
    wide = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=torch.float32, device=gpu)
    wide[:, :x.shape[1]] = torch.as_tensor(x, device=gpu)
    return wide[:, :x.shape[1]] if pad else wide


def device_moments(gpu, x, lw, centre, pad=0):
    from autoreparam_amd import diagnostics
    out = diagnostics.weighted_moments(strided(gpu, x, pad), torch.as_tensor(lw, device=gpu), torch.as_tensor(centre, device=gpu))
    return out.cpu().numpy()


def check_moments(got, x, lw, centre, what):
    ref, mag = mr.weighted_moments(x, lw, centre)
    D = x.shape[1]
    assert got.shape == ref.shape == (lw.shape[0], 4 + 2 * D)
    assert np.array_equal(got[:, 0], ref[:, 0]) and np.array_equal(got[:, 3], ref[:, 3]), what          # lw_max, the count: exact
    sums = [1, 2] + list(range(4, 4 + 2 * D))
    for b in range(lw.shape[0]):
        if np.isnan(lw[b]).any():
            assert np.isnan(got[b, sums]).all(), (what, b)
            continue
        allow = mr.bound(ref[b, 3], mag[b, sums])
        gap = np.abs(got[b, sums] - ref[b, sums])
        assert np.all(gap <= allow), (what, b, float(np.max(gap / np.maximum(allow, 1e-300))))
        if np.any(allow > 0):
            WORST["share"] = max(WORST["share"], float(np.max(gap[allow > 0] / allow[allow > 0])))
        if ref[b, 3] == 0:
            assert got[b, 0] == -np.inf and not got[b, 1:].any(), (what, b)


@pytest.mark.parametrize("D", mc.COLUMNS)
def test_weighted_moments_against_float64_at_every_walk(gpu, D):
    for R in mc.ROWS:
        for B in mc.TARGETS:
            x, lw, centre = mc.moments_case(R, D, B, seed=R * 1000 + D * 10 + B, far=(1.0e3 if B == 3 else 0.0))
            if B == 17:
                lw[5] = -np.inf                                           # nothing kept
                lw[7, R - 1] = np.nan                                     # one NaN: that target's sums and no other's
                lw[9] = 0.0                                               # the unweighted moments
            if R > 2:
                lw[-1, ::3] = -np.inf
                lw[:, R // 2] = -np.inf
                x[R // 2] = np.nan                                        # a draw every target leaves out may hold anything
            pad = 3 if (R + B) % 2 else 0
            got = device_moments(gpu, x, lw, centre, pad)
            check_moments(got, x, lw, centre, (R, D, B, pad))
            again = device_moments(gpu, x, lw, centre, pad)
            assert np.array_equal(bits(got), bits(again)), (R, D, B)       # two calls
            if B == 17:
                for b in (0, 7, 8, 16):                                   # alone, and at another place among others
                    alone = device_moments(gpu, x, lw[b:b + 1], centre, pad)
                    assert np.array_equal(bits(alone[0]), bits(got[b])), (R, D, b)
                moved = device_moments(gpu, x, lw[[16, 3, 0]], centre, pad)
                assert np.array_equal(bits(moved), bits(got[[16, 3, 0]])), (R, D)
    print("D = %d: largest share of the bound used so far %.3f" % (D, WORST["share"]))


def test_weighted_moments_of_zero_log_weights_are_the_plain_moments(gpu):
    x, _, centre = mc.moments_case(4099, 10, 1, seed=4)
    got = device_moments(gpu, x, np.zeros((1, 4099)), centre)
    e = x.astype(np.float64) - centre.astype(np.float64)[None]
    assert got[0, 0] == 0.0 and got[0, 1] == 4099.0 and got[0, 2] == 4099.0 and got[0, 3] == 4099.0
    assert np.allclose(got[0, 4::2], e.sum(axis=0), rtol=0, atol=4200 * 2.0 ** -52 * np.abs(e).sum(axis=0))
    assert np.allclose(got[0, 5::2], (e * e).sum(axis=0), rtol=4200 * 2.0 ** -52, atol=0)


@pytest.mark.parametrize("D", mc.COLUMNS)
def test_affine_rows_bit_for_bit(gpu, D):
    from autoreparam_amd import diagnostics
    for R in mc.ROWS:
        for B in mc.AFFINE_TARGETS:
            rng = np.random.default_rng(R * 100 + D + B)
            x = (rng.standard_normal((R, D)) * 5.0).astype(np.float32)
            if R > 2:
                x[1, 0], x[2, D - 1], x[R - 1, D // 2] = np.nan, np.inf, -np.inf
                x[0, 0] = np.float32(-0.0)
            m, u = (rng.standard_normal((B, D)).astype(np.float32) for _ in range(2))
            s = np.exp(rng.standard_normal((B, D)) * 0.5).astype(np.float32)
            pad = 5 if (R + B) % 2 else 0
            xd = strided(gpu, x, pad)
            up = lambda a: torch.as_tensor(a, device=gpu)
            for parity in (-1, 0, 1):
                got = diagnostics.affine_rows(xd, up(m), up(s), up(u), parity).cpu().numpy()
                want = mr.affine_rows(x, m, s, u, parity)
                # (a NaN that went through the map is a NaN; its payload is the hardware's)
                nan = np.isnan(want)
                assert got.shape == (B, R, D) and np.array_equal(np.isnan(got), nan), (R, D, B, parity)
                assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), (R, D, B, parity)
                if parity >= 0:                                            # the untouched rows, as bits
                    rest = (np.arange(R) & 1) != parity
                    assert np.array_equal(bits(got[:, rest]), bits(np.repeat(x[None, rest], B, axis=0))), (R, D, B, parity)


def test_affine_round_trip_at_unit_scale(gpu):
    """The forward map followed by the inverse one returns x within 4 units in the last place of max(|x|, |m|, |u|): three
    roundings each way, at s = 1 where the three magnitudes are in one unit."""
    from autoreparam_amd import diagnostics
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((4099, 65)) * 5.0).astype(np.float32)
    m, u = (rng.standard_normal((1, 65)).astype(np.float32) * 3 for _ in range(2))
    one = np.ones((1, 65), np.float32)
    up = lambda a: torch.as_tensor(a, device=gpu)
    fwd = diagnostics.affine_rows(up(x), up(m), up(one), up(u), -1)[0]
    back = diagnostics.affine_rows(fwd, up(u), up(one), up(m), -1)[0].cpu().numpy()
    scale = np.maximum(np.maximum(np.abs(x), np.abs(m)), np.abs(u)).astype(np.float32)
    assert np.all(np.abs(back.astype(np.float64) - x) <= 4 * np.spacing(scale))


def test_refusals_launch_nothing(gpu):
    from autoreparam_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    R, D, B = 65, 3, 2
    x = torch.zeros(R, D, dtype=torch.float32, device=gpu)
    lw = torch.zeros(B, R, dtype=torch.float64, device=gpu)
    centre = torch.zeros(D, dtype=torch.float32, device=gpu)
    need = int(L.arp_weighted_moments_workspace_bytes(R, D, B))
    assert need > 0 and need % 256 == 0
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=gpu)
    out = torch.full((B, 4 + 2 * D), -77.0, dtype=torch.float64, device=gpu)
    null = C.c_void_p(0)

    def moments(**k):
        a = dict(x=p(x), R=R, D=D, stride=D, lw=p(lw), B=B, lw_stride=R, centre=p(centre), out=p(out), ws=p(ws), bytes=need)
        a.update(k)
        return L.arp_weighted_moments(a["x"], a["R"], a["D"], a["stride"], a["lw"], a["B"], a["lw_stride"], a["centre"], a["out"],
                                      a["ws"], a["bytes"], _lib.stream())
    refused = [(dict(x=null), "x, lw, centre and out are required"), (dict(lw=null), "are required"),
               (dict(centre=null), "are required"), (dict(out=null), "are required"), (dict(R=0), "1 <= n_rows < 2\\^31"),
               (dict(R=1 << 31), "1 <= n_rows"), (dict(D=0), "1 <= D <= 255"), (dict(D=256), "1 <= D <= 255"),
               (dict(B=0), "n_targets <= 4096"), (dict(B=4097), "n_targets <= 4096"), (dict(stride=D - 1), "row_stride >= D"),
               (dict(lw_stride=R - 1), "lw_stride >= n_rows"), (dict(ws=null), "workspace too small"),
               (dict(bytes=need - 1), "workspace too small"), (dict(ws=C.c_void_p(ws.data_ptr() + 8)), "256-byte aligned")]
    for change, word in refused:
        assert moments(**change) == 1, change
        with pytest.raises(RuntimeError, match="arp_weighted_moments.*" + word):
            _lib.check(1)
    for shape in ((0, D, B), (R, 0, B), (R, 256, B), (R, D, 0), (R, D, 4097)):
        assert int(L.arp_weighted_moments_workspace_bytes(*shape)) == 0, shape
    torch.cuda.synchronize()
    assert bool((out == -77.0).all())
    assert moments() == 0
    torch.cuda.synchronize()
    assert not bool((out == -77.0).any())

    m = torch.zeros(B, D, dtype=torch.float32, device=gpu)
    res = torch.full((B, R, D), -77.0, dtype=torch.float32, device=gpu)

    def affine(**k):
        a = dict(x=p(x), R=R, D=D, stride=D, m=p(m), s=p(m), u=p(m), B=B, parity=-1, out=p(res))
        a.update(k)
        return L.arp_affine_rows(a["x"], a["R"], a["D"], a["stride"], a["m"], a["s"], a["u"], a["B"], a["parity"], a["out"],
                                 _lib.stream())
    refused = [(dict(x=null), "are required"), (dict(m=null), "are required"), (dict(s=null), "are required"),
               (dict(u=null), "are required"), (dict(out=null), "are required"), (dict(R=0), "1 <= n_rows"),
               (dict(D=256), "1 <= D <= 255"), (dict(B=0), "n_targets"), (dict(B=4097), "n_targets"),
               (dict(stride=D - 1), "row_stride >= D"), (dict(parity=2), "parity <= 1"), (dict(out=p(x)), "out != x"),
               (dict(R=(1 << 31) - 1, D=255, B=4096, stride=255), "2\\^35")]
    for change, word in refused:
        assert affine(**change) == 1, change
        with pytest.raises(RuntimeError, match="arp_affine_rows.*" + word):
            _lib.check(1)
    torch.cuda.synchronize()
    assert bool((res == -77.0).all())
    assert affine() == 0
    torch.cuda.synchronize()
    assert bool((res == 0.0).all())


# ---- the algorithm ----
def closures(case):
    y, var = case
    logp = lambda rows: -0.5 * (rows.to(torch.float64) ** 2).sum(dim=1)
    loglik = lambda t, rows: -0.5 * (y - rows[:, 0].to(torch.float64)) ** 2 / var - 0.5 * float(np.log(2.0 * np.pi * var))
    return logp, loglik


def run_device(gpu, case, seeds, batch):
    from autoreparam_amd import diagnostics
    out = []
    tau = diagnostics.pareto_k_threshold(mc.DRAWS)
    logp, loglik = closures(case)
    for seed in seeds:
        x = torch.as_tensor(mc.draws(seed), device=gpu)
        # three targets: the same term three times -- every one of them must come out the same, whatever the batch
        l0 = loglik(0, x).to(torch.float32)
        plain = diagnostics.psis_loo(torch.stack([l0] * 3)).cpu().numpy()
        left = torch.zeros(mc.DRAWS, dtype=torch.bool, device=gpu)
        out.append((plain, diagnostics.moment_match(x, left, logp, loglik, [0, 1, 2], plain[:, 1], plain[:, 0], tau, batch=batch)))
    return out


def test_moment_match_follows_the_restatement_and_repairs_the_estimate(gpu):
    exact = mc.exact_elpd(mc.HIGH)
    tau = pr.k_threshold(mc.DRAWS)
    by_three = run_device(gpu, mc.HIGH, mc.SEEDS, 3)
    by_one = run_device(gpu, mc.HIGH, mc.SEEDS, 1)
    for seed, (plain, res), (_, single) in zip(mc.SEEDS, by_three, by_one):
        x = mc.draws(seed)
        ref = mr.moment_match(x, np.zeros(mc.DRAWS, bool), mc.logp, lambda t, rows: mc.loglik(mc.HIGH, rows), [0], plain[:1, 1],
                              plain[:1, 0], tau)
        print("seed %d: plain k %.3f error %.3f; device k %.3f error %.3f maps %s (reference k %.3f error %.3f maps %s); "
              "k_full %.3f k_split %.3f ESS %.0f" % (seed, plain[0, 1], plain[0, 0] - exact, res.pareto_k[0], res.elpd[0] - exact,
                                                     res.maps[0], ref.pareto_k[0], ref.elpd[0] - exact, ref.maps[0],
                                                     res.pareto_k_full[0], res.pareto_k_split[0], res.is_ess[0]))
        assert res.attempted.all() and res.maps[0] == ref.maps[0] and res.iterations[0] == len(ref.maps[0])
        # S, U to the float32 rounding of the parameters
        assert np.allclose(res.scale[0], ref.scale[0], rtol=2.0 ** -22, atol=0)
        assert np.allclose(res.shift[0] + res.centre, ref.shift[0] + ref.centre, rtol=0, atol=2.0 ** -22 * np.abs(ref.shift[0]).max())
        # k-hat and elpd within what tests/psis_checks.py holds arp_psis_weights to (test_gpu_psis's constants)
        for name in ("pareto_k", "pareto_k_full", "pareto_k_split"):
            assert abs(getattr(res, name)[0] - getattr(ref, name)[0]) <= FACTOR * K_MEASURED, name
        assert abs(res.elpd[0] - ref.elpd[0]) <= FACTOR * ELPD_MEASURED
        assert res.is_ess[0] == pytest.approx(ref.is_ess[0], rel=1e-6)
        # the repair, on the device's own numbers
        assert plain[0, 1] > tau and len(res.maps[0]) >= 1 and res.pareto_k[0] < plain[0, 1]
        assert abs(res.elpd[0] - exact) <= 0.25 * abs(plain[0, 0] - exact)
        # the three identical targets, and batches of 1 and 3
        for field in ("elpd", "pareto_k", "pareto_k_full", "pareto_k_split", "is_ess", "scale", "shift"):
            a, b = getattr(res, field), getattr(single, field)
            assert np.array_equal(bits(np.asarray(a, np.float64)), bits(np.asarray(b, np.float64))), (seed, field)
            assert all(np.array_equal(bits(np.asarray(a[0], np.float64)), bits(np.asarray(a[t], np.float64))) for t in (1, 2)), field
        assert res.maps == single.maps and res.maps[0] == res.maps[1] == res.maps[2]


def test_moment_match_leaves_a_low_k_alone_and_honours_left_out_draws(gpu):
    from autoreparam_amd import diagnostics
    for plain, res in run_device(gpu, mc.LOW, mc.SEEDS[:2], 3):
        assert not res.attempted.any() and res.maps == ["", "", ""]
        assert np.array_equal(bits(res.elpd), bits(plain[:, 0])) and np.array_equal(bits(res.pareto_k), bits(plain[:, 1]))
        assert np.isnan(res.scale).all() and np.isnan(res.is_ess).all()
    # draws left out (their rows NaN) enter nothing: the result is that of the kept draws, as the restatement has it
    tau = pr.k_threshold(mc.DRAWS - 7)
    x = mc.draws(1)
    left = np.zeros(mc.DRAWS, bool)
    left[[0, 5, 64, 65, 1000, 4094, 4095]] = True
    x[left] = np.nan
    logp, loglik = closures(mc.HIGH)
    xd, ld = torch.as_tensor(x, device=gpu), torch.as_tensor(left, device=gpu)
    l0 = torch.where(ld, torch.zeros((), dtype=torch.float64, device=gpu), loglik(0, xd)).to(torch.float32)
    plain = diagnostics.psis_loo(l0[None], ld.to(torch.uint8)).cpu().numpy()
    res = diagnostics.moment_match(xd, ld, logp, loglik, [0], plain[:, 1], plain[:, 0], tau, batch=2)
    with np.errstate(all="ignore"):
        ref = mr.moment_match(x, left, mc.logp, lambda t, rows: mc.loglik(mc.HIGH, rows), [0], plain[:, 1], plain[:, 0], tau)
    assert res.maps == ref.maps and len(res.maps[0]) >= 1 and np.isfinite(res.elpd[0])
    assert abs(res.pareto_k[0] - ref.pareto_k[0]) <= FACTOR * K_MEASURED
    assert abs(res.elpd[0] - ref.elpd[0]) <= FACTOR * ELPD_MEASURED
