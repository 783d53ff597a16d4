"""GPU: the trajectory-length profile (trajectory_probe_kernel, arp_trajectory_probe, arp_jump_sums,
Engine.trajectory_probe / trajectory_sums, --trajectory_profile) -- fresh-momentum trajectories with every step recorded,
not replays of the sampler's transitions -- against the float64 replay of tests/trajectory_ref.py with the momenta the
device drew; the momentum stream it shares with the energy probe; the centred path; the fold against numpy float64; the
agreement with the sampler's realised jump; chunking; non-interference; refusals; the CLI.

Measured on an MI355X (largest deviation / tolerance of the parity test and of the fold, per quantity): DESIGN.md section 5."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

import energy_ref as er
import helpers
import trajectory_ref as tr

pytestmark = pytest.mark.gpu


def _engine(gpu, mname, options=()):
    from autoreparam_amd import engine
    eng = engine.Engine(helpers.spec(mname), gpu)
    for key, value in options:
        eng.set_option(key, value)
    return eng


def _np(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------
# 1. parity with the float64 replay
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", er.KINDS)
@pytest.mark.parametrize("mname,lanes,options", er.CASES, ids=["%s-%d%s" % (m, k, "-" + o[0][1] if o else "") for m, k, o in er.CASES])
def test_path_matches_float64_replay(oracle_lib, gpu, mname, lanes, options, kind):
    """lp0, ke0 and, at every l = 1 ... Lmax, the energy error of a trajectory of l steps and the state after step l (sampler
    coordinates) of every probed row against trajectory_ref.replay_path in float64 from the momenta the device drew:
    Lmax = 1 and 5, one row, a ragged wave and (one parameterisation per model) more than a workgroup, per-row step
    multipliers and none.  Bars: energy_ref.bars, calibrated on the CPU (tests/test_trajectory_host.py).  No row is left out
    and everything is finite."""
    sp = helpers.spec(mname)
    eng = _engine(gpu, mname, options)
    orc = oracle_lib.OracleModel(sp)
    a, b = helpers.params(sp, kind)
    eng.set_param(0, (a, b))
    worst, failed = {}, []
    for n in er.row_counts(lanes, kind):
        x = helpers.states(sp, n, seed=n, scale=er.STATE_SCALE)
        eps = er.eps0(orc, sp, a, b, x, tr.frac(mname))
        for Lmax in tr.LEAPFROGS_MAX:
            for kap in (None, er.kappas(n, n)):
                energy, path, p = eng.trajectory_probe(x, eps, Lmax, which=0, kappa=kap, seed=11, row_offset=5, lanes=lanes,
                                                       want_path=True, path_centred=False, want_p=True)
                energy, path, p = _np(energy), _np(path), _np(p)
                assert energy.shape == (Lmax + 1, n, 2) and path.shape == (Lmax, n, sp.D) and p.shape == (n, sp.D)
                assert np.isfinite(energy).all() and np.isfinite(path).all() and np.isfinite(p).all()
                ref = tr.replay_path(orc, a, b, x, p, eps, kap, Lmax, np.float64)
                for key, r in tr.ratios_by_step((energy[:, :, 0], energy[:, :, 1], path), ref, p).items():
                    worst[key] = max(worst.get(key, 0.0), r) if r == r else float("nan")
                    if not r <= 1.0:
                        failed.append((key, n, Lmax, kap is not None, r))
    print("trajectory probe %s lanes=%d %s %s: deviation / tolerance %s" % (
        mname, lanes, dict(options), kind, {k: round(v, 4) for k, v in worst.items()}))
    assert not failed, failed[:8]


# ---------------------------------------------------------------------------
# 2. the momentum stream is the energy probe's
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mname,lanes,options", er.CASES, ids=["%s-%d%s" % (m, k, "-" + o[0][1] if o else "") for m, k, o in er.CASES])
def test_same_stream_as_the_energy_probe(gpu, mname, lanes, options):
    """Every family and lane shape: p_out and ke0 are arp_energy_probe's bit for bit for equal (seed, row_offset, lanes) --
    the two kernels restate the same lines, and this is what keeps them in step (lp0 is not compared: nothing promises the
    bits of a gradient inlined into two kernels); rows [k, k + m) at offset 0 equal rows [0, m) at offset k in every output."""
    sp = helpers.spec(mname)
    eng = _engine(gpu, mname, options)
    eng.set_param(0, helpers.params(sp, "VIP"))
    n, k, m, Lmax = 300, 100, 70, 3
    x = helpers.states(sp, n, seed=1, scale=0.1)
    eps = np.full(sp.D, 1e-3, np.float32)
    kap = er.kappas(n, 3)
    for seed, offset in ((3, 0), (4, 12345678901)):
        out, p_e = eng.energy_probe(x, eps, Lmax, kappa=kap, seed=seed, row_offset=offset, lanes=lanes, want_p=True)
        energy, path, p = eng.trajectory_probe(x, eps, Lmax, kappa=kap, seed=seed, row_offset=offset, lanes=lanes, want_p=True)
        assert np.array_equal(_np(p), _np(p_e)) and np.isfinite(_np(p)).all()
        assert np.array_equal(_np(energy)[0, :, 1], _np(out)[:, 1]) and np.isfinite(_np(out)[:, 1]).all()
    whole = [_np(t) for t in eng.trajectory_probe(x, eps, Lmax, kappa=kap, seed=3, row_offset=0, lanes=lanes, want_p=True)]
    part = [_np(t) for t in eng.trajectory_probe(x[k:k + m], eps, Lmax, kappa=kap[k:k + m], seed=3, row_offset=k, lanes=lanes,
                                                 want_p=True)]
    # (the bits: at these steps time_series leaves float32, and NaN is a result like any other)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(bits(part[0]), bits(whole[0][:, k:k + m])) and np.array_equal(bits(part[1]), bits(whole[1][:, k:k + m]))
    assert np.array_equal(part[2], whole[2][k:k + m])
    other = _np(eng.trajectory_probe(x[k:k + m], eps, Lmax, kappa=kap[k:k + m], seed=3, row_offset=k + 1, lanes=lanes, want_p=True)[2])
    assert not np.array_equal(other, part[2])


# ---------------------------------------------------------------------------
# 3. the centred path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mname,lanes", [("8schools", 1), ("funnel", 1), ("radon_MA", 4), ("radon_sd_AZ", 8), ("election", 4),
                                         ("electric", 8), ("time_series", 4), ("german", 4)])
def test_centred_path(oracle_lib, gpu, mname, lanes):
    """path_centred = 1 against Engine.transform of the sampler-coordinate path of an otherwise identical call, at the
    tolerance tests/test_gpu_density.py::test_converter_properties holds the converters to; the flag changes nothing else:
    energies equal bit for bit, and so are two sampler-coordinate paths."""
    sp = helpers.spec(mname)
    eng = _engine(gpu, mname)
    a, b = helpers.params(sp, "VIP")
    eng.set_param(0, (a, b))
    n, Lmax = 67, 3
    x = helpers.states(sp, n, seed=6, scale=er.STATE_SCALE)
    eps = er.eps0(oracle_lib.OracleModel(sp), sp, a, b, x, tr.frac(mname))      # (the parity test's steps: finite for every model)
    kw = dict(kappa=er.kappas(n, 1), seed=8, row_offset=2, lanes=lanes)
    e_s, path_s = eng.trajectory_probe(x, eps, Lmax, path_centred=False, **kw)
    e_s2, path_s2 = eng.trajectory_probe(x, eps, Lmax, path_centred=False, **kw)
    e_c, path_c = eng.trajectory_probe(x, eps, Lmax, path_centred=True, **kw)
    e_none = eng.trajectory_probe(x, eps, Lmax, want_path=False, **kw)
    assert np.isfinite(_np(path_s)).all() and np.isfinite(_np(path_c)).all() and np.isfinite(_np(e_s)).all()
    assert np.array_equal(_np(path_s), _np(path_s2))
    assert np.array_equal(_np(e_s), _np(e_s2)) and np.array_equal(_np(e_s), _np(e_c)) and np.array_equal(_np(e_s), _np(e_none))
    want = _np(eng.transform(path_s.reshape(Lmax * n, sp.D), which=0, to_centered=True)).reshape(Lmax, n, sp.D)
    tol = 5e-5 if mname == "time_series" else 2e-5
    np.testing.assert_allclose(_np(path_c), want, rtol=tol, atol=tol)
    assert not np.array_equal(_np(path_c), _np(path_s))                       # (the parameterisation is not the identity)


# ---------------------------------------------------------------------------
# 4. the fold
# ---------------------------------------------------------------------------
# (tile - 1, tile, tile + 1 rows; 4 099: seventeen partials for the second stage, more than one batch of its loads)
FOLD_ROWS = tuple(sorted({1, 2, 63, 64, 65, 257, tr.JUMP_TILE - 1, tr.JUMP_TILE, tr.JUMP_TILE + 1, 4099}))


def _fold_case(n, D, Lmax, seed):
    """Random trajectories with planted rows (as many as n holds).  Returns x0 [n, D], path [Lmax, n, D], energy
    [Lmax + 1, n, 2] float32."""
    rs = np.random.RandomState(seed)
    x0 = rs.randn(n, D).astype(np.float32)
    path = (x0[None] + (0.5 + rs.rand(Lmax, n, 1)) * rs.randn(Lmax, n, D)).astype(np.float32)
    energy = np.stack([3.0 * rs.randn(Lmax + 1, n), 5.0 * rs.rand(Lmax + 1, n)], axis=2).astype(np.float32)
    last = Lmax

    def plant(row, l, dh):                      # an exact energy error at step l of `row`
        energy[0, row] = (0.0, 0.0)
        energy[l, row] = (-dh, 0.0)
    if n > 1:
        energy[1, 1, 0] = np.nan                # NaN energy: alpha = 0 ...
        path[0, 1, :] = np.nan                  # ... and a NaN path under it is ignored
    if n > 2:
        energy[last, 2, 1] = np.inf
    if n > 3:
        energy[0, 3, 0] = -np.inf               # not finite at every l
    if n > 4:
        plant(4, 1, 999.5)                      # not divergent (alpha underflows to 0: skipped)
    if n > 5:
        plant(5, last, 1000.5)                  # divergent
    if n > 6:
        plant(6, 1, -5000.0)                    # alpha = 1
    if n > 7:
        path[0, 7, D // 2] = np.nan             # NaN under alpha > 0: left out
    if n > 8:
        path[last - 1, 8, 0] = np.inf           # inf under alpha > 0: left out
    if n > 9:
        plant(9, 1, 1000.5)
        path[0, 9, :] = np.inf                  # under alpha = 0: ignored
    return x0, path, energy


def _fold(gpu, x0, path, energy):
    from autoreparam_amd import _lib
    L = _lib.lib()
    Lmax, n, D = path.shape
    t = [torch.as_tensor(np.ascontiguousarray(v), device=gpu) for v in (x0, path, energy)]
    sums = torch.full((Lmax, 5 + D), -7.0, dtype=torch.float64, device=gpu)
    with torch.cuda.device(gpu):
        need = int(L.arp_jump_workspace_bytes(n, D, Lmax))
        tiles = (n + tr.jump_tile(n, Lmax) - 1) // tr.jump_tile(n, Lmax)
        assert need == (0 if tiles == 1 else (tiles * Lmax * (5 + D) * 8 + 255) // 256 * 256)
        ws = torch.empty(need, dtype=torch.uint8, device=gpu) if need else None
        _lib.check(L.arp_jump_sums(_lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), n, D, Lmax, _lib.ptr(sums), _lib.ptr(ws),
                                   need, _lib.stream()))
        torch.cuda.synchronize()
    return _np(sums)


def _fold_ratio(got, want):
    """Counts exact; sum of alpha and J within FOLD_ALLOWANCE of the sum of |terms| (the terms are non-negative: the sum
    itself).  Returns the largest deviation / allowance."""
    exact = [0, 1, 2, 4]
    assert np.array_equal(got[:, exact], want[:, exact]), (got[:, exact], want[:, exact])
    assert np.isfinite(got).all()
    dev, allow = np.abs(got - want), tr.FOLD_ALLOWANCE * np.abs(want)
    assert (dev <= allow).all(), float(np.max(dev[allow > 0] / allow[allow > 0]))
    return float(np.max(dev[allow > 0] / allow[allow > 0])) if (allow > 0).any() else 0.0


@pytest.mark.parametrize("D", [1, 2, 71, 125, 256])
def test_fold_against_numpy(gpu, D):
    """arp_jump_sums on synthetic inputs with planted rows, every row count (tile edges, several partials) x Lmax 1 and 3:
    counts exact, sums within the allowance, two calls bitwise equal, and the sums of a split of the rows add to the
    whole's within the same allowance."""
    worst = 0.0
    for n in FOLD_ROWS:
        for Lmax in (1, 3):
            x0, path, energy = _fold_case(n, D, Lmax, seed=n + Lmax)
            want = tr.jump_sums(x0, path, energy)
            got = _fold(gpu, x0, path, energy)
            assert got[0, 0] == n
            if n > 9:
                assert want[0, 4] >= 1 and want[Lmax - 1, 4] >= 1 and want[0, 2] >= 2 and want[Lmax - 1, 1] >= 3    # (the planted rows count)
            worst = max(worst, _fold_ratio(got, want))
            assert np.array_equal(got, _fold(gpu, x0, path, energy))
            if n >= 65:
                cut = n // 3 + 1
                parts = _fold(gpu, x0[:cut], path[:, :cut], energy[:, :cut]) + _fold(gpu, x0[cut:], path[:, cut:], energy[:, cut:])
                worst = max(worst, _fold_ratio(parts, want))
    print("jump fold D=%d: largest deviation / allowance %.4f" % (D, worst))


@pytest.mark.parametrize("grow", [2, 4])
def test_fold_large_tiles(gpu, grow):
    """Enough rows that a workgroup's tile is 2 and 4 times the base tile (trajectory_ref.jump_tile): one row fewer than, equal
    to and more than a whole number of tiles."""
    D, Lmax = 2, 3
    tiles = 700                                           # (700 x 512 x 3 and 700 x 1 024 x 3 row-steps: the tile has grown `grow`-fold)
    worst = 0.0
    for n in (tiles * grow * tr.JUMP_TILE - 1, tiles * grow * tr.JUMP_TILE, tiles * grow * tr.JUMP_TILE + 1):
        assert tr.jump_tile(n, Lmax) == grow * tr.JUMP_TILE
        x0, path, energy = _fold_case(n, D, Lmax, seed=grow)
        got = _fold(gpu, x0, path, energy)
        worst = max(worst, _fold_ratio(got, tr.jump_sums(x0, path, energy)))
    assert np.array_equal(got, _fold(gpu, x0, path, energy))
    print("jump fold, tile x %d: largest deviation / allowance %.4f" % (grow, worst))


def test_fold_wide_rows(gpu):
    """D above the workgroup's width (column tiles) and not a multiple of it."""
    x0, path, energy = _fold_case(130, 600, 2, seed=1)
    _fold_ratio(_fold(gpu, x0, path, energy), tr.jump_sums(x0, path, energy))


# ---------------------------------------------------------------------------
# 5. agreement with the sampler
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mname,kind,frac", [("8schools", "NCP", 0.1), ("radon_MA", "CP", 0.5)])
def test_profile_agrees_with_the_sampler(oracle_lib, gpu, mname, kind, frac):
    """4 096 chains, fixed step, L = 4, 300 transitions; the profile of the final states at Lmax = 4, then one more
    transition of the sampler: J[4] / rows against the realised centred squared jump, within 5 sigma per element and for the
    standardised total (tests/test_trajectory_host.py holds the oracle to the same); no divergent row, an acceptance at
    which the test can tell; and arp_jump_sums / rows equals the host's float64 mean of the same device outputs."""
    from autoreparam_amd import engine
    sp = helpers.spec(mname)
    eng = _engine(gpu, mname)
    orc = oracle_lib.OracleModel(sp)
    a, b = helpers.params(sp, kind)
    eng.set_param(0, (a, b))
    Cn, L = 4096, 4
    q0 = helpers.states(sp, Cn, seed=2, scale=0.1)
    eps = er.eps0(orc, sp, a, b, q0, frac)
    st = engine.ChainState(torch.as_tensor(q0, device=gpu))
    eng.hmc_run(st, eps, L, 300, seed=9)
    q = st.q.clone()
    sums, energy = eng.trajectory_sums(q, eps, L, seed=33, lanes=4)
    _, path = eng.trajectory_probe(q, eps, L, seed=33, lanes=4, path_centred=True)
    before = st.accept_count.clone()
    eng.hmc_run(st, eps, L, 1, seed=9)
    rate = float(_np((st.accept_count - before).to(torch.float64)).mean())
    x0, x1 = _np(eng.transform(q, which=0, to_centered=True)), _np(eng.transform(st.q, which=0, to_centered=True))
    sums, energy, path = _np(sums), _np(energy), _np(path)
    alpha, divergent, _ = tr.alphas(energy)
    assert sums[L - 1, 0] == Cn and not divergent.any() and (sums[:, 1] == 0).all() and (sums[:, 4] == 0).all()
    host = (alpha[L - 1][:, None] * (path[L - 1].astype(np.float64) - x0.astype(np.float64)) ** 2).mean(axis=0)
    assert np.allclose(sums[L - 1, 5:] / Cn, host, rtol=1e-12, atol=0)
    assert abs(sums[L - 1, 3] / Cn - alpha[L - 1].mean()) <= 1e-12
    z, z_total = tr.sampler_pair(x0, x1, alpha[L - 1], path[L - 1])
    print("profile vs sampler %s %s: acceptance %.4f (probe %.4f), largest |z| %.2f, total z %.2f" % (
        mname, kind, rate, alpha[L - 1].mean(), np.abs(z).max(), z_total))
    assert 0.2 < rate < 0.999
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.0 and abs(z_total) <= 5.0


# ---------------------------------------------------------------------------
# 6. chunking is invisible
# ---------------------------------------------------------------------------
def test_chunking_is_invisible(gpu):
    """trajectory_sums with a max_path_bytes that forces three chunks against one chunk: energies equal bit for bit, sums
    within the fold allowance."""
    sp = helpers.spec("radon_MA")
    eng = _engine(gpu, "radon_MA")
    eng.set_param(0, helpers.params(sp, "VIP"))
    n, Lmax = 1300, 4
    x = helpers.states(sp, n, seed=7, scale=0.1)
    eps = np.full(sp.D, 0.05, np.float32)
    kw = dict(kappa=er.kappas(n, 4), seed=5, row_offset=77, lanes=4)
    one_s, one_e = eng.trajectory_sums(x, eps, Lmax, **kw)
    rows = (n + 2) // 3
    calls = []
    probe = eng.trajectory_probe
    eng.trajectory_probe = lambda xs, *args, **kwargs: (calls.append(int(xs.shape[0])), probe(xs, *args, **kwargs))[1]
    three_s, three_e = eng.trajectory_sums(x, eps, Lmax, max_path_bytes=rows * Lmax * sp.D * 4, **kw)
    assert calls == [rows, rows, n - 2 * rows]
    assert np.array_equal(_np(one_e), _np(three_e)) and np.isfinite(_np(one_e)).all()
    _fold_ratio(_np(three_s), _np(one_s))


# ---------------------------------------------------------------------------
# 7. non-interference
# ---------------------------------------------------------------------------
def test_profile_changes_nothing(gpu):
    """x is unchanged by a profile, and an hmc_run after a profile is bitwise the run without it."""
    from autoreparam_amd import engine
    sp = helpers.spec("radon_MA")
    eps = np.full(sp.D, 0.05, np.float32)
    q0 = helpers.states(sp, 300, seed=3, scale=0.1)

    def run(profile):
        eng = _engine(gpu, "radon_MA")
        eng.set_param(0, "NCP")
        st = engine.ChainState(torch.as_tensor(q0, device=gpu))
        eng.hmc_run(st, eps, 4, 10, seed=5)
        if profile:
            x = st.q.clone()
            eng.trajectory_probe(st.q, eps, 6, kappa=st.adapt[:, 0].contiguous(), seed=6, path_centred=True, want_p=True)
            eng.trajectory_sums(st.q, eps, 6, kappa=st.adapt[:, 0].contiguous(), seed=6)
            assert torch.equal(x, st.q)
        eng.hmc_run(st, eps, 4, 10, seed=5)
        torch.cuda.synchronize()
        return st
    a, b = run(False), run(True)
    for name in ("q", "grad", "logp", "rng", "accept_count", "adapt"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
def test_refusals(gpu):
    """A null handle, x, eps0 or energy_out, `which` outside 0 / 1, n_rows < 1 or too large for one launch, n_leapfrog_max < 1
    or > 256; a null x0, path, energy or sums of the fold, its shapes, a missing workspace: non-zero, a message that names
    the function, and nothing written."""
    from autoreparam_amd import _lib
    sp = helpers.spec("8schools")
    eng = _engine(gpu, "8schools")
    eng.set_param(0, "CP")
    L = _lib.lib()
    n, Lmax, D = 5, 2, sp.D
    x = torch.zeros(n, D, device=gpu)
    eps = torch.full((D,), 0.1, device=gpu)
    energy = torch.full((Lmax + 1, n, 2), 7.0, device=gpu)
    path = torch.full((Lmax, n, D), 7.0, device=gpu)
    sums = torch.full((Lmax, 5 + D), 7.0, dtype=torch.float64, device=gpu)
    null = C.c_void_p(0)
    good = dict(m=eng._h, which=0, x=_lib.ptr(x), n=n, L=Lmax, eps=_lib.ptr(eps), out=_lib.ptr(energy))
    bad = [dict(m=null), dict(x=null), dict(eps=null), dict(out=null), dict(which=-1), dict(which=2), dict(n=0), dict(n=-3),
           dict(L=0), dict(L=-1), dict(L=257), dict(n=0x7fffffff // 16 + 1)]

    def probe(k):
        return L.arp_trajectory_probe(k["m"], k["which"], k["x"], k["n"], k["L"], k["eps"], null, 1, 0, k["out"], _lib.ptr(path),
                                      1, null, 0, _lib.stream())
    fgood = dict(x0=_lib.ptr(x), path=_lib.ptr(path), e=_lib.ptr(energy), n=n, D=D, L=Lmax, sums=_lib.ptr(sums))
    fbad = [dict(x0=null), dict(path=null), dict(e=null), dict(sums=null), dict(n=0), dict(n=-1), dict(D=0), dict(L=0),
            dict(L=257), dict(n=0x7fffffff // 16 + 1), dict(n=tr.JUMP_TILE + 1)]         # (the last: no workspace)

    def fold(k):
        return L.arp_jump_sums(k["x0"], k["path"], k["e"], k["n"], k["D"], k["L"], k["sums"], null, 0, _lib.stream())
    with torch.cuda.device(gpu):
        for change in bad:
            assert probe(dict(good, **change)) != 0 and b"arp_trajectory_probe" in L.arp_last_error(), change
        for change in fbad:
            assert fold(dict(fgood, **change)) != 0 and b"arp_jump_sums" in L.arp_last_error(), change
        assert L.arp_jump_workspace_bytes(0, D, Lmax) == 0 and L.arp_jump_workspace_bytes(n, D, 257) == 0
        torch.cuda.synchronize()
        assert bool((energy == 7.0).all()) and bool((path == 7.0).all()) and bool((sums == 7.0).all())
        assert probe(good) == 0
        assert fold(fgood) == 0
        torch.cuda.synchronize()
    assert bool(torch.isfinite(energy).all()) and not bool((energy == 7.0).any()) and not bool((path == 7.0).any())
    assert bool(torch.isfinite(sums).all()) and bool((sums[:, 0] == n).all())
    with pytest.raises(RuntimeError):
        eng.trajectory_probe(_np(x), _np(eps), 2, lanes=3)


# ---------------------------------------------------------------------------
# 9. the CLI
# ---------------------------------------------------------------------------
KERNEL_KEYS = ("trajectory_accept_prob", "trajectory_divergence_rate", "trajectory_esjd_min", "trajectory_esjd_min_element",
               "trajectory_esjd_min_per_gradient", "trajectory_best_leapfrogs", "trajectory_run_leapfrogs",
               "trajectory_efficiency_vs_best")
TOP_KEYS = ("trajectory_leapfrogs_max", "trajectory_probe_trajectories", "trajectory_time_sec")
# what a sampling run of the parent commit writes into <method>.json besides the VI fit and the tuning runs
PLAIN_RUN_KEYS = {"ess_min", "sem_min", "mcmc_time_sec", "ess_estimator", "ess_min_batch_means", "sem_min_batch_means",
                  "batch_means_batch", "ess_constant_chains", "ess_chains", "split_rhat_max", "split_rhat_chains",
                  "rhat_max_all_chains", "diagnostics_time_sec"}
RUN_KEYS = {"CP": PLAIN_RUN_KEYS | {"acceptance_rate"},
            "i": PLAIN_RUN_KEYS | {"acceptance_rate_cp", "acceptance_rate_ncp", "num_leapfrog_steps", "initial_step_size_cp",
                                   "initial_step_size_ncp"}}


def _cli(args):
    from autoreparam_amd import flags as flags_mod
    from autoreparam_amd import main as cli
    return cli.main(args, flags=flags_mod.FlagValues())


def test_cli_trajectory_profile(gpu, tmp_path, capsys):
    """radon MN, --method=CP and --method=i at 256 chains with --trajectory_profile=6: the key sets, vectors of length 6, a
    best count in 1 ... 6, acceptances in (0, 1], the shapes of <method>_trajectory.npz, one analyze table per kernel; and
    the same runs without the flag, in a copy of the directory made before them: the parent's key set, no file."""
    from autoreparam_amd import analyze
    Cn, S, R, Lmax = 256, 120, 5, 6
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    common = ["--model=radon", "--dataset=MN", "--num_chains=%d" % Cn, "--seed=3", "--num_optimization_steps=400"]
    hm = ["--num_samples=%d" % S, "--num_burnin_steps=200", "--num_adaptation_steps=150"]
    for m in ("CP", "NCP"):
        _cli(common + ["--results_dir=" + on, "--inference=VI", "--method=" + m])
        _cli(common + ["--results_dir=" + on, "--inference=HMCtuning", "--method=" + m, "--num_leapfrog_steps=4"] + hm)
    shutil.copytree(on, off)
    for m in ("CP", "i"):
        _cli(common + ["--results_dir=" + on, "--inference=HMC", "--method=" + m, "--trajectory_profile=%d" % Lmax,
                       "--energy_probe_steps=%d" % R] + hm)
        _cli(common + ["--results_dir=" + off, "--inference=HMC", "--method=" + m] + hm)
    assert capsys.readouterr().out.count("expected squared jump per gradient is largest at") == 3
    sp = helpers.spec("radon_MN")
    for m, kernels in (("CP", 1), ("i", 2)):
        r = json.load(open(os.path.join(on, m + "_tied.json")))
        plain = json.load(open(os.path.join(off, m + "_tied.json")))
        fit = {"elbo", "variational_fit_time_secs", "actual_num_variational_steps", "estimated_elbo_std", "learning_rate",
               "initial_step_size", "learned_reparam", "learned_variational_params", "tuning_runs"}
        assert set(plain) - fit == RUN_KEYS[m], sorted(set(plain) ^ (RUN_KEYS[m] | fit))
        extra = set(TOP_KEYS) | (set(KERNEL_KEYS) if kernels == 1 else {"trajectory_by_kernel"})
        assert set(r) - set(plain) == extra and set(plain) <= set(r)
        assert not os.path.exists(os.path.join(off, m + "_tied_trajectory.npz"))
        assert not os.path.exists(os.path.join(on, m + "_tied_energy.npz"))
        assert all(len(r[k]) == 1 for k in extra)
        assert r["trajectory_leapfrogs_max"] == [Lmax] and r["trajectory_probe_trajectories"] == [(R + 1) * Cn * kernels]
        assert 0 <= r["trajectory_time_sec"][0] <= r["diagnostics_time_sec"][0]
        per_kernel = [{k: r[k][0] for k in KERNEL_KEYS}] if kernels == 1 else r["trajectory_by_kernel"][0]
        assert len(per_kernel) == kernels
        for d in per_kernel:
            assert set(d) == set(KERNEL_KEYS)
            for k in KERNEL_KEYS[:5]:
                assert len(d[k]) == Lmax and all(v is not None and np.isfinite(v) for v in d[k]), k
            assert 1 <= d["trajectory_best_leapfrogs"] <= Lmax and d["trajectory_run_leapfrogs"] == 4
            assert all(0.0 < v <= 1.0 for v in d["trajectory_accept_prob"])
            assert all(0.0 <= v <= 1.0 for v in d["trajectory_divergence_rate"])
            assert all(0 <= v < sp.D for v in d["trajectory_esjd_min_element"]) and all(v > 0 for v in d["trajectory_esjd_min"])
            assert 0.0 < d["trajectory_efficiency_vs_best"] <= 1.0
        z = np.load(os.path.join(on, m + "_tied_trajectory.npz"))
        assert list(z["leapfrogs"]) == list(range(1, Lmax + 1))
        want = {"leapfrogs"}
        for j in range(kernels):
            tag = "" if j == 0 else "_%d" % j
            want |= {"accept_prob" + tag, "divergence_rate" + tag}
            assert z["accept_prob" + tag].shape == (Lmax,) and z["divergence_rate" + tag].shape == (Lmax,)
            for name, shape in zip(sp.part_names, sp.part_shapes):
                want.add("esjd%s/%s" % (tag, name))
                assert z["esjd%s/%s" % (tag, name)].shape == (Lmax,) + tuple(shape)
                assert np.isfinite(z["esjd%s/%s" % (tag, name)]).all()
        assert set(z.files) == want
        assert sorted(np.load(os.path.join(on, m + "_tied_rhat.npz")).files) == sorted(np.load(os.path.join(off, m + "_tied_rhat.npz")).files)
    lines = analyze.report_trajectory(analyze.load(str(tmp_path), "on"), str(tmp_path), "on")
    assert len([l for l in lines if "trajectory profile over" in l]) == 3          # CP, and the two kernels of i
    assert len([l for l in lines if l.strip().startswith("leapfrogs")]) == 3
    assert analyze.report_trajectory(analyze.load(str(tmp_path), "off"), str(tmp_path), "off") == []
