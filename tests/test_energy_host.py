"""CPU: the host half of the energy probe -- diagnostics.energy_sums / energy_from_sums on hand-made trajectories, the
flags, main._convergence_report with and without --energy_diagnostics on a stand-in engine, the ABI lists -- and the
calibration of tests/test_gpu_energy.py's bars: a float32 numpy replay (tests/energy_ref.py) of every case the GPU test
runs, momenta from numpy, against the float64 replay, held to the same bars before the device is."""
import os
import re

import numpy as np
import pytest
import torch

import energy_ref as er
import helpers
import rhat_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENERGY_KEYS = ("divergence_rate", "divergent_trajectories", "energy_probe_trajectories", "energy_nonfinite",
               "energy_error_mean", "energy_error_sd", "energy_accept_prob", "energy_kinetic_share", "energy_time_sec")


def _out4(dh, lp0=None, ke0=None):
    """[N, 4] float32 trajectories with the given energy errors: lp1 = lp0 - dh, ke1 = ke0."""
    dh = np.asarray(dh, np.float64)
    lp0 = np.full(len(dh), -3.0) if lp0 is None else np.asarray(lp0, np.float64)
    ke0 = np.full(len(dh), 2.0) if ke0 is None else np.asarray(ke0, np.float64)
    return torch.as_tensor(np.stack([lp0, ke0, lp0 - dh, ke0], axis=1).astype(np.float32))


def test_energy_from_sums_on_hand_made_sums():
    from autoreparam_amd import diagnostics
    # 10 rows, 2 divergent of which 1 not finite; the other 8: sum dh = 4, sum dh^2 = 10; sum accept 6; E0: sum 50, sum^2 340
    e = diagnostics.energy_from_sums([10, 2, 1, 4.0, 10.0, 6.0, 50.0, 340.0, 20.0], D=6)
    assert isinstance(e, diagnostics.Energy)
    assert e._fields == ("divergence_rate", "divergent", "nonfinite", "rows", "error_mean", "error_sd", "accept_prob", "kinetic_share")
    assert (e.rows, e.divergent, e.nonfinite) == (10, 2, 1) and e.divergence_rate == 0.2
    assert e.error_mean == 0.5 and abs(e.error_sd - np.sqrt((10.0 - 16.0 / 8) / 7)) < 1e-15
    assert e.accept_prob == 0.6
    var_e0 = (340.0 - 2500.0 / 10) / 9
    assert abs(e.kinetic_share - 3.0 / var_e0) < 1e-15
    # nothing to divide by: NaN, never an exception
    z = diagnostics.energy_from_sums(np.zeros(9), D=3)
    assert z.rows == 0 and all(np.isnan(v) for v in (z.divergence_rate, z.error_mean, z.error_sd, z.accept_prob, z.kinetic_share))
    one = diagnostics.energy_from_sums([1, 1, 1, 0, 0, 0, 1.0, 1.0, 1.0], D=3)
    assert one.divergence_rate == 1.0 and np.isnan(one.error_mean) and np.isnan(one.kinetic_share)


def test_energy_sums_counts_divergent_and_nonfinite_rows():
    """One NaN, one +inf, one energy error of 1000.5 and one of 999.5 among ordinary rows: 3 divergent, 2 not finite, and
    the moments are those of the other rows."""
    from autoreparam_amd import diagnostics
    good = np.array([0.25, -0.5, 999.5, 0.0, 1.5])
    dh = np.concatenate([good[:2], [np.nan, np.inf, 1000.5], good[2:]])
    out = _out4(dh, lp0=np.linspace(-5.0, -1.0, len(dh)), ke0=np.linspace(1.0, 3.0, len(dh)))
    s = diagnostics.energy_sums(out)
    assert s.dtype == torch.float64 and tuple(s.shape) == (9,)
    s = s.numpy()
    o = out.numpy().astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = (o[:, 0] - o[:, 2]) + (o[:, 3] - o[:, 1])              # (the float32 rows' own energy errors)
    keep = np.isfinite(d) & ~(d > 1000.0)
    assert keep.sum() == 5 and np.allclose(d[keep], good, atol=1e-4)
    assert (s[0], s[1], s[2]) == (8, 3, 2)
    assert abs(s[3] - d[keep].sum()) < 1e-9 and abs(s[4] - (d[keep] ** 2).sum()) < 1e-6
    assert abs(s[5] - np.minimum(1.0, np.exp(-d[keep])).sum()) < 1e-12
    e0 = o[:, 1] - o[:, 0]
    assert abs(s[6] - e0.sum()) < 1e-9 and abs(s[7] - (e0 ** 2).sum()) < 1e-9 and abs(s[8] - o[:, 1].sum()) < 1e-9
    e = diagnostics.energy_from_sums(s, D=4)
    assert (e.divergent, e.nonfinite, e.rows) == (3, 2, 8) and e.divergence_rate == 3 / 8
    assert abs(e.error_mean - d[keep].mean()) < 1e-9 and abs(e.error_sd - d[keep].std(ddof=1)) < 1e-6
    assert abs(e.kinetic_share - 2.0 / e0.var(ddof=1)) < 1e-9
    # -inf is not finite either; a huge negative error is an acceptance, not a divergence
    s2 = diagnostics.energy_sums(_out4([-np.inf, -2000.0])).numpy()
    assert (s2[0], s2[1], s2[2], s2[5]) == (2, 1, 1, 1.0)


def test_energy_sums_add_over_ranks():
    from autoreparam_amd import diagnostics
    rs = np.random.RandomState(3)
    dh = rs.randn(101) * 0.7
    dh[[5, 40]] = np.nan
    dh[77] = 4000.0
    out = _out4(dh, lp0=rs.randn(101) * 3, ke0=rs.rand(101) * 5)
    whole = diagnostics.energy_sums(out).numpy()
    parts = diagnostics.energy_sums(out[:37]).numpy() + diagnostics.energy_sums(out[37:]).numpy()
    assert np.array_equal(whole[:3], parts[:3]) and np.allclose(whole, parts, rtol=1e-13, atol=1e-12)
    a, b = diagnostics.energy_from_sums(whole, 5), diagnostics.energy_from_sums(parts, 5)
    assert np.allclose(a, b, rtol=1e-12)
    with pytest.raises(ValueError):
        diagnostics.energy_sums(out[:, :3])


def test_flag_defaults():
    from autoreparam_amd.flags import FlagValues
    f = FlagValues()
    assert f.energy_diagnostics is False and f.energy_probe_steps == 8 and f.convergence_diagnostics is True
    rest = f.parse(["--energy_diagnostics", "--energy_probe_steps=3", "--model=radon"])
    assert f.energy_diagnostics is True and f.energy_probe_steps == 3 and not rest
    f.parse(["--noenergy_diagnostics"])
    assert f.energy_diagnostics is False


def test_probe_steps_are_evenly_spaced_with_both_ends():
    from autoreparam_amd import main as cli
    assert cli.probe_steps(100, 8) == sorted(set(cli.probe_steps(100, 8))) and len(cli.probe_steps(100, 8)) == 8
    assert cli.probe_steps(100, 8)[0] == 0 and cli.probe_steps(100, 8)[-1] == 99
    assert cli.probe_steps(5, 8) == [0, 1, 2, 3, 4] and cli.probe_steps(1, 8) == [0] and cli.probe_steps(0, 8) == []
    assert cli.probe_steps(10, 2) == [0, 9] and cli.probe_steps(10, 0) == []


class _FakeEngine(object):
    """Stands in for engine.Engine on the host: the identity for transform, scripted energy errors for energy_probe (row r
    of a call at row offset o gets the error of global row o + r; kernel 1's are shifted by one)."""

    def __init__(self, dh_of):
        self.dh_of, self.calls = dh_of, []

    def transform(self, x, which=0, to_centered=True):
        return torch.as_tensor(x).clone()

    def energy_probe(self, x, eps0, n_leapfrog, which=0, kappa=None, seed=0, row_offset=0, lanes=0, want_p=False, want_q=False):
        n = int(x.shape[0])
        assert kappa is not None and tuple(kappa.shape) == (n,)
        self.calls.append((which, int(n_leapfrog), int(row_offset), int(seed), n))
        return _out4(self.dh_of(which, np.arange(n) + row_offset))


def _report(monkeypatch, kernels, flags_on, S=6, Cn=4):
    from autoreparam_amd import diagnostics, inference, main as cli, models, parallel
    from autoreparam_amd.flags import FlagValues
    cfg = models.get_model_by_name("8schools", "")
    D = cfg.model.D
    x = np.random.RandomState(0).randn(S, Cn, D).astype(np.float32)

    def moments(trace, split=True):
        m, v = rhat_ref.moments(trace.numpy(), split)
        return torch.as_tensor(m), torch.as_tensor(v)

    def fold(mean, var):
        m, v = mean.reshape(-1, D).numpy().astype(np.float64), var.reshape(-1, D).numpy().astype(np.float64)
        ok = np.isfinite(v)
        z = lambda a: np.where(ok, a, 0.0).sum(axis=0)
        return torch.as_tensor(np.stack([ok.sum(axis=0) * 1.0, z(m), z(m * m), z(v), (ok & (v == 0)).sum(axis=0) * 1.0]))
    monkeypatch.setattr(diagnostics, "split_moments", moments)
    monkeypatch.setattr(diagnostics, "fold", fold)
    monkeypatch.setattr(parallel, "all_reduce_sum", lambda value, device=None: torch.as_tensor(np.asarray(value)))

    def dh_of(which, rows):      # divergent: global rows 1 (final state: offset S * num_chains) and every row that is 2 mod 9
        d = 0.01 * (rows % 7) - 0.02 + which
        return np.where(rows % 9 == 2, 2000.0, np.where(rows == S * Cn + 1, np.nan, d))
    eng = _FakeEngine(dh_of)
    kappa = torch.ones(Cn)
    ctx = inference.ProbeContext(eng, torch.as_tensor(x[-1]), 0, tuple(
        inference.ProbeKernel(j, np.full(D, 0.1, np.float32), 3 + j, kappa) for j in range(kernels)))
    base = inference.KernelResults(inference.HmcInnerResults(None), 1.0, S, None, None, torch.as_tensor(x))
    kr = inference._with_probe(base, ctx)
    assert kr._fields == base._fields and tuple(kr) == tuple(base) and kr.probe is ctx
    f = FlagValues()
    f.num_chains, f.seed, f.energy_probe_steps, f.energy_diagnostics = Cn, 4, 3, flags_on
    keys, arrays = cli._convergence_report(kr, cfg, f, None)
    return keys, arrays, eng, cfg, (S, Cn, D)


@pytest.mark.parametrize("kernels", [1, 2])
def test_convergence_report_with_and_without_the_flag(monkeypatch, kernels, tmp_path):
    """Without --energy_diagnostics no key, no array and no probe call; with it the ten keys (and `energy_by_kernel` for two
    kernels), the arrays of <base>_energy.npz, the row offsets and the per-kernel leapfrog counts."""
    from autoreparam_amd import main as cli
    off_keys, off_arrays, eng, _, _ = _report(monkeypatch, kernels, False)
    assert not eng.calls and not [k for k in off_keys if k.startswith(("energy", "diverg"))]
    assert cli.ENERGY_ARRAYS not in off_arrays
    keys, arrays, eng, cfg, (S, Cn, D) = _report(monkeypatch, kernels, True)
    extra = set(ENERGY_KEYS) | ({"energy_by_kernel"} if kernels == 2 else set())
    assert set(keys) - set(off_keys) == extra and set(off_keys) <= set(keys)
    assert {k: v for k, v in arrays.items() if k != cli.ENERGY_ARRAYS}.keys() == off_arrays.keys()
    steps = [-1, 0, 2, 5]                                            # 3 of 6 recorded steps, and the final state
    want_calls = [(j, 3 + j, Cn * (S if s < 0 else s), n) for j in range(kernels) for s in steps for n in [Cn]]
    assert [(c[0], c[1], c[2], c[4]) for c in eng.calls] == want_calls
    assert len({c[3] for c in eng.calls}) == kernels                 # one derived seed per kernel
    rows = np.concatenate([np.arange(Cn) + Cn * (S if s < 0 else s) for s in steps])
    div = int(((rows % 9 == 2) | (rows == S * Cn + 1)).sum())
    assert keys["energy_probe_trajectories"] == kernels * len(rows) and keys["divergent_trajectories"] == kernels * div
    assert keys["energy_nonfinite"] == kernels and keys["divergence_rate"] == div / len(rows)
    assert 0 < keys["energy_accept_prob"] < 1 and keys["energy_time_sec"] >= 0 and keys["diagnostics_time_sec"] >= keys["energy_time_sec"]
    if kernels == 2:
        two = keys["energy_by_kernel"]
        assert len(two) == 2 and all(d["divergent_trajectories"] == div for d in two)
        assert abs(two[1]["energy_error_mean"] - two[0]["energy_error_mean"] - 1.0) < 1e-6
    en = arrays[cli.ENERGY_ARRAYS]
    assert list(en["steps"]) == steps and en["energy_error"].shape == (len(steps), Cn) and en["energy_error"].dtype == np.float32
    assert ("energy_error_1" in en) == (kernels == 2)
    assert len(en["divergent_chain"]) == kernels * div == len(en["divergent_step"]) == len(en["divergent_kernel"])
    got = sorted(zip(en["divergent_kernel"], en["divergent_step"], en["divergent_chain"]))
    want = sorted((j, s, c) for j in range(kernels) for s in steps for c in range(Cn)
                  if (c + Cn * (S if s < 0 else s)) % 9 == 2 or c + Cn * (S if s < 0 else s) == S * Cn + 1)
    assert got == want
    for name, shape in zip(cfg.model.part_names, cfg.model.part_shapes):
        assert en["divergent_where/" + name].shape == (kernels * div,) + tuple(shape)
    # the side files: _rhat.npz without the energy arrays, _energy.npz with them
    cli._save_diagnostics(str(tmp_path / "m"), arrays)
    assert sorted(np.load(str(tmp_path / "m_rhat.npz")).files) == sorted(off_arrays)
    assert sorted(np.load(str(tmp_path / "m_energy.npz")).files) == sorted(en)
    cli._save_diagnostics(str(tmp_path / "n"), off_arrays)
    assert os.path.exists(str(tmp_path / "n_rhat.npz")) and not os.path.exists(str(tmp_path / "n_energy.npz"))


def test_header_declares_and_binding_lists_the_symbol():
    from autoreparam_amd import _lib
    text = open(os.path.join(ROOT, "include", "autoreparam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\barp_energy_probe\s*\(", src) and "arp_energy_probe" in _lib.SYMBOLS
    assert "#define ARP_ABI_VERSION 2" in text
    # what it is and is not, and what p_out depends on
    comment = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    assert "NOT a replay" in comment and "p_out depends on the lanes per chain" in " ".join(comment.split())


_MODELS = []
for _m, _, _ in er.CASES:
    if _m not in _MODELS:
        _MODELS.append(_m)


@pytest.mark.parametrize("mname", _MODELS)
def test_float32_replay_stays_inside_the_bars(oracle_lib, mname):
    """Every case tests/test_gpu_energy.py runs for this model (parameterisations, row counts of all its lanes, L, step
    multipliers), momenta from numpy: the float32 numpy replay against the float64 one, inside every bar the device is
    held to.  The largest deviation / tolerance per model: DESIGN.md section 5."""
    sp = helpers.spec(mname)
    orc = oracle_lib.OracleModel(sp)
    worst = {}
    for kind in er.KINDS:
        a, b = helpers.params(sp, kind)
        for n in sorted({n for m, lanes, _ in er.CASES if m == mname for n in er.row_counts(lanes, kind)}):
            x = helpers.states(sp, n, seed=n, scale=er.STATE_SCALE)
            eps = er.eps0(orc, sp, a, b, x, er.frac(mname))
            p = np.random.RandomState(77 + n).randn(n, sp.D).astype(np.float32)
            for L in er.LEAPFROGS:
                for kap in (None, er.kappas(n, n)):
                    ref = er.replay(orc, a, b, x, p, eps, kap, L, np.float64)
                    got = er.replay(orc, a, b, x, p, eps, kap, L, np.float32)
                    assert all(np.isfinite(v).all() for v in ref)
                    for key, r in er.ratios(got, ref, p).items():
                        worst[key] = max(worst.get(key, 0.0), r) if r == r else float("nan")
    print("float32 replay %s: deviation / tolerance %s" % (mname, {k: round(v, 4) for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), worst
