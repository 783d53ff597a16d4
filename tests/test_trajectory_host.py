"""CPU: the host half of the trajectory-length profile -- diagnostics.profile_from_sums on hand-made sums, the flag,
main._convergence_report with and without --trajectory_profile on a stand-in engine, the ABI lists -- and the calibration
of tests/test_gpu_trajectory.py: a float32 numpy replay (tests/trajectory_ref.py) of every case the GPU test runs against
the float64 one, held to energy_ref's bars at every leapfrog count before the device is; and the agreement of the
Metropolis-weighted jump of fresh-momentum trajectories with the realised jump of the oracle sampler's next transition."""
import os
import re

import numpy as np
import pytest
import torch

import energy_ref as er
import helpers
import rhat_ref
import trajectory_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_KEYS = ("trajectory_accept_prob", "trajectory_divergence_rate", "trajectory_esjd_min", "trajectory_esjd_min_element",
               "trajectory_esjd_min_per_gradient", "trajectory_best_leapfrogs", "trajectory_run_leapfrogs",
               "trajectory_efficiency_vs_best")
TOP_KEYS = ("trajectory_leapfrogs_max", "trajectory_probe_trajectories", "trajectory_time_sec")


# ---------------------------------------------------------------------------
# 1. profile_from_sums
# ---------------------------------------------------------------------------
def _sums(rows, div, nonf, acc, left, J):
    J = np.asarray(J, np.float64)
    head = np.stack([np.broadcast_to(np.asarray(v, np.float64), (J.shape[0],)) for v in (rows, div, nonf, acc, left)], axis=1)
    return np.concatenate([head, J], axis=1)


def test_profile_from_sums_arithmetic_and_argmax():
    from autoreparam_amd import diagnostics
    # 10 rows, variances (2, 0.5, 4): esjd = J / (10 v)
    J = np.array([[4.0, 2.0, 8.0],       # l = 1: 0.2, 0.4, 0.2   -> min 0.2 (element 0), per gradient 0.2
                  [20.0, 2.0, 40.0],     # l = 2: 1.0, 0.4, 1.0   -> min 0.4 (element 1), per gradient 0.2: a tie with l = 1
                  [30.0, 2.5, 12.0]])    # l = 3: 1.5, 0.5, 0.3   -> min 0.3 (element 2), per gradient 0.1
    p = diagnostics.profile_from_sums(_sums(10, [0, 1, 2], [0, 0, 1], [9.0, 6.0, 3.0], [0, 0, 2], J), [2.0, 0.5, 4.0])
    assert isinstance(p, diagnostics.Profile)
    assert p._fields == ("leapfrogs", "rows", "divergent", "nonfinite", "left_out", "accept_prob", "divergence_rate", "esjd",
                         "esjd_min", "esjd_min_element", "per_gradient", "best_leapfrogs")
    assert list(p.leapfrogs) == [1, 2, 3] and list(p.rows) == [10, 10, 10]
    assert list(p.divergent) == [0, 1, 2] and list(p.nonfinite) == [0, 0, 1] and list(p.left_out) == [0, 0, 2]
    assert np.allclose(p.accept_prob, [0.9, 0.6, 0.3], rtol=1e-15) and np.allclose(p.divergence_rate, [0, 0.1, 0.2], rtol=1e-15)
    assert np.allclose(p.esjd, [[0.2, 0.4, 0.2], [1.0, 0.4, 1.0], [1.5, 0.5, 0.3]], rtol=1e-15)
    assert np.allclose(p.esjd_min, [0.2, 0.4, 0.3], rtol=1e-15) and list(p.esjd_min_element) == [0, 1, 2]
    assert np.allclose(p.per_gradient, [0.2, 0.2, 0.1], rtol=1e-15)
    assert p.per_gradient[0] == p.per_gradient[1] and p.best_leapfrogs == 1        # a tie goes to the smallest l
    # a later, strictly larger figure wins
    J2 = J.copy(); J2[2] = [90.0, 22.5, 180.0]                                      # l = 3: 4.5 each -> per gradient 1.5
    assert diagnostics.profile_from_sums(_sums(10, 0, 0, 5.0, 0, J2), [2.0, 0.5, 4.0]).best_leapfrogs == 3


def test_profile_from_sums_leaves_out_elements_without_a_variance():
    from autoreparam_amd import diagnostics
    J = np.array([[1.0, 1e-9, 3.0, 5.0, 0.5]])
    p = diagnostics.profile_from_sums(_sums(4, 0, 0, 4.0, 0, J), [1.0, 0.0, np.nan, -2.0, 1.0])
    assert p.esjd_min_element[0] == 4 and p.esjd_min[0] == 0.5 / 4 and p.best_leapfrogs == 1
    none = diagnostics.profile_from_sums(_sums(4, 0, 0, 4.0, 0, J), [0.0, 0.0, np.nan, -2.0, np.inf])
    assert np.isnan(none.esjd_min[0]) and none.esjd_min_element[0] == -1 and np.isnan(none.per_gradient[0])
    assert none.best_leapfrogs == 0


def test_profile_from_sums_of_nothing_is_nan():
    from autoreparam_amd import diagnostics
    z = diagnostics.profile_from_sums(np.zeros((3, 5 + 4)), np.ones(4))
    assert list(z.rows) == [0, 0, 0] and z.best_leapfrogs == 0
    for v in (z.accept_prob, z.divergence_rate, z.esjd_min, z.per_gradient, z.esjd):
        assert np.isnan(v).all()
    e = diagnostics.profile_from_sums(np.zeros((0, 5 + 4)), np.ones(4))
    assert e.best_leapfrogs == 0 and e.esjd.shape == (0, 4) and len(e.per_gradient) == 0
    w = diagnostics.profile_from_sums(np.zeros((2, 5 + 4)), np.ones(3))             # a variance of the wrong length
    assert w.best_leapfrogs == 0 and np.isnan(w.esjd_min).all()
    assert diagnostics.profile_from_sums(np.zeros(7), np.ones(3)).best_leapfrogs == 0
    assert diagnostics.profile_from_sums(torch.zeros(2, 6, dtype=torch.float64), torch.ones(1)).best_leapfrogs == 0


def test_jump_sums_add_over_a_split_of_the_rows():
    """The reference fold on random trajectories with planted bad rows: the sums of two parts of the rows add to the
    whole's, and the profiles agree."""
    from autoreparam_amd import diagnostics
    rs = np.random.RandomState(4)
    n, D, L = 101, 7, 3
    x0 = rs.randn(n, D).astype(np.float32)
    path = (x0[None] + rs.randn(L, n, D)).astype(np.float32)
    energy = rs.randn(L + 1, n, 2).astype(np.float32)
    energy[1, 5, 0] = np.nan
    energy[2, 40, 0] = -5000.0
    path[0, 9, 3] = np.nan
    whole = tr.jump_sums(x0, path, energy)
    parts = tr.jump_sums(x0[:37], path[:, :37], energy[:, :37]) + tr.jump_sums(x0[37:], path[:, 37:], energy[:, 37:])
    assert np.array_equal(whole[:, [0, 1, 2, 4]], parts[:, [0, 1, 2, 4]]) and np.allclose(whole, parts, rtol=1e-13, atol=1e-13)
    # (energy[l] and path[l - 1] belong to sums[l - 1])
    assert whole[0, 0] == n and whole[0, 1] == 1 and whole[0, 2] == 1 and whole[1, 1] == 1 and whole[1, 2] == 0
    assert whole[2, 1] == 0 and whole[1, 4] == 0
    assert whole[0, 4] == 1 and np.isfinite(whole).all()
    var = x0.astype(np.float64).var(axis=0)
    a, b = diagnostics.profile_from_sums(whole, var), diagnostics.profile_from_sums(parts, var)
    assert a.best_leapfrogs == b.best_leapfrogs and np.allclose(a.esjd, b.esjd, rtol=1e-12)


# ---------------------------------------------------------------------------
# 2. the flag
# ---------------------------------------------------------------------------
def test_flag_default_and_refusals():
    from autoreparam_amd.flags import FlagValues
    f = FlagValues()
    assert f.trajectory_profile == 0
    assert not f.parse(["--trajectory_profile=6"]) and f.trajectory_profile == 6
    for good in (0, 1, 256):
        f.parse(["--trajectory_profile=%d" % good])
        assert f.trajectory_profile == good
    for bad in ("-1", "257", "100000"):
        with pytest.raises(ValueError):
            FlagValues().parse(["--trajectory_profile=" + bad])
    with pytest.raises(ValueError):
        FlagValues().parse(["--trajectory_profile=many"])


# ---------------------------------------------------------------------------
# 3. _convergence_report on a stand-in engine
# ---------------------------------------------------------------------------
class _FakeEngine(object):
    """Stands in for engine.Engine on the host: the identity for transform; trajectory_sums scripts sums that depend on the
    kernel alone (kernel j's jump grows up to l = 2 + j and is flat afterwards: best leapfrog count 2 + j)."""

    def __init__(self, D):
        self.D, self.calls = D, []

    def transform(self, x, which=0, to_centered=True):
        return torch.as_tensor(x).clone()

    def energy_probe(self, *args, **kwargs):
        raise AssertionError("the energy probe was not asked for")

    def trajectory_sums(self, x, eps0, n_leapfrog_max, which=0, kappa=None, seed=0, row_offset=0, lanes=0, max_path_bytes=1 << 30):
        n = int(x.shape[0])
        assert kappa is not None and tuple(kappa.shape) == (n,)
        self.calls.append((which, int(n_leapfrog_max), int(row_offset), int(seed), n))
        l = np.arange(1, n_leapfrog_max + 1, dtype=np.float64)
        J = n * np.minimum(l, 2.0 + which)[:, None] ** 2 * (1.0 + np.arange(self.D))[None, :]
        s = np.concatenate([np.stack([np.full_like(l, n), 0 * l, 0 * l, 0.5 * n + 0 * l, 0 * l], axis=1), J], axis=1)
        return torch.as_tensor(s), torch.zeros(n_leapfrog_max + 1, n, 2)


class _BothProbesEngine(_FakeEngine):
    """_FakeEngine with an energy probe that records its call and reports trajectories without an energy error."""

    def __init__(self, D):
        super(_BothProbesEngine, self).__init__(D)
        self.energy_calls = []

    def energy_probe(self, x, eps0, n_leapfrog, which=0, kappa=None, seed=0, row_offset=0, lanes=0, want_p=False, want_q=False):
        n = int(x.shape[0])
        assert kappa is not None and tuple(kappa.shape) == (n,)
        self.energy_calls.append((which, int(n_leapfrog), int(row_offset), int(seed), n))
        return torch.zeros(n, 4)


def _report(monkeypatch, kernels, Lmax, S=6, Cn=4, run_leapfrogs=3, energy=False, engine=_FakeEngine):
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
    reduces = []

    def all_reduce_sum(value, device=None):
        reduces.append(np.asarray(value).size)
        return torch.as_tensor(np.asarray(value))
    monkeypatch.setattr(diagnostics, "split_moments", moments)
    monkeypatch.setattr(diagnostics, "fold", fold)
    monkeypatch.setattr(parallel, "all_reduce_sum", all_reduce_sum)
    eng = engine(D)
    kappa = torch.ones(Cn)
    ctx = inference.ProbeContext(eng, torch.as_tensor(x[-1]), 0, tuple(
        inference.ProbeKernel(j, np.full(D, 0.1, np.float32), run_leapfrogs + 5 * j, kappa) for j in range(kernels)))
    base = inference.KernelResults(inference.HmcInnerResults(None), 1.0, S, None, None, torch.as_tensor(x))
    kr = inference._with_probe(base, ctx)
    f = FlagValues()
    f.num_chains, f.seed, f.energy_probe_steps, f.trajectory_profile, f.energy_diagnostics = Cn, 4, 3, Lmax, energy
    keys, arrays = cli._convergence_report(kr, cfg, f, None)
    return keys, arrays, eng, cfg, (S, Cn, D), reduces


@pytest.mark.parametrize("kernels", [1, 2])
def test_both_probes_visit_the_same_rows(monkeypatch, kernels):
    """With --energy_diagnostics and --trajectory_profile both on, Engine.energy_probe and Engine.trajectory_sums see the
    same sequence of (which, row_offset, rows) -- the trajectory report's "the rows the energy report probes" -- and at every
    visit their seeds differ by the difference of the two reports' seed constants (so by the same amount within a kernel)."""
    keys, arrays, eng, _, (S, Cn, D), _ = _report(monkeypatch, kernels, 4, energy=True, engine=_BothProbesEngine)
    rows = lambda calls: [(c[0], c[2], c[4]) for c in calls]
    assert rows(eng.energy_calls) == rows(eng.calls)
    assert rows(eng.calls) == [(j, Cn * (S if s < 0 else s), Cn) for j in range(kernels) for s in (-1, 0, 2, 5)]
    apart = [(t[3] - e[3]) % (1 << 64) for e, t in zip(eng.energy_calls, eng.calls)]
    assert apart == [0x54524A50 - 0x454E5247] * len(eng.calls)
    assert keys["energy_probe_trajectories"] == keys["trajectory_probe_trajectories"] == kernels * 4 * Cn


@pytest.mark.parametrize("kernels", [1, 2])
def test_convergence_report_with_and_without_the_flag(monkeypatch, kernels, tmp_path):
    """Without --trajectory_profile no key, no array and no probe call; with it the key set of the issue (per kernel under
    `trajectory_by_kernel` for two), one all-reduce more, the energy report's row offsets with the probe's own seed, the
    per-kernel leapfrog counts, and <base>_trajectory.npz next to an unchanged <base>_rhat.npz."""
    from autoreparam_amd import main as cli
    off_keys, off_arrays, eng, _, _, off_reduces = _report(monkeypatch, kernels, 0)
    assert not eng.calls and not [k for k in off_keys if k.startswith("trajectory")]
    assert cli.TRAJECTORY_ARRAYS not in off_arrays and cli.ENERGY_ARRAYS not in off_arrays
    Lmax = 4
    keys, arrays, eng, cfg, (S, Cn, D), reduces = _report(monkeypatch, kernels, Lmax)
    extra = set(TOP_KEYS) | (set(KERNEL_KEYS) if kernels == 1 else {"trajectory_by_kernel"})
    assert set(keys) - set(off_keys) == extra and set(off_keys) <= set(keys)
    assert {k: v for k, v in arrays.items() if k != cli.TRAJECTORY_ARRAYS}.keys() == off_arrays.keys()
    assert len(reduces) == len(off_reduces) + 1 and reduces[-1] == kernels * Lmax * (5 + D)       # one all-reduce carries the sums
    steps = [-1, 0, 2, 5]                                            # 3 of 6 recorded steps, and the final state
    want_calls = [(j, Lmax, Cn * (S if s < 0 else s), Cn) for j in range(kernels) for s in steps]
    assert [(c[0], c[1], c[2], c[4]) for c in eng.calls] == want_calls
    seeds = sorted({c[3] for c in eng.calls})
    assert len(seeds) == kernels
    energy_seed = (4 * 0x9E3779B97F4A7C15 + 0x454E5247) & 0xFFFFFFFFFFFFFFFF
    assert not set(seeds) & {energy_seed, energy_seed + 1}           # a seed constant of its own
    rows = kernels * len(steps) * Cn
    assert keys["trajectory_leapfrogs_max"] == Lmax and keys["trajectory_probe_trajectories"] == rows
    assert 0 <= keys["trajectory_time_sec"] <= keys["diagnostics_time_sec"]
    per_kernel = [keys] if kernels == 1 else keys["trajectory_by_kernel"]
    assert len(per_kernel) == kernels
    for j, d in enumerate(per_kernel):
        assert (set(d) == set(KERNEL_KEYS)) if kernels == 2 else (set(KERNEL_KEYS) <= set(d))
        for k in KERNEL_KEYS[:5]:
            assert len(d[k]) == Lmax, k
        assert d["trajectory_accept_prob"] == [0.5] * Lmax and d["trajectory_divergence_rate"] == [0.0] * Lmax
        assert d["trajectory_best_leapfrogs"] == 2 + j and d["trajectory_run_leapfrogs"] == 3 + 5 * j
        assert len(set(d["trajectory_esjd_min_element"])) == 1 and 0 <= d["trajectory_esjd_min_element"][0] < D
        pg = d["trajectory_esjd_min_per_gradient"]
        assert all(abs(pg[l] - d["trajectory_esjd_min"][l] / (l + 1)) < 1e-15 for l in range(Lmax))
        if j == 0:
            assert abs(d["trajectory_efficiency_vs_best"] - pg[2] / pg[1]) < 1e-15 and d["trajectory_efficiency_vs_best"] < 1
        else:
            assert d["trajectory_efficiency_vs_best"] is None                      # the run's 8 leapfrogs exceed Lmax
    tj = arrays[cli.TRAJECTORY_ARRAYS]
    assert list(tj["leapfrogs"]) == [1, 2, 3, 4]
    want = {"leapfrogs"}
    for j in range(kernels):
        tag = "" if j == 0 else "_%d" % j
        want |= {"accept_prob" + tag, "divergence_rate" + tag}
        assert tj["accept_prob" + tag].shape == (Lmax,) and tj["divergence_rate" + tag].shape == (Lmax,)
        for name, shape in zip(cfg.model.part_names, cfg.model.part_shapes):
            want.add("esjd%s/%s" % (tag, name))
            assert tj["esjd%s/%s" % (tag, name)].shape == (Lmax,) + tuple(shape)
    assert set(tj) == want
    # the side files: _rhat.npz as without the flag, _trajectory.npz beside it, no _energy.npz
    cli._save_diagnostics(str(tmp_path / "m"), arrays)
    assert sorted(np.load(str(tmp_path / "m_rhat.npz")).files) == sorted(off_arrays)
    assert sorted(np.load(str(tmp_path / "m_trajectory.npz")).files) == sorted(tj)
    assert not os.path.exists(str(tmp_path / "m_energy.npz"))
    cli._save_diagnostics(str(tmp_path / "n"), off_arrays)
    assert os.path.exists(str(tmp_path / "n_rhat.npz")) and not os.path.exists(str(tmp_path / "n_trajectory.npz"))


def test_analyze_prints_one_table_per_kernel():
    from autoreparam_amd import analyze
    d = {"trajectory_accept_prob": [0.9, 0.8], "trajectory_divergence_rate": [0.0, None], "trajectory_esjd_min": [0.1, 0.3],
         "trajectory_esjd_min_element": [0, 2], "trajectory_esjd_min_per_gradient": [0.1, 0.15], "trajectory_best_leapfrogs": 2,
         "trajectory_run_leapfrogs": 4, "trajectory_efficiency_vs_best": None}
    top = {"trajectory_leapfrogs_max": [2], "trajectory_probe_trajectories": [64], "trajectory_time_sec": [0.01]}
    one = dict(top, **{k: [v] for k, v in d.items()})
    two = dict(top, trajectory_by_kernel=[[d, dict(d, trajectory_best_leapfrogs=1)]])
    lines = analyze.report_trajectory({"CP": one, "i": two, "NCP": {"ess_min": [1.0]}})
    assert len([l for l in lines if "trajectory profile over" in l]) == 3
    assert len([l for l in lines if "<-- best" in l]) == 3 and any(l.startswith("i kernel 1") for l in lines)
    assert analyze.report_trajectory({"NCP": {"ess_min": [1.0]}}) == []


# ---------------------------------------------------------------------------
# 4. the ABI lists
# ---------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_symbols():
    from autoreparam_amd import _lib
    text = open(os.path.join(ROOT, "include", "autoreparam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("arp_trajectory_probe", "arp_jump_sums", "arp_jump_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SYMBOLS, name
    assert "#define ARP_ABI_VERSION 2" in text
    # what the profile is and is not
    comment = " ".join(" ".join(re.findall(r"/\*.*?\*/", text, flags=re.S)).replace(" * ", " ").split())
    for phrase in ("NOT replays of the sampler's transitions", "a run at another count would adapt others",
                   "one-transition (lag-one) criterion, not an effective sample size"):
        assert phrase in comment, phrase
    kernel = " ".join(open(os.path.join(ROOT, "autoreparam_amd", "csrc", "trajectory_probe.h")).read().replace("//", " ").split())
    for phrase in ("NOT replays of the sampler's transitions", "a run at another count would adapt others",
                   "one-transition (lag-one) criterion, not an effective sample size"):
        assert phrase in kernel, phrase


# ---------------------------------------------------------------------------
# 5. calibration of the parity bars
# ---------------------------------------------------------------------------
_MODELS = []
for _m, _, _ in er.CASES:
    if _m not in _MODELS:
        _MODELS.append(_m)


@pytest.mark.parametrize("mname", _MODELS)
def test_float32_replay_path_stays_inside_the_bars(oracle_lib, mname):
    """Every case tests/test_gpu_trajectory.py runs for this model (parameterisations, row counts of all its lanes, Lmax 1
    and 5, step multipliers), momenta from numpy: the float32 numpy replay against the float64 one, inside every bar of
    energy_ref.bars at every l.  The largest deviation / tolerance per model: DESIGN.md section 5."""
    sp = helpers.spec(mname)
    orc = oracle_lib.OracleModel(sp)
    worst = {}
    for kind in er.KINDS:
        a, b = helpers.params(sp, kind)
        for n in sorted({n for m, lanes, _ in er.CASES if m == mname for n in er.row_counts(lanes, kind)}):
            x = helpers.states(sp, n, seed=n, scale=er.STATE_SCALE)
            eps = er.eps0(orc, sp, a, b, x, tr.frac(mname))
            p = np.random.RandomState(77 + n).randn(n, sp.D).astype(np.float32)
            for Lmax in tr.LEAPFROGS_MAX:
                for kap in (None, er.kappas(n, n)):
                    ref = tr.replay_path(orc, a, b, x, p, eps, kap, Lmax, np.float64)
                    got = tr.replay_path(orc, a, b, x, p, eps, kap, Lmax, np.float32)
                    assert all(np.isfinite(v).all() for v in ref)
                    for key, r in tr.ratios_by_step(got, ref, p).items():
                        worst[key] = max(worst.get(key, 0.0), r) if r == r else float("nan")
    print("float32 replay_path %s: deviation / tolerance %s" % (mname, {k: round(v, 4) for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_replay_path_ends_where_replay_ends(oracle_lib):
    """replay_path at l = Lmax is energy_ref.replay of Lmax steps, bit for bit in float64 (the same operations in the
    same order), for every Lmax up to 5."""
    sp = helpers.spec("radon_MA")
    orc = oracle_lib.OracleModel(sp)
    a, b = helpers.params(sp, "VIP")
    x = helpers.states(sp, 9, seed=1, scale=er.STATE_SCALE)
    eps = er.eps0(orc, sp, a, b, x, 0.05)
    p = np.random.RandomState(5).randn(9, sp.D).astype(np.float32)
    kap = er.kappas(9, 2)
    lp, ke, path = tr.replay_path(orc, a, b, x, p, eps, kap, 5)
    for L in range(1, 6):
        lp0, ke0, lp1, ke1, q1 = er.replay(orc, a, b, x, p, eps, kap, L)
        assert np.array_equal(lp0, lp[0]) and np.array_equal(ke0, ke[0])
        assert np.array_equal(lp1, lp[L]) and np.array_equal(ke1, ke[L]) and np.array_equal(q1, path[L - 1])


# ---------------------------------------------------------------------------
# 6. the weighted jump of probed trajectories against the sampler's realised jump, on the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mname,kind,frac", [("8schools", "NCP", 0.1), ("radon_MA", "CP", 0.5)])
def test_weighted_jump_agrees_with_the_oracle_sampler(oracle_lib, mname, kind, frac):
    """4 096 chains of the float32 oracle sampler, fixed step, L = 4, 300 transitions; from its states the float64 replay of
    one fresh-momentum trajectory per chain: alpha (x_4 - x_0)^2 in centred coordinates against the squared jump the
    sampler's next transition realised -- equal in expectation given the state (the Metropolis test accepts with probability
    alpha) -- within 5 sigma for every element and for the standardised total."""
    sp = helpers.spec(mname)
    orc = oracle_lib.OracleModel(sp)
    a, b = helpers.params(sp, kind)
    Cn, L = 4096, 4
    q0 = helpers.states(sp, Cn, seed=2, scale=0.1)
    eps = er.eps0(orc, sp, a, b, q0, frac)
    st = oracle_lib.new_state(q0, np.float32)
    orc.hmc_run(st, a, b, eps, L, 300, seed=9)
    q = st["q"].copy()
    p = np.random.RandomState(41).randn(Cn, sp.D)
    lp, ke, path = tr.replay_path(orc, a, b, q, p, eps, None, L, np.float64)
    alpha, divergent, _ = tr.alphas(np.stack([lp, ke], axis=2))
    assert not divergent.any()
    before = st["accept_count"].copy()
    orc.hmc_run(st, a, b, eps, L, 1, seed=9)
    rate = float((st["accept_count"] - before).mean())
    x0 = orc.transform(q, a, b, True)
    z, z_total = tr.sampler_pair(x0, orc.transform(st["q"], a, b, True), alpha[L - 1], orc.transform(path[L - 1], a, b, True))
    print("weighted jump vs oracle sampler %s %s: acceptance %.4f (probe %.4f), largest |z| %.2f, total z %.2f" % (
        mname, kind, rate, alpha[L - 1].mean(), np.abs(z).max(), z_total))
    assert 0.2 < rate < 0.999
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.0 and abs(z_total) <= 5.0
