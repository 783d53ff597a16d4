"""--superchain_size and nested R-hat on the host: the flag, the tie of the initial population, the float64 yardstick
(tests/nested_rhat_ref.py) against what is known about the statistic, the host arithmetic on the kernels' sums
(diagnostics.nested_rhat_from_sums) and main._nested_report with the device calls replaced by the yardstick."""
import types

import numpy as np
import pytest

import nested_rhat_ref as ref
import rhat_ref


def test_flag_parses_and_defaults_to_zero():
    from autoreparam_amd import flags as flags_mod
    f = flags_mod.FlagValues()
    assert f.superchain_size == 0
    rest = f.parse(["--superchain_size=64", "--model=radon"])
    assert f.superchain_size == 64 and f.model == "radon" and not rest


# ---- the tie

def _population(C, seed=0):
    rs = np.random.RandomState(seed)
    return [rs.randn(C).astype(np.float32), rs.randn(C, 3).astype(np.float32), rs.randn(C, 2, 2).astype(np.float32)]


def test_every_chain_takes_its_leaders_state():
    from autoreparam_amd import main
    parts = _population(12)
    for M, ws in ((2, 1), (3, 1), (4, 1), (6, 2), (3, 4)):
        tied = main.tie_superchains(parts, M, ws)
        assert len(tied) == len(parts)
        for p, t in zip(parts, tied):
            assert t.shape == p.shape and t.dtype == p.dtype
            for c in range(12):
                assert np.array_equal(t[c], p[(c // M) * M])
    assert all(np.array_equal(p, q) for p, q in zip(parts, _population(12)))          # the input is not written


def test_size_zero_returns_the_population_untouched():
    from autoreparam_amd import main
    parts = _population(12)
    assert main.tie_superchains(parts, 0) is parts
    assert main.tie_superchains(parts, 0, 8) is parts


@pytest.mark.parametrize("M,C,ws,what", [(1, 12, 1, "at least 2"), (-2, 12, 1, "at least 2"), (5, 12, 1, "divide"),
                                         (12, 12, 1, "at least two"), (3, 12, 8, "whole superchains"),
                                         (4, 12, 2, "whole superchains")])
def test_refusals(M, C, ws, what):
    from autoreparam_amd import main
    with pytest.raises(ValueError) as e:
        main.tie_superchains(_population(C), M, ws)
    assert what in str(e.value)
    with pytest.raises(ValueError):
        main.check_superchains(M, C, ws)


def test_initial_population_ties_and_refuses_before_drawing(monkeypatch):
    from autoreparam_amd import main, parallel, util
    config = types.SimpleNamespace(model=types.SimpleNamespace(part_names=["a", "b"]))
    fit = {"learned_variational_params": {"a_loc": [0.0, 1.0], "a_scale": [1.0, 2.0], "b_loc": 3.0, "b_scale": 0.5}}
    flags = types.SimpleNamespace(num_chains=12, seed=5, superchain_size=0)
    plain = main._initial_population(fit, config, flags)
    want = list(util.variational_inits_from_params(fit["learned_variational_params"], ["a", "b"], 12, seed=5).values())
    assert all(p.tobytes() == w.tobytes() for p, w in zip(plain, want))
    flags.superchain_size = 3
    tied = main._initial_population(fit, config, flags)
    for p, t in zip(plain, tied):
        assert all(np.array_equal(t[c], p[(c // 3) * 3]) for c in range(12))
    drawn = []
    monkeypatch.setattr(util, "variational_inits_from_params", lambda *a, **k: drawn.append(1))
    flags.superchain_size = 5
    with pytest.raises(ValueError):
        main._initial_population(fit, config, flags)
    monkeypatch.setattr(parallel, "world", lambda: (1, 8))                            # 12 chains, M = 3, 8 ranks
    flags.superchain_size = 3
    with pytest.raises(ValueError):
        main._initial_population(fit, config, flags)
    assert not drawn


# ---- the yardstick against what is known

def _formula(K, M):
    """The warning level of the issue, restated: (1 + 3 sqrt(2 / (K - 1))) / M + (1.01^2 - 1)."""
    return (1.0 + 3.0 * np.sqrt(2.0 / (K - 1.0))) / M + (1.01 ** 2 - 1.0)


def _level(K, M):
    """The level the command line warns at."""
    from autoreparam_amd import main
    return float(main.nested_warn_level(K, M))


def _nested(x, M):
    """The statistic as the project forms it (diagnostics.nested_rhat_from_sums) from the yardstick's float64 sums of the
    [S, C, D] draws x, after holding it to the yardstick's centred form (the columns here have means within a few sd of 0:
    the raw-sums bound is below 1e-12)."""
    from autoreparam_amd import diagnostics
    want = ref.nested(x, M)
    got = diagnostics.nested_rhat_from_sums(ref.sums(*ref.chain_moments(x), M))
    for a, b in zip(got, want):
        assert np.allclose(a, b, rtol=1e-10, atol=0, equal_nan=True)
    return got


def test_warning_level_is_the_issues_formula():
    from autoreparam_amd import main
    for K, M in ((2, 2), (8, 8), (10, 4), (64, 16), (16, 64), (512, 128), (1024, 64)):
        assert float(main.nested_warn_level(K, M)) == pytest.approx(_formula(K, M), rel=1e-15)
    lv = main.nested_warn_level(np.array([1.0, 0.0, 64.0]), 16)
    assert np.isnan(lv[:2]).all() and lv[2] == pytest.approx(_formula(64, 16), rel=1e-15)


def _draws(seed, K, M, S, D, offset_sd=0.0):
    rs = np.random.RandomState(seed)
    x = rs.randn(S, K * M, D)
    if offset_sd:
        x += np.repeat(offset_sd * rs.randn(K, D), M, axis=0)[None]
    return x


def test_stationary_excess_is_one_over_m():
    K, M, D = 64, 16, 64
    margin = 4.0 * np.sqrt(2.0 / ((K - 1) * D))
    assert abs(margin - 0.089) < 5e-4
    for S, want in ((1, 1.0 / M), (50, 1.0 / (M * 50 * (1.0 + 1.0 / 50)))):
        got = _nested(_draws(3, K, M, S, D), M)
        assert (got.superchains == K).all() and (got.left_out == 0).all()
        rel = got.excess.mean() / want - 1.0
        print("S = %d: mean B / W = %.6f, expected %.6f (%+.2f %%, allowed %.1f %%)" % (S, got.excess.mean(), want, 100 * rel,
                                                                                     100 * margin))
        assert abs(rel) <= margin
        assert np.allclose(got.rhat, np.sqrt(1.0 + got.between / got.within), rtol=1e-15)


@pytest.mark.parametrize("K,M,S", [(64, 16, 1), (64, 16, 50), (16, 64, 1), (8, 8, 4), (512, 128, 1)])
def test_warning_rule_is_silent_on_stationary_input(K, M, S):
    worst = 0.0
    for seed in range(100):
        got = _nested(_draws(seed, K, M, S, 5), M)
        worst = max(worst, float((got.excess / _level(K, M)).max()))
        assert (got.excess <= _level(K, M)).all(), seed
    print("(K, M, S) = (%d, %d, %d): largest B / W over 100 seeds is %.3f of the warning level" % (K, M, S, worst))


@pytest.mark.parametrize("K,M,S,sd", [(64, 16, 50, 0.5), (64, 64, 50, 0.3)])
def test_warning_rule_fires_on_superchain_offsets(K, M, S, sd):
    least = np.inf
    for seed in range(50):
        got = _nested(_draws(seed, K, M, S, 5, offset_sd=sd), M)
        least = min(least, float((got.excess / _level(K, M)).min()))
        assert (got.excess > _level(K, M)).all(), seed
    print("(K, M, S) = (%d, %d, %d), offsets of sd %.1f: smallest B / W over 50 seeds is %.2f x the warning level" % (
        K, M, S, sd, least))


def test_two_draws_per_chain_split_rhat_is_blind_nested_is_not():
    """S = 2: a half-chain is one draw and has no variance.  Offsets of sd 0.5 put B / W at (0.25 + 1 / (2 M)) / 1.5 = 0.17
    with a sampling sd of sqrt(2 / (K - 1)) = 9 % of itself at K = 256; the level at M = 64 is 0.040, eight sd below."""
    K, M, D = 256, 64, 5
    x = _draws(1, K, M, 2, D, offset_sd=0.5)
    assert np.isnan(rhat_ref.rhat(x, True)[0]).all()
    got = _nested(x, M)
    assert np.isfinite(got.rhat).all() and (got.excess > _level(K, M)).all()
    calm = _nested(_draws(1, K, M, 2, D), M)
    assert np.isfinite(calm.rhat).all() and (calm.excess <= _level(K, M)).all()


def test_left_out_superchains_and_degenerate_inputs():
    K, M, D = 6, 4, 3
    x = _draws(2, K, M, 5, D)
    y = x.copy()
    y[3, 1 * M + 2, 0] = np.nan                     # superchain 1, element 0
    y[0, 4 * M, 0] = np.inf                         # superchain 4, element 0
    got = _nested(y, M)
    assert got.superchains.tolist() == [4, 6, 6] and got.left_out.tolist() == [2, 0, 0]
    keep = [c for c in range(K * M) if c // M not in (1, 4)]
    alone = _nested(x[:, keep], M)
    assert np.allclose(got.rhat[0], alone.rhat[0], rtol=1e-12) and np.allclose(got.rhat[1:], _nested(x, M).rhat[1:], rtol=1e-12)
    assert np.isnan(_nested(np.ones((3, 8, 2)), 4).rhat).all()                   # W = 0
    assert np.isnan(_nested(x[:, :M], M).rhat).all()                            # one superchain
    one = _nested(x[:1], M)                                                      # one draw per chain
    assert np.isfinite(one.rhat).all() and np.allclose(one.rhat, ref.by_step(x, M)[0], rtol=1e-12)


# ---- the host arithmetic on the kernels' sums

def test_from_sums_agrees_with_the_yardstick():
    """Sums formed in float64 numpy -> diagnostics.nested_rhat_from_sums against the yardstick's centred form.  Tolerance:
    B = (sum g^2 - (sum g)^2 / K) / (K - 1) subtracts two numbers of size K gbar^2 (1 + ...), each a sum of K + 1 rounded
    terms: relative error of B <= ~ 2^-52 K gbar^2 / ((K - 1) B), allowed 8 x (the roundings of the K-term sums), plus
    1e-13 for the rest of the arithmetic -- 1e-10 for the column 100 sd away at K = 64, M = 8, S = 6."""
    from autoreparam_amd import diagnostics
    K, M, S, D = 64, 8, 6, 7
    x = _draws(4, K, M, S, D)
    x[:, :, 3] += 100.0
    x[:, :, 5] *= 1e-3
    x[2, 5 * M + 1, 6] = np.nan
    mean, var = ref.chain_moments(x)
    want = ref.from_moments(mean, var, M)
    got = diagnostics.nested_rhat_from_sums(ref.sums(mean, var, M))
    assert isinstance(got, diagnostics.NestedRhat) and got._fields == ("rhat", "excess", "between", "within", "superchains", "left_out")
    assert all(v.shape == (D,) and v.dtype == np.float64 for v in got)
    assert got.superchains.tolist() == [K] * 6 + [K - 1] and got.left_out.tolist() == [0] * 6 + [1]
    gbar = np.nanmean(np.where(np.isfinite(mean), mean, np.nan), axis=0)
    bound = 2.0 ** -52 * K * gbar ** 2 / ((K - 1) * want.between)
    tol = 8.0 * bound + 1e-13
    print("relative tolerance per column: %s" % tol)
    assert 5e-11 < tol[3] < 2e-9
    assert (np.abs(got.between / want.between - 1.0) <= tol).all()
    assert (np.abs(got.within / want.within - 1.0) <= 1e-13).all()
    assert (np.abs(got.excess / want.excess - 1.0) <= tol).all()
    assert (np.abs(got.rhat / want.rhat - 1.0) <= tol).all()
    # one draw per chain, and the profile
    step = diagnostics.nested_rhat_by_step(ref.step_sums(x, M))
    want_step = ref.by_step(x, M)
    assert step.shape == (S, D) and step.dtype == np.float64
    assert (np.abs(step / want_step - 1.0) <= 8.0 * 2.0 ** -52 * 101.0 ** 2 * M + 1e-13).all()      # (B ~ 1 / M here)
    # degenerate sums: NaN, never an error
    z = np.zeros((6, 2))
    assert np.isnan(diagnostics.nested_rhat_from_sums(z).rhat).all()
    z[0] = 1.0
    assert np.isnan(diagnostics.nested_rhat_from_sums(z).rhat).all()
    z[0], z[2] = 3.0, 1.0                                                           # W = 0
    assert np.isnan(diagnostics.nested_rhat_from_sums(z).rhat).all()


# ---- the report

class _Spec(object):
    part_names = ["a", "b"]

    @staticmethod
    def unpack(flat):
        return [flat[:1], flat[1:]]


def _by_part(arrays, rows):
    for key, flat in rows:
        for name, part in zip(_Spec.part_names, _Spec.unpack(flat)):
            arrays["%s/%s" % (key, name)] = part


def _report(monkeypatch, x, M, moments=None, reduce=None, fold=None, step=None):
    """main._nested_report on the float64 [S, C, D] numpy trace x with the device left out: the yardstick's sums stand in
    for the kernels (fold / step: other sums), `reduce` for parallel.all_reduce_sum.  Returns (keys, arrays, the values every
    all-reduce was given)."""
    import torch
    from autoreparam_amd import diagnostics, main, parallel
    sent = []

    def all_reduce(value, device=None):
        sent.append(np.array(value, np.float64))
        return torch.as_tensor(sent[-1] if reduce is None else reduce(len(sent) - 1, sent[-1]))

    def split_moments(trace, split=True):
        assert split is False
        mean, var = ref.chain_moments(trace.numpy())
        var = np.full_like(mean, np.nan) if var is None else var
        return torch.as_tensor(mean)[None], torch.as_tensor(var)[None]

    def nested_fold(mean, var, m):
        return torch.as_tensor(fold if fold is not None else ref.sums(mean.numpy(), None if var is None else var.numpy(), m))

    def nested_step_sums(trace, m):
        return torch.as_tensor(step if step is not None else ref.step_sums(trace.numpy(), m))

    monkeypatch.setattr(parallel, "all_reduce_sum", all_reduce)
    monkeypatch.setattr(diagnostics, "split_moments", split_moments)
    monkeypatch.setattr(diagnostics, "nested_fold", nested_fold)
    monkeypatch.setattr(diagnostics, "nested_step_sums", nested_step_sums)
    arrays = {}
    mom = None if moments is None else tuple(torch.as_tensor(v) for v in moments)
    keys = main._nested_report(torch.as_tensor(x), mom, M, None, arrays, _by_part)
    return keys, arrays, sent


KEYS = ("nested_rhat_max", "nested_rhat_superchains", "nested_rhat_superchain_size", "nested_rhat_chains", "nested_rhat_floor",
        "nested_rhat_left_out", "nested_rhat_first_step_max", "nested_rhat_last_step_max", "nested_rhat_time_sec")


def test_report_keys_and_arrays(monkeypatch, capsys):
    K, M, S, D = 6, 4, 5, 3
    x = _draws(7, K, M, S, D)
    x[1, 2 * M + 1, 2] = np.nan
    keys, arrays, _ = _report(monkeypatch, x, M)
    assert sorted(keys) == sorted(KEYS)
    want = ref.nested(x, M)
    steps = ref.by_step(x, M)
    assert keys["nested_rhat_max"] == pytest.approx(np.nanmax(want.rhat), rel=1e-12)
    assert keys["nested_rhat_superchains"] == K - 1 and keys["nested_rhat_left_out"] == 1
    assert keys["nested_rhat_superchain_size"] == M and keys["nested_rhat_chains"] == K * M
    assert keys["nested_rhat_floor"] == np.sqrt(1.0 + 1.0 / M)
    assert keys["nested_rhat_first_step_max"] == pytest.approx(steps[0].max(), rel=1e-12)
    assert keys["nested_rhat_last_step_max"] == pytest.approx(steps[-1].max(), rel=1e-12)
    assert keys["nested_rhat_time_sec"] >= 0
    assert sorted(arrays) == ["nested_rhat/a", "nested_rhat/b", "nested_rhat_by_step", "nested_rhat_by_step_element"]
    assert np.allclose(np.concatenate([arrays["nested_rhat/a"], arrays["nested_rhat/b"]]), want.rhat, rtol=1e-12)
    assert arrays["nested_rhat_by_step"].shape == (S,) and arrays["nested_rhat_by_step_element"].shape == (S,)
    assert np.allclose(arrays["nested_rhat_by_step"], np.nanmax(steps, axis=1), rtol=1e-12)
    assert np.array_equal(arrays["nested_rhat_by_step_element"], np.nanargmax(steps, axis=1))
    assert "nested R-hat over 5 superchains of 4" in capsys.readouterr().out


def test_report_one_draw_per_chain_passes_no_variance(monkeypatch):
    x = _draws(8, 5, 3, 1, 2)
    keys, arrays, _ = _report(monkeypatch, x, 3)                  # (the stand-in's var is NaN: it must not be read)
    assert keys["nested_rhat_max"] == pytest.approx(ref.nested(x, 3).rhat.max(), rel=1e-12)
    assert keys["nested_rhat_first_step_max"] == keys["nested_rhat_last_step_max"] == pytest.approx(keys["nested_rhat_max"], rel=1e-12)


def test_report_profile_is_null_with_fewer_than_two_kept_superchains(monkeypatch, capsys):
    """A streaming run: the statistic of all chains from the in-kernel moments, the profile from the kept trace."""
    K, M, S, D = 6, 4, 5, 3
    x = _draws(9, K, M, S, D)
    moments = ref.chain_moments(x)
    keys, arrays, _ = _report(monkeypatch, x[:, :M + 3], M, moments=moments)      # one whole superchain kept
    assert keys["nested_rhat_first_step_max"] is None and keys["nested_rhat_last_step_max"] is None
    assert keys["nested_rhat_chains"] == K * M and keys["nested_rhat_superchains"] == K
    assert keys["nested_rhat_max"] == pytest.approx(ref.nested(x, M).rhat.max(), rel=1e-12)
    assert sorted(arrays) == ["nested_rhat/a", "nested_rhat/b"]
    assert "fewer than two" in capsys.readouterr().out
    keys, arrays, _ = _report(monkeypatch, x[:, :2 * M + 3], M, moments=moments)  # two: chains [0, 2 M) of the kept trace
    assert keys["nested_rhat_first_step_max"] == pytest.approx(ref.by_step(x[:, :2 * M], M)[0].max(), rel=1e-12)
    assert "nested_rhat_by_step" in arrays


def test_report_warns_once_above_the_level_and_not_just_below(monkeypatch, capsys):
    from autoreparam_amd import main
    K, M, S, D = 10, 4, 2, 3
    level = _formula(K, M)
    assert float(main.nested_warn_level(K, M)) == pytest.approx(level, rel=1e-15)
    x = np.zeros((S, K * M, D))

    def fold_sums(excess):                                        # W = 1, gbar = 0: B = sum g^2 / (K - 1)
        f = np.zeros((6, D))
        f[0], f[3] = K, K
        f[2, 1] = excess * (K - 1)
        return f

    def step_sums(excess):
        s = np.zeros((4, S, D))
        s[0], s[3] = K, K
        s[2, 0, 2] = excess * (K - 1)
        return s

    for fold, step, n in ((level * (1 + 1e-9), 0.0, 1), (level * (1 - 1e-9), 0.0, 0), (0.0, level * (1 + 1e-9), 1),
                          (0.0, level * (1 - 1e-9), 0), (10 * level, 10 * level, 1)):
        keys, _, _ = _report(monkeypatch, x, M, fold=fold_sums(fold), step=step_sums(step))
        out = capsys.readouterr().out
        assert out.count("WARNING") == n, (fold, step, out)
        assert keys["nested_rhat_max"] == pytest.approx(np.sqrt(1.0 + fold), rel=1e-12)
        assert keys["nested_rhat_first_step_max"] == pytest.approx(np.sqrt(1.0 + step), rel=1e-12)
    # later steps do not warn by themselves: the profile is there to be read
    s = step_sums(0.0)
    s[2, 1, 0] = 10 * level * (K - 1)
    _report(monkeypatch, x, M, fold=fold_sums(0.0), step=s)
    assert "WARNING" not in capsys.readouterr().out


def test_two_half_jobs_add_up_to_the_whole_job(monkeypatch):
    """World size 2: every rank folds its own whole superchains, one all-reduce per set of sums."""
    K, M, S, D = 8, 3, 4, 3
    x = _draws(10, K, M, S, D, offset_sd=0.4)
    x[2, 5 * M, 1] = np.inf
    half = K // 2 * M
    whole_keys, whole_arrays, whole_sent = _report(monkeypatch, x, M)
    _, _, a = _report(monkeypatch, x[:, :half], M)
    _, _, b = _report(monkeypatch, x[:, half:], M)
    assert len(whole_sent) == len(a) == len(b) == 2
    for w, u, v in zip(whole_sent, a, b):
        assert np.allclose(u + v, w, rtol=1e-13, atol=1e-13)
    for mine, other in ((x[:, :half], b), (x[:, half:], a)):
        keys, arrays, _ = _report(monkeypatch, mine, M, reduce=lambda i, v, other=other: v + other[i])
        for k in KEYS[:-1]:
            assert keys[k] == pytest.approx(whole_keys[k], rel=1e-12), k
        assert keys["nested_rhat_chains"] == K * M and keys["nested_rhat_left_out"] == 1
        for k in whole_arrays:
            assert np.allclose(arrays[k], whole_arrays[k], rtol=1e-12), k
