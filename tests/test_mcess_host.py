"""--bulk_tail_ess on the host: the flag, and the float64 yardstick of the multi-chain ESS (tests/mcess_ref.py) against
what is known about it -- the asymptotic ESS of AR(1) chains, and the case the per-chain ESS cannot see."""
import numpy as np

import mcess_ref
from oracle import ess_ref


def test_flag_parses_and_defaults_off():
    from autoreparam_amd import flags as flags_mod
    f = flags_mod.FlagValues()
    assert f.bulk_tail_ess is False
    rest = f.parse(["--bulk_tail_ess", "--model=radon"])
    assert f.bulk_tail_ess is True and f.model == "radon" and not rest
    g = flags_mod.FlagValues()
    g.parse(["--nobulk_tail_ess"])
    assert g.bulk_tail_ess is False


RHOS = (0.0, 0.3, 0.6, 0.9, -0.4)


def test_yardstick_on_ar1_is_the_asymptotic_ess():
    """ESS / N = (1 - rho) / (1 + rho) within a factor [0.8, 1.25] on 64 chains of 1 000 draws."""
    x = ess_ref.ar1(1000, (64, 5), np.asarray(RHOS), seed=7)
    N = 1000 * 64
    for d, rho in enumerate(RHOS):
        got = mcess_ref.ess_one(x[:, :, d], split=True)
        ratio = got.ess / (N * (1 - rho) / (1 + rho))
        print("rho %.1f: ESS %.0f, ratio to the asymptotic value %.3f, cut at lag %d" % (rho, got.ess, ratio, got.max_t))
        assert 0.8 <= ratio <= 1.25


def test_yardstick_sees_chain_offsets_the_per_chain_ess_cannot():
    """White noise about chain offsets of sd 3: every chain alone looks perfect, the pooled sequence does not."""
    rs = np.random.RandomState(11)
    S, Cn = 400, 16
    x = rs.randn(S, Cn, 1) + 3.0 * rs.randn(1, Cn, 1)
    N = S * Cn
    got = mcess_ref.ess_one(x[:, :, 0], split=True)
    per_chain = ess_ref.ess_fft(x)[:, 0].sum()
    print("multi-chain ESS of the mean %.1f of N = %d; per-chain ESS summed %.0f" % (got.ess, N, per_chain))
    assert got.ess < 0.05 * N
    assert per_chain > 0.5 * N


def test_yardstick_degenerate_rows():
    assert np.isnan(mcess_ref.ess_one(np.ones((64, 4))).ess)
    for S in (1, 2, 3, 7):
        assert np.isnan(mcess_ref.ess_one(np.random.RandomState(0).randn(S, 3), split=True).ess)
    assert np.isfinite(mcess_ref.ess_one(np.random.RandomState(0).randn(7, 3), split=False).ess)


def _report(monkeypatch, world, result=None, k=4):
    """main._bulk_tail_report with the device left out: `world` for parallel.world, `result` for bulk_tail_ess."""
    from autoreparam_amd import diagnostics, main, parallel
    calls = []
    monkeypatch.setattr(parallel, "world", lambda: world)
    monkeypatch.setattr(main, "_bulk_tail_fit_chains", lambda trace, k: k)

    def fake(trace):
        calls.append(trace)
        return result
    monkeypatch.setattr(diagnostics, "bulk_tail_ess", fake)

    class Trace(object):                                     # (only sliced)
        def __getitem__(self, key):
            return ("slice", key)
    arrays = {}
    keys = main._bulk_tail_report(Trace(), k, None, arrays, lambda a, rows: a.update({key: v for key, v in rows}))
    return keys, arrays, calls


def test_sharded_job_writes_nulls_says_so_once_and_computes_nothing(monkeypatch, capsys):
    keys, arrays, calls = _report(monkeypatch, (0, 2))
    assert keys == {"ess_bulk_min": None, "ess_tail_min": None, "ess_mean_min": None, "mcse_mean_over_sd_max": None,
                    "bulk_tail_ess_chains": 0, "bulk_tail_ess_time_sec": None}
    assert not arrays and not calls
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "sharded" in out and "skipped" in out


def test_warning_below_100_per_chain_and_not_above(monkeypatch, capsys):
    from autoreparam_amd import diagnostics
    k = 4
    sd = np.array([1.0, 2.0, 1.0])

    def result(bulk, tail):
        mean = np.array([500.0, 400.0, np.nan])
        return diagnostics.BulkTailEss(np.asarray(bulk), np.asarray(tail), mean, sd / np.sqrt(mean), sd)
    keys, arrays, calls = _report(monkeypatch, (0, 1), result([450.0, 399.0, np.nan], [900.0, 800.0, np.nan]), k)
    out = capsys.readouterr().out
    assert out.count("WARNING") == 1 and "100 per chain" in out          # 399 < 100 x 4
    assert keys["ess_bulk_min"] == 399.0 and keys["ess_tail_min"] == 800.0 and keys["ess_mean_min"] == 400.0
    assert keys["mcse_mean_over_sd_max"] == 1.0 / np.sqrt(400.0) and keys["bulk_tail_ess_chains"] == k
    assert len(calls) == 1 and sorted(arrays) == ["ess_bulk", "ess_mean", "ess_tail", "mcse_mean"]
    _report(monkeypatch, (0, 1), result([450.0, 400.0, np.nan], [900.0, 400.0, np.nan]), k)
    assert "WARNING" not in capsys.readouterr().out                      # exactly 100 per chain is enough
    keys, _, _ = _report(monkeypatch, (0, 1), result([np.nan] * 3, [np.nan] * 3), k)
    assert "WARNING" not in capsys.readouterr().out and keys["ess_bulk_min"] is None
