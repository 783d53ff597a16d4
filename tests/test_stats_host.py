"""CPU: the yardstick of the in-kernel statistics (tests/stats_ref.py) against inference.StreamingStats, and the two
float32 recurrences the kernels run -- restated in NumPy as the kernels have them -- against float64 on AR(1) series, at
the suite's small shape and at production batch lengths with a first sample far from the mean.  The last is what shows
without a GPU that the recurrences can meet the bars tests/test_gpu_stats.py holds the kernels to."""
import numpy as np
import pytest
import torch

import stats_ref


def _routes(launch_ends):
    return (("per-sample", stats_ref.per_sample_planes),
            ("fold", lambda x, b: stats_ref.welford_fold_planes(x, b, launch_ends)))


def _errors(x, batch, planes):
    """(mean error / scale, var error / scale^2, largest relative ESS error where the float64 ESS is finite, uncapped)"""
    from autoreparam_amd import engine
    S = x.shape[0]
    m64, v64, e64 = stats_ref.summary(x, batch)
    mean, var, ess = (t.numpy() for t in engine.stats_summary(torch.as_tensor(planes), S, batch))
    scale = np.abs(x.astype(np.float64)).max(axis=0) + 1
    ok = np.isfinite(e64) & (e64 < S)
    assert ok.mean() > 0.2
    return (np.abs(mean - m64) / scale).max(), (np.abs(var - v64) / scale ** 2).max(), (np.abs(ess - e64) / e64)[ok].max()


@pytest.mark.parametrize("S,batch,chunks", [(24, 4, (24,)), (26, 4, (5, 1, 13, 7)), (12, 1, (12,)), (40, 20, (19, 21))])
def test_float64_part_equals_streaming_stats(S, batch, chunks):
    from autoreparam_amd import inference
    x = stats_ref.ar1(S, 7, 5, 0.5, 1, seed=3, mean=-1.0, sd=2.0)
    mean, var, ess = stats_ref.summary(x, batch)
    ss = inference.StreamingStats(7, 5, batch, "cpu")
    r = 0
    for n in chunks:
        ss.update(torch.as_tensor(x[r:r + n])); r += n
    assert np.allclose(ss.mean().numpy(), mean, rtol=1e-12, atol=1e-12)
    assert np.allclose(ss.var().numpy(), var, rtol=1e-10, atol=1e-12)
    # StreamingStats keeps its batch means and its result in float32
    assert np.allclose(ss.ess().numpy(), ess, rtol=1e-5)
    # by hand: complete batches only, capped at n
    nb = S // batch
    bm = np.stack([x[k * batch:(k + 1) * batch].astype(np.float64).mean(axis=0) for k in range(nb)])
    assert np.allclose(ess, np.minimum(S * var / (batch * bm.var(axis=0, ddof=1)), S), rtol=1e-12)
    with pytest.raises(ValueError):
        stats_ref.summary(x[:2 * batch - 1], batch)


@pytest.mark.parametrize("rho,off", [(0.5, 0), (0.6, 3), (0.8, 10)])
def test_restated_planes_at_the_suite_shape(rho, off):
    """S = 24, batch 4, under the tolerances of the GPU tests: 2e-6 scale, 2e-6 scale^2, rtol 2e-3."""
    x = stats_ref.ar1(24, 16, 5, rho, off, seed=5, mean=0.5, sd=1.5)
    for name, fn in _routes((5, 6, 13)):
        em, ev, ee = _errors(x, 4, fn(x, 4))
        assert em < 2e-6 and ev < 2e-6 and ee < 2e-3, (name, em, ev, ee)


def test_planes_mean_what_the_header_says():
    """ref has moved to the mean of the first 4 batches (the last power of two); s1 / s2 / cur / sb1 / sb2 are about it;
    both routes agree."""
    S, batch = 27, 4
    x = stats_ref.ar1(S, 5, 3, 0.3, 6, seed=2)
    x64 = x.astype(np.float64)
    for name, fn in _routes((2, 9, 10, 20)):
        ref, s1, s2, cur, sb1, sb2 = fn(x, batch).astype(np.float64)
        assert np.allclose(ref, x64[:4 * batch].mean(axis=0), atol=1e-6), name
        d = x64 - ref
        nb = S // batch
        bm = d[:nb * batch].reshape(nb, batch, 5, 3).mean(axis=1)
        assert np.allclose(s1, d.sum(axis=0), atol=2e-5), name
        assert np.allclose(cur, d[:nb * batch].sum(axis=0), atol=2e-5), name
        assert np.allclose(s2, (d * d).sum(axis=0), rtol=2e-6), name
        assert np.allclose(sb1, bm.sum(axis=0), atol=1e-5), name
        assert np.allclose(sb2, (bm * bm).sum(axis=0), rtol=2e-5, atol=1e-6), name


def test_what_moving_ref_is_worth():
    """The recurrences as they were (ref stays the first sample) miss the ESS bar at production batch lengths once the
    first sample sits a few standard deviations out; with the move they meet it (the parametrised test below)."""
    S, batch = 16384, 2048
    x = stats_ref.ar1(S, 64, 2, 0.6, 10, seed=1, mean=2.0, sd=1.5)
    _, _, before = _errors(x, batch, stats_ref.per_sample_planes(x, batch, reref=False))
    _, _, after = _errors(x, batch, stats_ref.per_sample_planes(x, batch))
    print("ESS rel. error at 10 sd: %.2e without the move, %.2e with it" % (before, after))
    assert before > 2e-3 > 3 * after
    y = stats_ref.ar1(S, 64, 2, 0.995, 3, seed=1)
    for name, fn in _routes((5000, 5001, 11000)):
        em, ev, ee = _errors(y, 64, fn(y, 64))
        assert em < 1e-6 and ev < 1e-6 and ee < 2e-3, (name, em, ev, ee)


@pytest.mark.parametrize("off", [0, 3, 10])
@pytest.mark.parametrize("rho", [0.0, 0.6])
@pytest.mark.parametrize("batch", [2048, 64])
def test_restated_recurrences_meet_the_bars_at_production_batch_lengths(batch, rho, off):
    """S = 16 384, batch = S // 8 and 64, the first sample `off` standard deviations out: mean within 2e-6 (max|x| + 1),
    variance within 2e-6 (max|x| + 1)^2 on BOTH routes, batch-means ESS within rtol 2e-3 of float64."""
    S = 16384
    x = stats_ref.ar1(S, 64, 2, rho, off, seed=1, mean=2.0, sd=1.5)
    for name, fn in _routes((5000, 5001, 11000)):
        em, ev, ee = _errors(x, batch, fn(x, batch))
        print("%s batch %d rho %.1f off %d: mean %.2e scale, var %.2e scale^2, ESS rel %.2e" % (name, batch, rho, off, em, ev, ee))
        assert em < 2e-6 and ev < 2e-6 and ee < 2e-3, (name, em, ev, ee)
