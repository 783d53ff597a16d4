"""GPU: arp_sbc_fold against tests/sbc_ref.py at the smallest shapes at which it can go wrong.  A tile of the kernel holds
8 192 / (Q | 1) rows -- 31 at Q = 256, 32 at 255, 126 at 65 and 64, 744 at 11, 8 192 at 1 -- so n_draws = 257 crosses tiles
from Q = 64 up, and two more shapes cross them at Q = 11 and Q = 1; Q = 256 fills the workgroup, 255 and 65 leave a ragged
last wave.  Counts, left_out and n_left_out are exact; each sum is within n_draws 2^-53 sum |term| of the fsum value (the
bound of recursive summation in any order, not a measured tolerance); two calls are bitwise equal; padding is never read."""
import numpy as np
import pytest
import torch

import sbc_ref

pytestmark = pytest.mark.gpu

N_DRAWS = (1, 63, 64, 65, 257)
QS = (1, 11, 64, 65, 255, 256)
TILE_CROSSINGS = ((1489, 11), (8193, 1))         # (n_draws, Q): more than one tile where 257 rows are one


def make_case(n_rep, n_draws, Q, seed):
    """Draws over many magnitudes, with what compares badly: column 0 holds +-0 against a truth of +-0; column 1 (Q > 1)
    denormals against a denormal truth; column 2 (Q > 2) one value many times, equal to the truth in every other replicate;
    the other columns are rounded to one decimal, so draws repeat and some equal the truth."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n_rep, n_draws, Q)) * 10.0 ** rng.integers(-3, 4, size=(1, 1, Q))).astype(np.float32)
    t = (rng.standard_normal((n_rep, Q)) * 10.0 ** rng.integers(-3, 4, size=(1, Q))).astype(np.float32)
    x[:, :, 3::2] = np.round(x[:, :, 3::2], 1)
    t[:, 3::2] = np.round(t[:, 3::2], 1)
    x[:, :, 0] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), size=(n_rep, n_draws))
    t[:, 0] = np.array([0.0, -0.0, 0.0], np.float32)[:n_rep]
    if Q > 1:
        tiny = np.array([1e-40, -1e-40, 3e-45, -3e-45, 1.1e-38, 0.0], np.float32)
        x[:, :, 1] = rng.choice(tiny, size=(n_rep, n_draws))
        t[:, 1] = np.array([3e-45, -1e-40, 1e-40], np.float32)[:n_rep]
    if Q > 2:
        x[:, :, 2] = np.float32(2.5)
        x[:, ::3, 2] = np.float32(-7.25)
        t[:, 2] = np.array([2.5, 0.1, -7.25], np.float32)[:n_rep]
    return x, t


def fold(draws, truth):
    from autoreparam_amd import diagnostics
    counts, sums, left_out, n_left_out = diagnostics.sbc_fold(draws, truth)
    torch.cuda.synchronize()
    return counts.cpu().numpy(), sums.cpu().numpy(), left_out.cpu().numpy(), int(n_left_out.item())


def padded(x, t, gpu, fill):
    """The same values as an inner block of wider buffers whose padding holds `fill`"""
    n_rep, n_draws, Q = x.shape
    wide = torch.full((n_rep, n_draws + 2, Q + 3), fill, dtype=torch.float32, device=gpu)
    wide[:, :n_draws, :Q] = torch.as_tensor(x, device=gpu)
    wide_t = torch.full((n_rep, Q + 5), fill, dtype=torch.float32, device=gpu)
    wide_t[:, :Q] = torch.as_tensor(t, device=gpu)
    return wide[:, :n_draws, :Q], wide_t[:, :Q]


def check_against_reference(x, t, gpu):
    n_rep, n_draws, Q = x.shape
    ref = sbc_ref.fold(x, t)
    tight = fold(torch.as_tensor(x, device=gpu), torch.as_tensor(t, device=gpu))
    counts, sums, left_out, n_left_out = tight
    assert counts.dtype == np.int32 and sums.dtype == np.float64 and left_out.dtype == np.uint8
    assert np.array_equal(counts, ref["counts"]) and np.array_equal(left_out, ref["left_out"]) and n_left_out == ref["n_left_out"]
    err, bound = np.abs(sums - ref["sums"]), sbc_ref.sum_bound(n_draws, ref["abs_terms"])
    assert np.all(err <= bound), (float(np.max(err / np.where(bound > 0, bound, 1.0))), n_rep, n_draws, Q)
    # two calls, and the same values behind other strides: bitwise equal (the padding is NaN: a read of it would show)
    again = fold(torch.as_tensor(x, device=gpu), torch.as_tensor(t, device=gpu))
    wide = fold(*padded(x, t, gpu, float("nan")))
    raw = lambda v: np.atleast_1d(np.asarray(v)).view(np.uint8)
    for a, b, c in zip(tight, again, wide):
        assert np.array_equal(raw(a), raw(b)) and np.array_equal(raw(a), raw(c))
    return float(np.max(err / np.where(bound > 0, bound, np.inf)))


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("n_draws", N_DRAWS)
def test_against_the_reference(gpu, n_draws, Q):
    worst = max(check_against_reference(*make_case(n_rep, n_draws, Q, 100 * n_draws + Q + n_rep), gpu) for n_rep in (1, 3))
    print("n_draws %d, Q %d: largest sum error / bound %.3g" % (n_draws, Q, worst))


@pytest.mark.parametrize("n_draws,Q", TILE_CROSSINGS)
def test_tile_crossings_at_small_q(gpu, n_draws, Q):
    check_against_reference(*make_case(3, n_draws, Q, n_draws), gpu)


def test_replicates_left_out(gpu):
    """NaN or +-inf in a draw, in the last row's last column, in another thread's column, in the truth: the replicate is
    left out, its counts and sums are zeros (a product with a mask would have kept the NaN), its neighbours are untouched"""
    for n_draws, Q in ((65, 11), (257, 256), (1, 1)):
        x, t = make_case(3, n_draws, Q, 5)
        x, t = np.concatenate([x, x, x[:1]]), np.concatenate([t, t, t[:1]])             # 7 replicates
        x[1, n_draws // 2, Q // 2] = np.nan
        x[2, n_draws - 1, Q - 1] = np.inf
        t[4, Q - 1] = np.nan
        x[5, 0, 0] = -np.inf
        t[6, 0] = np.inf
        ref = sbc_ref.fold(x, t)
        assert ref["left_out"].tolist() == [0, 1, 1, 0, 1, 1, 1]
        for fill in (0.0, float("nan")):
            counts, sums, left_out, n_left_out = fold(*padded(x, t, gpu, fill))
            assert left_out.tolist() == [0, 1, 1, 0, 1, 1, 1] and n_left_out == 5
            assert not counts[left_out != 0].any() and np.array_equal(sums[left_out != 0], np.zeros((5, Q, 2)))
            assert np.array_equal(counts, ref["counts"])
            assert np.all(np.abs(sums - ref["sums"]) <= sbc_ref.sum_bound(n_draws, ref["abs_terms"]))


def test_every_refusal_launches_nothing(gpu):
    from autoreparam_amd import _lib, diagnostics
    L = _lib.lib()
    n_rep, n_draws, Q = 2, 5, 3
    x = torch.zeros(n_rep, n_draws, Q, dtype=torch.float32, device=gpu)
    t = torch.zeros(n_rep, Q, dtype=torch.float32, device=gpu)
    counts = torch.full((n_rep, Q, 2), -7, dtype=torch.int32, device=gpu)
    sums = torch.full((n_rep, Q, 2), -7.0, dtype=torch.float64, device=gpu)
    left_out = torch.full((n_rep,), 9, dtype=torch.uint8, device=gpu)
    n_left_out = torch.full((), -7, dtype=torch.int64, device=gpu)
    good = dict(draws=x, n_rep=n_rep, n_draws=n_draws, Q=Q, rep_stride=n_draws * Q, row_stride=Q, truth=t, truth_stride=Q,
                counts=counts, sums=sums, left_out=left_out, n_left_out=n_left_out)
    order = ("draws", "n_rep", "n_draws", "Q", "rep_stride", "row_stride", "truth", "truth_stride", "counts", "sums", "left_out",
             "n_left_out")

    def call(**change):
        a = dict(good, **change)
        args = [_lib.ptr(a[k]) if k in ("draws", "truth", "counts", "sums", "left_out", "n_left_out") else int(a[k]) for k in order]
        rc = L.arp_sbc_fold(*args, _lib.stream())
        return rc, L.arp_last_error().decode()
    cases = [(dict(draws=None), "are required"), (dict(truth=None), "are required"), (dict(counts=None), "are required"),
             (dict(sums=None), "are required"), (dict(left_out=None), "are required"), (dict(n_left_out=None), "are required"),
             (dict(Q=0), "1 <= Q <= 256"), (dict(Q=257, row_stride=257, truth_stride=257, rep_stride=5 * 257), "1 <= Q <= 256"),
             (dict(n_draws=0), "1 <= n_draws <= 2^24"), (dict(n_draws=(1 << 24) + 1, rep_stride=1 << 40), "1 <= n_draws <= 2^24"),
             (dict(n_rep=0), "1 <= n_rep <= 2^20"), (dict(n_rep=(1 << 20) + 1), "1 <= n_rep <= 2^20"),
             (dict(row_stride=Q - 1), "row_stride >= Q"), (dict(rep_stride=n_draws * Q - 1), "rep_stride >= n_draws * row_stride"),
             (dict(row_stride=Q + 1), "rep_stride >= n_draws * row_stride"), (dict(truth_stride=Q - 1), "truth_stride >= Q")]
    for change, message in cases:
        rc, text = call(**change)
        assert rc != 0 and text.startswith("arp_sbc_fold: ") and message in text, (change, text)
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((sums == -7.0).all()) and bool((left_out == 9).all()) and int(n_left_out.item()) == -7
    rc, _ = call()
    torch.cuda.synchronize()
    assert rc == 0 and int(n_left_out.item()) == 0 and bool((left_out == 0).all()) and bool((counts[:, :, 1] == n_draws).all())
    # the wrapper refuses the same, before any call
    for shape, message in (((2, 3, 257), "1 <= Q <= 256"), ((2, 0, 3), "1 <= L"), ((0, 3, 3), "1 <= N")):
        with pytest.raises(ValueError, match=message):
            diagnostics.sbc_fold(torch.zeros(shape, dtype=torch.float32, device=gpu),
                                 torch.zeros(shape[0], shape[2], dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError, match="truth must be"):
        diagnostics.sbc_fold(x, torch.zeros(n_rep, Q + 1, dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError, match="float32 draws"):
        diagnostics.sbc_fold(x.double(), t.double())
