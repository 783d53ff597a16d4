"""GPU: arp_psis_loo (csrc/psis.hip) against the float64 definition tests/psis_ref.py where tests/test_gpu_psis.py does
not go -- that file's tails end at M = 794, its rows are all <= 0 and of magnitude one, and its masks always keep most
draws.  Here (rows and references: tests/psis_cases.py, shared with tests/test_gpu_psis_weights_shapes.py):
  tail lengths   M a power of two and one more, 64 ... 4 097 (the bitonic network's padded length p2 up to 8 192), M =
                 3 072 (2^20 draws, the most --vi_check_draws takes) and M = 12 288 (2^24 draws, the API's limit: 48 KiB
                 of dynamic LDS);
  signs          positive rows, rows that straddle zero, the cut-off AT zero and at the smallest positive value (the
                 radix select's top byte changes sides there), offsets of +-1e4 and +-700;
  magnitudes     float32 subnormals, a row whose exp(cutoff) underflows, a row of +-1.5e38;
  an exact shift a row on a grid of 2^-10 plus 1 024, 8 192, -8 192: llmin - ll is the same bits, so k, sigma, cutoff and
                 tail_len must be the same BITS, and elpd_loo and lppd move by the shift;
  masks          every draw masked (R' = 0), and 1, 2, 4, 24, 25 kept draws of 70 001.
tail_len, cutoff and draws_used EQUAL; lppd and p_waic within psis.hip's header bounds; pareto_k, gpd_sigma and elpd_loo
within 16 x the largest deviation measured over these very cases on an MI355X, per class of tail length (MEASURED
below); each recorded figure must itself stay below M^2 2^-53, what float64 predicts at the class's largest M.  On a
row with an offset elpd_loo gets 8 2^-53 max|ll| on top: both sides form lw + ll and add a shift of the size of max|ll|
back, a few roundings each at that magnitude (largest multiple measured: OFFSET_MEASURED below).

Every case first asserts on the CPU, from the reference, that it is what it says (psis_cases.check_claims): M, p2,
the sign of the cut-off value, the kept count, fitted or not."""
import numpy as np
import pytest

import psis_cases as pcs
import psis_checks as pc
import psis_ref as pr

pytestmark = pytest.mark.gpu

# class (the largest M in it) -> largest |k - k_ref|, |sigma - sigma_ref| / |sigma_ref|, |elpd_loo - ref| (rows without
# an offset) over every case of this file, measured on an MI355X; the tests allow 16 x these.  Where each occurred:
#   M <= 1 025   k and elpd_loo at R = 116 508, M = 1 024; sigma at 25 kept draws of 70 001, M = 5 (1.8e-14 at M = 1 024)
#   M <= 4 097   all three at R = 1 864 136, M = 4 097 (at M = 3 072: 1.25e-14, 1.23e-14, 6.66e-14)
#   M = 12 288   R = 2^24; elpd_loo there is a log-sum-exp over 1.7e7 terms
# Float64 predicts up to M^2 2^-53 = 1.2e-10, 1.9e-9 and 1.7e-8: the figures grow far more slowly than that, and a
# float32 step would leave 1e-8 or more.
MEASURED = {
    1025: (1.78e-14, 2.43e-14, 9.15e-14),
    4097: (3.06e-14, 3.04e-14, 1.01e-13),
    12288: (2.32e-14, 2.37e-14, 1.12e-12),
}
# largest |elpd_loo - ref| on a row with an offset, in units of 2^-53 max|ll|, measured on an MI355X (VI-like rows, M =
# 513, 3 072 and 4 096: one unit in the last place of an elpd_loo of about 700); 8 are allowed
OFFSET_MULTIPLE, OFFSET_MEASURED = 8.0, 1.41


def klass(M):
    return min(c for c in MEASURED if M <= c)


def check(gpu, case, pad):
    """One call of psis_loo on the case's rows (NaN under its mask) against its references; prints the record."""
    M = int(case.ref8[:, 4].max())
    got = pc.device(gpu, case.poisoned, case.mask, pad=pad)
    worst = pc.compare(got, case.ref8, case.ll, case.mask, (case.what, case.names), MEASURED[klass(M)], case.offset, OFFSET_MULTIPLE)
    print("psis_loo %s: M %d (class %d): largest deviation k %.3g, sigma (relative) %.3g, elpd_loo %.3g, with an offset %.3g x 2^-53 max|ll|"
          % (case.what, M, klass(M), worst[0], worst[1], worst[2], worst[3]))
    return got


def test_recorded_figures_are_below_the_float64_prediction():
    for M, figures in MEASURED.items():
        assert all(0.0 < f < M * M * 2.0 ** -53 for f in figures), (M, figures)
    assert OFFSET_MEASURED <= OFFSET_MULTIPLE


@pytest.mark.parametrize("R", pcs.SMALL_RS)
def test_table_rows_of_every_sign_and_magnitude(gpu, R):
    """Every kind of row at R = 300, 4 097 and where M crosses 64 ... 1 024 (p2 up to 2 048)."""
    case = pcs.table_case(R)
    M = pcs.TABLE.get(R, pr.tail_len(R))
    pcs.check_claims(case, M)
    if R == 116509:
        assert pcs.p2_of(M) == 2048                                # the network past anything test_gpu_psis.py sorts
    check(gpu, case, pad=13)


@pytest.mark.parametrize("R", pcs.LARGE_RS)
def test_long_tails(gpu, R):
    """M = 2 048 ... 4 097: p2 = 2 048, 4 096 and 8 192; three rows of different content in one call."""
    case = pcs.large_case(R)
    pcs.check_claims(case, pcs.TABLE[R])
    assert pcs.p2_of(pcs.TABLE[R]) >= 2048 and all(case.fitted)
    check(gpu, case, pad=3)


def test_long_tail_with_a_tenth_masked(gpu):
    case = pcs.large_case(466034, True)
    pcs.check_claims(case)
    assert 1024 < case.ref8[0, 4] < 2048 and 0 < case.mask.sum() < 466034 // 8
    check(gpu, case, pad=5)


def test_the_limit_of_2_to_the_24_draws(gpu):
    """One row at the API's limit: M = 12 288, 140 profile points, 48 KiB of dynamic LDS.  The time is the reference's."""
    case = pcs.limit_case()
    pcs.check_claims(case, 12288)
    assert np.unique(case.ll[0, :1 << 16]).size < 1 << 13          # ties are plentiful
    check(gpu, case, pad=0)


@pytest.mark.parametrize("R", (4097, 29128))
def test_an_exact_shift_changes_no_bit_of_the_fit(gpu, R):
    case = pcs.shift_case(R)
    pcs.check_claims(case)
    base = case.ll[0].astype(np.float64)
    for n, c in enumerate(pcs.SHIFTS, 1):
        assert np.array_equal(case.ll[n].astype(np.float64), base + c)                 # the shift was exact
        assert (c > 0 and case.ll[n].min() > 0) or (c < 0 and case.ll[n].max() < 0)
    got = check(gpu, case, pad=7)
    bits = got.view(np.uint64)
    Rk = float(R)
    for n, c in enumerate(pcs.SHIFTS, 1):
        assert np.array_equal(bits[n, [1, 4, 5, 6, 7]], bits[0, [1, 4, 5, 6, 7]]), (c, got[n], got[0])
        big = np.abs(case.ll[n]).max() + np.abs(case.ll[0]).max()
        assert abs((got[n, 0] - got[0, 0]) - c) <= OFFSET_MULTIPLE * pc.U53 * big, (c, "elpd_loo", got[n, 0], got[0, 0])
        # the true lppd moves by c exactly; each side is within the header's bound of its own
        assert abs((got[n, 2] - got[0, 2]) - c) <= 2 * (Rk + 32) * pc.U53 + 4 * pc.U53 * big, (c, "lppd", got[n, 2], got[0, 2])


@pytest.mark.parametrize("R", (1, 300, 70001))
def test_every_draw_masked(gpu, R):
    """R' = 0 in both rows of a call (the mask is per draw); then, on the SAME workspace, the same rows with a tenth masked."""
    empty, tenth = pcs.pair_cases(R)
    pcs.check_claims(empty)
    pcs.check_claims(tenth)
    assert empty.ref8[0, 7] == 0 and np.all(empty.mask != 0) and np.isnan(empty.poisoned).all() and tenth.ref8[0, 7] > 0
    for n in range(2):
        assert np.array_equal(empty.ref8[n], np.array(pcs.EMPTY), equal_nan=True)
    ws = pc.api_workspace(gpu, 2, R)
    got = pc.api_call(gpu, empty.poisoned, empty.mask, ws)
    for n in range(2):
        assert np.array_equal(got[n], np.array(pcs.EMPTY), equal_nan=True), (n, got[n])
    pc.compare(got, empty.ref8, empty.ll, empty.mask, empty.what, MEASURED[1025])
    later = pc.api_call(gpu, tenth.poisoned, tenth.mask, ws)
    pc.compare(later, tenth.ref8, tenth.ll, tenth.mask, tenth.what, MEASURED[1025])
    fresh = check(gpu, tenth, pad=0)
    assert np.array_equal(later.view(np.uint64), fresh.view(np.uint64))


@pytest.mark.parametrize("where", ("stride", "end"))
@pytest.mark.parametrize("kept", (1, 2, 4, 24, 25))
def test_few_kept_draws_in_a_long_row(gpu, kept, where):
    """What vi_check's mask looks like after a bad fit: 70 001 draws of which 1 ... 25 are kept, all in one thread's
    stride of the passes or all at the end of the row.  24 and 25 straddle the no-fit threshold (M = 4 and 5)."""
    case = pcs.few_kept_case(70001, kept, where)
    pcs.check_claims(case, kept // 5)
    assert np.all(case.ref8[:, 7] == kept) and np.isnan(case.ref8[:, 3]).all() == (kept == 1)
    assert np.isfinite(case.ref8[:, 1]).all() == (kept == 25)
    assert where != "stride" or np.all(np.flatnonzero(case.mask == 0) % pcs.THREADS == 7)
    check(gpu, case, pad=1)
