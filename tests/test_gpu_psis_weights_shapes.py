"""GPU: arp_psis_weights (csrc/psis.hip, csrc/psis_weights.hip) against tests/vicheck_ref.py: weights_row where the
arp_psis_weights part of tests/test_gpu_vicheck.py does not go, on the rows of tests/test_gpu_psis_shapes.py (rows and
references: tests/psis_cases.py, built once for both files):
  tail lengths   past one rank chunk of 2 048 members: M = 2 048 (exactly one chunk), 2 049 (a second chunk holding one
                 member), 3 072 (2^20 draws, the most --vi_check_draws takes), 4 096 / 4 097 (a third chunk) and 12 288
                 (2^24 draws: six chunks, 48 rounds of the rank loop); below that every M a power of two and one more;
  signs and magnitudes, an exact shift (every lw the same BITS), every draw masked, 1 ... 25 kept draws of 70 001;
  a group of ties at the cut-off whose members lie in different thread segments of the members pass.
out is arp_psis_loo's bit for bit (psis_checks.device_weights); the draws whose weight differs from the raw one are
the reference's tail; raw positions EQUAL; smoothed positions within 16 x the largest deviation measured over these
very cases on an MI355X, per class of tail length, relative to max(|lw|, 1) (LW_MEASURED below); each recorded figure
must itself stay below M^2 2^-53, what float64 predicts at the class's largest M."""
import numpy as np
import pytest

import psis_cases as pcs
import psis_checks as pc
import psis_ref as pr
import vicheck_ref as vr

pytestmark = pytest.mark.gpu

# class (the largest M in it) -> largest |lw_dev - lw_ref| / max(|lw_ref|, 1) at a smoothed position over every case of
# this file, measured on an MI355X; the tests allow 16 x these.  Where each occurred: R = 116 508, M = 1 024; R =
# 1 864 136, M = 4 097 (at M = 3 072: 5.13e-14); R = 2^24.  Float64 predicts up to M^2 2^-53 = 1.2e-10, 1.9e-9, 1.7e-8.
LW_MEASURED = {
    1025: 1.03e-13,
    4097: 1.57e-13,
    12288: 1.02e-13,
}


def klass(M):
    return min(c for c in LW_MEASURED if M <= c)


def check(gpu, case, pad):
    """One call of psis_weights (and of psis_loo, for out) on the case's rows against its references; prints the record."""
    M = int(case.ref8[:, 4].max())
    out, lw = pc.device_weights(gpu, case.poisoned, case.mask, pad=pad)
    worst = pc.compare_weights(lw, case.ll, case.mask, case.names, case.what, LW_MEASURED[klass(M)], case.refs)
    print("psis_weights %s: M %d (class %d): largest deviation at a smoothed position %.3g" % (case.what, M, klass(M), worst))
    for n in range(case.ll.shape[0]):                              # the exact columns of out, once more through this entry point
        assert out[n, 4] == case.ref8[n, 4] and out[n, 7] == case.ref8[n, 7], (case.what, n)
        assert out[n, 5] == case.ref8[n, 5] or (np.isnan(out[n, 5]) and np.isnan(case.ref8[n, 5])), (case.what, n)
    return out, lw


def test_recorded_figures_are_below_the_float64_prediction():
    for M, figure in LW_MEASURED.items():
        assert 0.0 < figure < M * M * 2.0 ** -53, (M, figure)


@pytest.mark.parametrize("R", pcs.SMALL_RS)
def test_table_rows_of_every_sign_and_magnitude(gpu, R):
    """Every kind of row at R = 300, 4 097 and where M crosses 64 ... 1 024: the second round of the rank loop over m0
    begins at M = 257."""
    case = pcs.table_case(R)
    pcs.check_claims(case, pcs.TABLE.get(R, pr.tail_len(R)))
    check(gpu, case, pad=13)


@pytest.mark.parametrize("R", pcs.LARGE_RS)
def test_tails_past_one_rank_chunk(gpu, R):
    case = pcs.large_case(R)
    M = pcs.TABLE[R]
    pcs.check_claims(case, M)
    assert all(case.fitted) and all(r[2].size == M for r in case.refs)     # fitted: the rank loop runs
    chunks = -(-M // pcs.CHUNK)
    assert chunks == {466033: 1, 466034: 2, 1048576: 2, 1864135: 2, 1864136: 3}[R]
    assert R == 466033 or M > pcs.CHUNK                            # the loop over c0 goes past 0
    check(gpu, case, pad=3)


def test_long_tail_with_a_tenth_masked(gpu):
    case = pcs.large_case(466034, True)
    pcs.check_claims(case)
    assert 1024 < case.ref8[0, 4] < 2048 and 0 < case.mask.sum() < 466034 // 8
    check(gpu, case, pad=5)


def test_the_limit_of_2_to_the_24_draws(gpu):
    """One row at the API's limit, through both entry points.  The time is the reference's."""
    case = pcs.limit_case()
    pcs.check_claims(case, 12288)
    assert case.refs[0][2].size == 12288 == 6 * pcs.CHUNK
    check(gpu, case, pad=0)


@pytest.mark.parametrize("R", (4097, 29128))
def test_an_exact_shift_changes_no_bit_of_any_weight(gpu, R):
    case = pcs.shift_case(R)
    pcs.check_claims(case)
    base = case.ll[0].astype(np.float64)
    for n, c in enumerate(pcs.SHIFTS, 1):
        assert np.array_equal(case.ll[n].astype(np.float64), base + c)                 # the shift was exact
    out, lw = check(gpu, case, pad=7)
    for n, c in enumerate(pcs.SHIFTS, 1):
        assert np.array_equal(lw[n].view(np.uint64), lw[0].view(np.uint64)), (c, np.flatnonzero(lw[n] != lw[0])[:8])
        assert np.array_equal(out[n, [1, 4, 5, 6, 7]].view(np.uint64), out[0, [1, 4, 5, 6, 7]].view(np.uint64)), c


def test_a_group_of_ties_over_the_whole_row_is_split_by_draw_index(gpu):
    """R = 466 034, M = 2 049 (two rank chunks): 51 equal values spread over the thread segments [t L, (t + 1) L) of the
    members pass, about one in every fifth, with the cut-off rank inside the group.  The members inside the tail are those of the lowest draw
    indices, and within the group the smoothed weights descend with the draw index (tests/test_gpu_vicheck.py:
    test_weights_split_a_group_of_ties_by_draw_index at R = 300)."""
    R = 466034
    M = pcs.TABLE[R]
    ll, at, value = pcs.tie_row(R, 5)
    _, ref, tail = vr.weights_row(ll)
    s = np.sort(ll)
    below = int((s < value).sum())
    n_in = M - below
    L = -(-R // pcs.THREADS)
    assert tail.size == M > pcs.CHUNK and at.size == 51 and s[M] == value == s[M - 1]  # the cut-off lies inside the group
    assert 0 < n_in < at.size and np.unique(at // L).size >= at.size - 1 and np.unique(at[:n_in] // L).size >= n_in - 1
    assert np.array_equal(np.intersect1d(at, tail), at[:n_in])     # the reference: the lowest draw indices
    other = pcs.large_case(R).ll[0]                                # a neighbour of different content
    rows = np.stack([ll, other, ll[::-1].copy()])
    _, lw = pc.device_weights(gpu, rows, pad=9)
    worst = pc.compare_weights(lw, rows, None, ["ties", "exp k=0.5", "ties reversed"], "ties R=%d" % R, LW_MEASURED[klass(M)])
    print("psis_weights ties R=%d: M %d (class %d): largest deviation at a smoothed position %.3g" % (R, M, klass(M), worst))
    for row, got, where in ((ll, lw[0], at), (rows[2], lw[2], (R - 1 - at)[::-1])):
        raw = float(row.min()) - row.astype(np.float64)
        inside = where[got[where] != raw[where]]
        assert np.array_equal(inside, where[:n_in]), (inside, where[:n_in])
        assert np.all(np.diff(got[inside]) < 0.0), got[inside]
        assert np.array_equal(got[where[n_in:]], raw[where[n_in:]])


@pytest.mark.parametrize("R", (1, 300, 70001))
def test_every_draw_masked(gpu, R):
    """R' = 0 in both rows of a call: the columns of an empty row and lw = -inf everywhere; then, on the SAME workspace,
    the same rows with a tenth masked."""
    empty, tenth = pcs.pair_cases(R)
    pcs.check_claims(empty)
    pcs.check_claims(tenth)
    assert empty.ref8[0, 7] == 0 and np.all(empty.mask != 0) and np.isnan(empty.poisoned).all() and tenth.ref8[0, 7] > 0
    ws = pc.api_workspace(gpu, 2, R)
    out, lw = pc.api_call(gpu, empty.poisoned, empty.mask, ws, weights=True)
    for n in range(2):
        assert np.array_equal(out[n], np.array(pcs.EMPTY), equal_nan=True), (n, out[n])
    assert lw.shape == (2, R) and np.all(np.isneginf(lw))
    pc.compare_weights(lw, empty.ll, empty.mask, empty.names, empty.what, LW_MEASURED[1025], empty.refs)
    out, later = pc.api_call(gpu, tenth.poisoned, tenth.mask, ws, weights=True)
    pc.compare_weights(later, tenth.ll, tenth.mask, tenth.names, tenth.what, LW_MEASURED[1025], tenth.refs)
    fresh_out, fresh = check(gpu, tenth, pad=0)
    assert np.array_equal(later.view(np.uint64), fresh.view(np.uint64)) and np.array_equal(out.view(np.uint64), fresh_out.view(np.uint64))


@pytest.mark.parametrize("where", ("stride", "end"))
@pytest.mark.parametrize("kept", (1, 2, 4, 24, 25))
def test_few_kept_draws_in_a_long_row(gpu, kept, where):
    """70 001 draws of which 1 ... 25 are kept, all in one thread's stride of the passes or all at the end of the row
    (the last thread segment of the members pass); fitted from 25 kept draws on."""
    case = pcs.few_kept_case(70001, kept, where)
    pcs.check_claims(case, kept // 5)
    assert all(r[2].size == (5 if kept == 25 else 0) for r in case.refs)
    out, lw = check(gpu, case, pad=1)
    kept_lw = lw[:, case.mask == 0]
    assert np.all(np.isfinite(kept_lw)) and np.all(kept_lw <= 0.0)
    assert kept == 25 or (kept_lw == 0.0).any(axis=1).all()            # raw weights: the largest is 0
