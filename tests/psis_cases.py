"""The rows of tests/test_gpu_psis_shapes.py and tests/test_gpu_psis_weights_shapes.py and their float64 references,
built once per session and shared by the two files (a reference at R = 2^24 takes several seconds on a CPU): tail
lengths at the edges of psis.hip's sort and of psis_weights.hip's rank chunks, log-likelihoods of every sign and
magnitude, and masks that leave few draws or none.  Nothing here touches the GPU.

A Case carries what its rows CLAIM (fitted or not; where the cut-off lies; the tail length), and `check_claims` asserts
those claims on the reference, so that a case cannot go vacuous without a test failing."""
import collections
import functools

import numpy as np

import psis_ref as pr
import vicheck_ref as vr

# R at which tail_len(R) reaches a power of two, and one more: psis_ref.tail_len
TABLE = collections.OrderedDict([
    (455, 64), (456, 65), (1820, 128), (1821, 129), (7281, 256), (7282, 257), (29127, 512), (29128, 513),
    (116508, 1024), (116509, 1025), (466033, 2048), (466034, 2049), (1048576, 3072), (1864135, 4096), (1864136, 4097),
    (1 << 24, 12288)])
SMALL_RS = (300, 4097) + tuple(R for R in TABLE if R <= 116509)
LARGE_RS = tuple(R for R in TABLE if 116509 < R < (1 << 24))
CHUNK = 2048                   # psis_weights.hip: kPwChunk
THREADS = 256                  # both kernels' workgroup

Row = collections.namedtuple("Row", ["name", "values", "fitted", "offset", "claim"])
Case = collections.namedtuple("Case", ["what", "names", "ll", "mask", "poisoned", "refs", "ref8", "fitted", "offset", "claims"])


def p2_of(M):
    """The padded length of psis.hip's bitonic network for a tail of M."""
    p2 = 1
    while p2 < M:
        p2 <<= 1
    return p2


def vi_like(rs, R):
    return 700.0 + 3.0 * rs.randn(R) + 2.0 * rs.exponential(size=R)


def triples(rs, R):
    return rs.permutation(np.repeat(-0.5 * rs.exponential(size=(R + 2) // 3), 3)[:R])


def table_rows(R, seed):
    """Every kind of row of the small sizes: what test_gpu_psis.py feeds (all <= 0, of magnitude one) and then positive,
    straddling, offset, subnormal, wide and huge rows.  claim(s, M) speaks about the sorted float32 row s."""
    rs = np.random.RandomState(seed)
    M = pr.tail_len(R)
    rows = [Row("exp k=%g" % k, -k * rs.exponential(size=R), True, False, None) for k in (0.1, 0.5, 0.9, 1.5)]
    rows.append(Row("triples", triples(rs, R), True, False, None))
    # (30 % of the draws hold the smaller value: the tail is constant, its exceedances are all zero)
    rows.append(Row("two values", np.where(rs.rand(R) < 0.3, -2.0, -0.5), False, False, lambda s, M: s[0] == s[M]))
    rows.append(Row("positive", 2.0 + 0.3 * rs.randn(R), True, False, lambda s, M: s[0] > 0.0))
    rows.append(Row("straddling", 0.5 * rs.randn(R), True, False, lambda s, M: s[0] < 0.0 and s[M] < 0.0 and s[-1] > 0.0))
    zeros = np.array([0.0, -0.0, 0.0])
    v = np.concatenate([-rs.exponential(size=M), zeros, rs.exponential(size=R - M - 3)])
    rows.append(Row("cut-off at zero", rs.permutation(v), True, False,
                    lambda s, M: s[M - 1] < 0.0 and np.all(s[M:M + 3] == 0.0) and s[M + 3] > 0.0))
    v = np.concatenate([-rs.exponential(size=M), rs.exponential(size=R - M)])
    rows.append(Row("cut-off at the smallest positive", rs.permutation(v), True, False, lambda s, M: s[M - 1] < 0.0 < s[M]))
    rows.append(Row("offset +1e4", 1e4 + rs.randn(R), True, True, lambda s, M: s[0] > 9e3))
    rows.append(Row("offset -1e4", -1e4 + rs.randn(R), True, True, lambda s, M: s[-1] < -9e3))
    rows.append(Row("VI-like", vi_like(rs, R), True, True, lambda s, M: s[0] > 600.0))
    rows.append(Row("VI-like negated", -vi_like(rs, R), True, True, lambda s, M: s[-1] < -600.0))
    tiny = float(np.finfo(np.float32).tiny)
    rows.append(Row("subnormal normal", 1e-40 * rs.randn(R), False, False,
                    lambda s, M: np.abs(s).max() < tiny and s[0] < 0.0 < s[-1] and s[M] != 0.0))
    rows.append(Row("subnormal -exp", -1e-40 * rs.exponential(size=R), False, False,
                    lambda s, M: np.abs(s).max() < tiny and s[M] < 0.0))
    rows.append(Row("wide", -300.0 * rs.exponential(size=R), False, True, lambda s, M: np.exp(float(s[0]) - float(s[M])) == 0.0))
    rows.append(Row("huge", 3e38 * rs.rand(R) - 1.5e38, False, True, lambda s, M: s[0] < -1e38 and s[-1] > 1e38))
    return rows


def large_rows(R, seed):
    """Three rows of different content: a neighbour's workspace or members slice would show if strides were wrong."""
    rs = np.random.RandomState(seed)
    return [Row("exp k=0.5", -0.5 * rs.exponential(size=R), True, False, None), Row("triples", triples(rs, R), True, False, None),
            Row("VI-like", vi_like(rs, R), True, True, lambda s, M: s[0] > 600.0)]


def limit_rows(R, seed):
    """exp k=0.5 on a grid of 2^-10: ties are plentiful."""
    rs = np.random.RandomState(seed)
    return [Row("exp k=0.5 on a grid", np.round(-0.5 * rs.exponential(size=R) * 1024.0) / 1024.0, True, False, None)]


SHIFTS = (1024.0, 8192.0, -8192.0)


def shift_rows(R, seed):
    """A row on a grid of 2^-10 and the same row shifted by c: the shift is exact in float32, so llmin - ll is the same
    bits in all four rows."""
    rs = np.random.RandomState(seed)
    base = (np.round(rs.randn(R) * 1024.0) / 1024.0).astype(np.float32)
    rows = [Row("grid", base, True, False, None)]
    for c in SHIFTS:
        shifted = base + np.float32(c)
        assert shifted.dtype == np.float32 and np.array_equal(shifted.astype(np.float64), base.astype(np.float64) + c)
        rows.append(Row("grid %+g" % c, shifted, True, True, None))
    return rows


def make_case(what, rows, mask=None):
    names = [r.name for r in rows]
    ll = np.stack([np.asarray(r.values) for r in rows]).astype(np.float32)
    poisoned = ll
    if mask is not None:
        poisoned = ll.copy()
        poisoned[:, np.asarray(mask) != 0] = np.nan                # must never be read
    refs = [vr.weights_row(row, mask) for row in ll]
    return Case(what, names, ll, mask, poisoned, refs, np.stack([r[0] for r in refs]), [r.fitted for r in rows],
                [r.offset for r in rows], [r.claim for r in rows])


def tenth_mask(R, seed):
    rs = np.random.RandomState(seed)
    mask = (rs.rand(R) < 0.1).astype(np.uint8)
    mask[rs.randint(R)] = 0
    return mask


@functools.lru_cache(maxsize=None)
def table_case(R):
    return make_case("table R=%d" % R, table_rows(R, R))


@functools.lru_cache(maxsize=None)
def large_case(R, masked=False):
    return make_case("large R=%d%s" % (R, " masked" if masked else ""), large_rows(R, R), tenth_mask(R, R + 1) if masked else None)


@functools.lru_cache(maxsize=None)
def limit_case():
    return make_case("R=2^24", limit_rows(1 << 24, 24))


@functools.lru_cache(maxsize=None)
def shift_case(R):
    return make_case("shift R=%d" % R, shift_rows(R, R + 7))


def few_kept_mask(R, kept, where):
    """All but `kept` draws masked: the kept ones in one thread's stride of the kernels' passes (i = 7 mod 256), or at the
    very end of the row."""
    mask = np.ones(R, np.uint8)
    if where == "stride":
        mask[7 + THREADS * np.arange(kept) * 11] = 0               # (11: spread over the row, still 7 mod 256)
    else:
        mask[R - kept:] = 0
    assert int((mask == 0).sum()) == kept
    return mask


@functools.lru_cache(maxsize=None)
def few_kept_case(R, kept, where):
    rs = np.random.RandomState(1000 * kept + len(where))
    rows = [Row("exp k=0.5", -0.5 * rs.exponential(size=R), None, False, None), Row("positive", 2.0 + 0.3 * rs.randn(R), None, False, None),
            Row("VI-like", vi_like(rs, R), None, True, None)]
    return make_case("R=%d, %d kept (%s)" % (R, kept, where), rows, few_kept_mask(R, kept, where))


def check_claims(case, M=None):
    """On the CPU, from the reference: the tail length, which rows are fitted, and what each row says about its sorted
    values -- a case that stops being what it says fails here, whatever the device does."""
    keep = np.ones(case.ll.shape[1], bool) if case.mask is None else case.mask == 0
    for n, name in enumerate(case.names):
        r8 = case.ref8[n]
        assert r8[7] == keep.sum(), (case.what, name)
        assert r8[4] == pr.tail_len(int(keep.sum())) and (M is None or r8[4] == M), (case.what, name, r8[4], M)
        if case.fitted[n] is not None:
            assert np.isfinite(r8[0]) and np.isfinite(r8[2]), (case.what, name, r8)
            if case.fitted[n]:
                assert np.isfinite(r8[1]) and np.isfinite(r8[6]) and case.refs[n][2].size == r8[4], (case.what, name, r8)
            else:
                assert r8[1] == np.inf and np.isnan(r8[6]) and case.refs[n][2].size == 0, (case.what, name, r8)
        if case.claims[n] is not None:
            assert case.claims[n](np.sort(case.ll[n][keep]), int(r8[4])), (case.what, name)


def tie_row(R, seed, copies=50):
    """(ll [R] float32, positions, value): a row whose value of rank about M - 20 is repeated at `copies` further places
    spread evenly over the whole row, so that the cut-off rank M falls inside the group of equal values."""
    rs = np.random.RandomState(seed)
    ll = (-0.5 * rs.exponential(size=R)).astype(np.float32)
    M = pr.tail_len(R)
    order = np.argsort(ll, kind="stable")
    value = ll[order[M - 20]]
    high = np.flatnonzero(ll > ll[order[2 * M]])                    # places whose own value is far above the tail
    at = high[np.linspace(0, high.size - 1, copies).astype(np.int64)]
    ll[at] = value
    return ll, np.flatnonzero(ll == value), value


EMPTY = (np.nan, np.inf, np.nan, np.nan, 0.0, np.nan, np.nan, 0.0)          # the columns of a row without a kept draw


@functools.lru_cache(maxsize=None)
def pair_cases(R):
    """(all masked, a tenth masked): the same two rows of different content, NaN under either mask."""
    rs = np.random.RandomState(R + 3)
    rows = [Row("exp k=0.5", -0.5 * rs.exponential(size=R), None, False, None), Row("positive", 2.0 + 0.3 * rs.randn(R), None, False, None)]
    return make_case("R=%d, all masked" % R, rows, np.ones(R, np.uint8)), make_case("R=%d, a tenth masked" % R, rows, tenth_mask(R, R + 1))
