"""CPU: everything tests/test_gpu_ess_routes.py rests on, checked before any GPU run.

  * the yardstick (tests/ess_direct_ref.py) equals oracle/ess_ref.py: ess_fft on the AR(1) traces of the older ESS tests;
  * every series of every case of tests/ess_cases.py cuts at its intended lag with sens >= 4 x allowance, and every
    case takes the route it states (predicates of the yardstick);
  * a float32 NumPy restatement of each route's SUMMATION ORDER (csrc/ess.hip, csrc/ess_tail.h) stays within the project's
    float32 element tolerance, |rho - rho64| <= 3e-5, on those very inputs -- so a device result outside the allowance
    (2 cut + 3) 3e-5 / tau is the kernel's doing, not the arithmetic's:
        sweep 1      windows of 128 products (float fma chains) added into float running totals, centred afterwards in
                     double about the reference level r (retaken about the mean where m^2 > 16)
        dense        one unflushed float fma chain per lag
        cooperative  four interleaved float fma chains, added in double
        far          windows of 128 products flushed into double
        matrix core  per (lag, sample index mod 16) a float fma chain, folded every 65 536 samples; diagonal sums in float
"""
import functools

import numpy as np
import pytest

import ess_cases
import ess_direct_ref
from ess_cases import W, RHO_TOL
from oracle import ess_ref

F32, F64 = np.float32, np.float64


# ---- the yardsticks are one

def _older_traces():
    rho = np.array([0.0, 0.3, 0.6, 0.9, -0.4])
    x = (ess_ref.ar1(600, (37, 5), rho, seed=5) * [1.0, 10.0, 0.1, 3.0, 1.0] + [0.0, 100.0, -5.0, 1e3, 0.0]).astype(F32)
    yield "ar1_600", x
    drift = x.copy()
    drift[:20] += np.array([50.0, 5e3, 3.0, 2e4, -80.0], F32)
    yield "drift", drift
    yield "short_9", x[:9]
    yield "slow_3000", ess_ref.ar1(3000, (16, 3), [0.98, 0.95, 0.5], seed=7).astype(F32)
    rho = np.array([0.995, 0.97, 0.5, 0.9, -0.2])
    yield "long_6000", (ess_ref.ar1(6000, (24, 5), rho, seed=11) * [1.0, 4.0, 0.1, 30.0, 1.0]
                        + [0.0, -20.0, 5.0, 1e3, 0.0]).astype(F32)
    rho64 = np.zeros(64); rho64[5] = 0.99; rho64[40] = 0.6
    yield "one_slow_per_wave", ess_ref.ar1(4000, (3, 64), rho64, seed=13).astype(F32)
    yield "inner_40", ess_ref.ar1(40, (16, 5), [0.0, 0.3, 0.6, 0.9, -0.4], seed=11).astype(F32)


def test_yardstick_equals_the_fft_oracle():
    """FFT and direct lag sums in float64 agree to ~ 1e-13 on rho; 1e-8 on the ESS leaves room for the longest sums."""
    for name, x in _older_traces():
        S = x.shape[0]
        flat = x.reshape(S, -1)
        got = ess_direct_ref.ess(flat)
        want = ess_ref.ess_fft(flat)
        np.testing.assert_allclose(got.ess, want, rtol=1e-8, err_msg=name)
        # cut and rho as the FFT form has them
        xc = flat.astype(F64) - flat.astype(F64).mean(axis=0)
        for i in range(0, flat.shape[1], 7):
            ac = np.array([(xc[:S - k, i] * xc[k:, i]).sum() / (S - k) for k in range(min(S, 40))])
            rho = ac / ac[0]
            first = np.flatnonzero(rho < 0)
            if first.size:
                assert got.cut[i] == first[0], (name, i)
            k = min(got.cut[i], len(rho) - 1)
            np.testing.assert_allclose(got.rho[:k + 1, i], rho[:k + 1], rtol=0, atol=1e-12)
    assert np.isnan(ess_direct_ref.ess(np.ones((50, 3), F32)).ess).all()
    two = ess_direct_ref.ess(np.array([[1.0], [2.0]], F32))
    assert two.ess[0] == 2.0 and two.cut[0] == 1 and two.rho[1, 0] == -1.0


def test_sens_is_the_change_of_the_ess_when_the_cut_moves():
    c, ref = ess_cases.case("dense_vote")
    S = c.x.shape[0]
    for i in (9, 31, 64, 127):
        k = ref.cut[i]
        longer = S / (ref.tau[i] + 2.0 * (S - k) / S * ref.rho[k, i])
        shorter = S / (ref.tau[i] - 2.0 * (S - k + 1) / S * ref.rho[k - 1, i])
        # first order: |d ESS| / ESS = |d tau| / tau
        rel = min(abs(longer / ref.ess[i] - 1), abs(shorter / ref.ess[i] - 1))
        assert abs(rel / ref.sens[i] - 1) < 0.5 and ref.sens[i] > 0


# ---- every case: cut, margin, route

@pytest.mark.parametrize("name", ess_cases.NAMES)
def test_case_cuts_where_intended_and_takes_its_route(name):
    c, ref = ess_cases.case(name)
    S, n = c.x.shape
    nan = c.K == 0
    assert np.isnan(ref.ess[nan]).all() and not np.isnan(ref.ess[~nan]).any()
    assert (ref.cut[~nan] == c.K[~nan]).all(), (name, ref.cut, c.K)
    assert (ref.sens[~nan] >= 4.0 * ess_cases.allowance_rel(ref)[~nan]).all(), name
    for mode in c.modes:
        p = ess_cases.plan(S, n, ref.cut, mode)
        assert p.unfinished == c.expect["unfinished"] and p.dense == c.expect["dense"], (name, p.unfinished, p.dense)
        if mode != "plain":
            assert S + 72 > ess_cases.LDS_FLOATS and p.listed == c.expect.get("listed", p.listed), (name, p.listed)
    retakes, _ = ess_cases.retake_predicate(c.x)
    assert list(np.flatnonzero(retakes)) == c.expect.get("retakes", []), name


def test_the_cases_cover_every_route_and_hand_over():
    seen = {}
    for name in ess_cases.NAMES:
        c, ref = ess_cases.case(name)
        for mode in c.modes:
            for r, k in zip(ess_cases.plan(*c.x.shape, ref.cut, mode).route, ref.cut):
                seen.setdefault(r, set()).add(int(k))
    want = {"sweep1": {1, 3, 15, 16}, "dense": {17, 48}, "coop16": {17, 80, 81}, "coop48": {49, 112, 113},
            "far16": {17, 32, 33, 64, 65}, "far48": {49, 80, 81}, "mfma16": {17, 256, 257, 272, 273, 304, 305},
            "mfma48": {49, 256, 257, 272, 273, 288, 289, 304, 305}}
    for r, ks in want.items():
        assert ks <= seen.get(r, set()), (r, sorted(ks - seen.get(r, set())))
    assert ess_cases.case("limit_S2232_dense")[0].x.shape[0] + 72 == ess_cases.LDS_FLOATS


# ---- float32 restatements of the routes' summation orders

def seq32(p):
    """p [T, ...] float64 (exact products of float32 values, or float32 partial sums) -> the float32 chain
    acc = fl32(acc + p[t]) over t."""
    acc = np.zeros(p.shape[1:], F32)
    for t in range(p.shape[0]):
        acc = (acc + p[t]).astype(F32)
    return acc


def _pad(p, m):
    T = p.shape[0]
    if T % m:
        p = np.concatenate([p, np.zeros((m - T % m,) + p.shape[1:], p.dtype)])
    return p


def back_products(y, lags):
    """P[t, i, ...] = y[t] y[t - lags[i]] (0 before the start), exact in float64: the sums indexed by the LEADING sample."""
    S = y.shape[0]
    y64 = y.astype(F64)
    P = np.zeros((S, len(lags)) + y.shape[1:])
    for i, k in enumerate(lags):
        if k < S:
            P[k:, i] = y64[k:] * y64[:S - k]
    return P


def fwd_products(y, lags):
    """P[u, i] = y[u] y[u + lags[i]] (0 past the end): the sums indexed by the LAGGED sample."""
    S = y.shape[0]
    y64 = y.astype(F64)
    P = np.zeros((S, len(lags)) + y.shape[1:])
    for i, k in enumerate(lags):
        if k < S:
            P[:S - k, i] = y64[:S - k] * y64[k:]
    return P


def windows32(P):
    """[T, ...] -> [T / 128, ...]: float32 chains over windows of 128 consecutive rows."""
    P = _pad(P, 128)
    return seq32(P.reshape((-1, 128) + P.shape[1:]).swapaxes(0, 1))


def sweep_first(x):
    """ess_kernel up to lag 16: rho32 [17, n] (nan from lag S on), mean [n] float32 and c0 [n] as the later stages get them."""
    S, n = x.shape
    nh = min(S, W)
    d = np.zeros(n, F32)
    for j in range(1, nh):
        d = d + (x[j] - x[0])
    r = x[0] + d / F32(nh)

    def attempt(x, r):
        y = x - r                                                                # float32
        tot = seq32(windows32(back_products(y, range(W + 1))).astype(F64))       # [17, n] float running totals
        T = seq32(windows32(y.astype(F64)).astype(F64)).astype(F64)
        mp = T / S
        mean = r + mp.astype(F32)
        c0 = (tot[0].astype(F64) - S * mp * mp) / S
        return y, tot.astype(F64), T, mp, mean, c0

    y, tot, T, mp, mean, c0 = attempt(x, r)
    again = np.flatnonzero(mp * mp > 16.0 * c0)
    if again.size:
        r = r.copy(); r[again] = mean[again]
        y2, tot2, T2, mp2, mean2, c02 = attempt(x[:, again], r[again])
        y = y.copy(); y[:, again] = y2
        tot[:, again], T[again], mp[again], mean[again], c0[again] = tot2, T2, mp2, mean2, c02
    rho = np.full((W + 1, n), np.nan)
    rho[0] = 1.0
    head = np.zeros(n); tail = np.zeros(n)
    y64 = y.astype(F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(1, W + 1):
            if j - 1 < nh:
                head = head + y64[j - 1]
                tail = tail + y64[S - j]
            if j < S:
                rho[j] = (tot[j] - mp * (2.0 * T - head - tail) + (S - j) * mp * mp) / (S - j) / c0
    return rho, mean, c0, set(again.tolist())


def dense32(y, lags):
    return seq32(back_products(y, lags)).astype(F64)


def coop32(y, lags):
    P = _pad(fwd_products(y, lags), 4)
    a = seq32(P.reshape((-1, 4) + P.shape[1:])).astype(F64)                       # [4, lags]
    return (a[0] + a[1]) + (a[2] + a[3])


def far32(y, lags):
    return windows32(back_products(y, lags)).astype(F64).sum(axis=0)


def mfma32(y, lags, start):
    """ess_tail_kernel: element (m, n) of block j is the chain over kappa of y[16 kappa + m] y[16 kappa + m + 16 j + n - m],
    folded into the lag's float sum every 4 096 kappa; lag 16 j + d is diagonal d of block j (m < 16 - d) plus diagonal
    d - 16 of block j + 1 (m >= 16 - d), each summed over m in float first.  Where block j is the last of a round of 16
    blocks (from block start / 16 on) the second diagonal arrives a round later, after every fold of the first."""
    P = _pad(fwd_products(y, lags), 16)
    P = P.reshape(-1, 16, len(lags))                                               # [kappa, m, lag]
    chains = [seq32(P[k0:k0 + 4096]) for k0 in range(0, P.shape[0], 4096)]         # per fold: [m, lag] float32
    out = np.zeros(len(lags))
    for i, L in enumerate(lags):
        j, d = divmod(L, 16)
        parts = [(seq32(ch[:16 - d, i:i + 1].astype(F64))[0], seq32(ch[16 - d:, i:i + 1].astype(F64))[0]) for ch in chains]
        split = (j - start // 16) % 16 == 15 and d >= 1
        order = [p[0] for p in parts] + [p[1] for p in parts] if split else [v for p in parts for v in p]
        out[i] = seq32(np.array(order, F64)[:, None])[0]
    return out


TAILS = {"coop": coop32, "far": far32}


@functools.lru_cache(maxsize=None)
def first_stages(name):
    """rho32 of the lags the first-stage sweeps take (sweep 1, and the dense pass where the wave takes it)."""
    c, ref = ess_cases.case(name)
    S, n = c.x.shape
    rho1, mean, c0, again = sweep_first(c.x)
    p = ess_cases.plan(S, n, ref.cut, "plain")
    dense = {}
    cols = [i for i in range(n) if p.dense[i // 64] and ref.cut[i] > W]
    if cols:
        top = int(min(ref.cut[cols].max(), W + ess_cases.DENSE_LAGS))
        lags = list(range(W + 1, top + 1))
        acc = dense32(c.x[:, cols] - mean[cols], lags)
        for q, i in enumerate(cols):
            dense[i] = acc[:, q] / (S - np.array(lags)) / c0[i]
    return rho1, mean, c0, dense, again


def restated_errors(name, mode):
    """{route: largest |rho32 - rho64| over the lags 0 .. cut that route takes}."""
    c, ref = ess_cases.case(name)
    S, n = c.x.shape
    rho1, mean, c0, dense, again = first_stages(name)
    p = ess_cases.plan(S, n, ref.cut, mode)
    worst = {}

    def note(route, err):
        worst[route] = max(worst.get(route, 0.0), float(err))

    for i in range(n):
        if c.K[i] == 0:
            continue
        cut = int(ref.cut[i])
        k1 = min(cut, W, S - 1)
        note("retake" if i in again else "sweep1", np.abs(rho1[:k1 + 1, i] - ref.rho[:k1 + 1, i]).max())
        start = W
        if i in dense:
            k2 = min(cut, W + ess_cases.DENSE_LAGS)
            note("dense", np.abs(dense[i][:k2 - W] - ref.rho[W + 1:k2 + 1, i]).max())
            start = W + ess_cases.DENSE_LAGS
        if cut > start and S > W:
            route = p.route[i]
            assert route[-2:] == str(start) and route[:-2] in ("coop", "far", "mfma"), (name, i, route)
            y = c.x[:, i] - mean[i]
            for l0 in range(start + 1, min(cut, S - 1) + 1, 64):
                lags = list(range(l0, min(l0 + 64, min(cut, S - 1) + 1)))
                s = mfma32(y, lags, start) if route[:-2] == "mfma" else TAILS[route[:-2]](y, lags)
                note(route, np.abs(s / (S - np.array(lags)) / c0[i] - ref.rho[lags, i]).max())
    return worst


@pytest.mark.parametrize("name", ess_cases.NAMES)
def test_restated_summation_orders_stay_inside_the_rho_tolerance(name):
    c, _ = ess_cases.case(name)
    tails = sorted({"far" if m == "plain" else "mfma" for m in c.modes})          # (short series: the one cooperative tail)
    for t in tails:
        worst = restated_errors(name, "plain" if t == "far" else "ws")
        print(name, t, " ".join("%s %.2g" % kv for kv in sorted(worst.items())))
        for route, err in worst.items():
            assert err <= RHO_TOL, (name, route, err)
