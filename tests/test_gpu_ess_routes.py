"""GPU: arp_ess / arp_ess_ws (csrc/ess.hip, csrc/ess_tail.h) against the float64 yardstick tests/ess_direct_ref.py, per
series, at every route of the kernel and with the cut -- the first negative lag -- placed on the hand-overs between its
stages and rounds (tests/ess_cases.py: inputs, seeds and route predicates, all checked on the CPU by
tests/test_ess_routes_host.py).

Allowance, per series: |ESS - ESS64| <= ESS64 (2 cut + 3) 3e-5 / tau64 -- the project's float32 element tolerance on
every rho up to the cut, carried through tau (the form of tests/test_gpu_mcess.py).  Every series of every case moves by
at least four times that if its cut moves by one lag, so none is excused and a lag dropped or counted twice fails.
The float32 restatement of each route's summation order stays below 5e-6 on rho on these inputs
(test_ess_routes_host.py), a sixth of the tolerance.

Each test prints the largest error / allowance per route (NOTES_r07.md has the figures of the first run).
"""
import numpy as np
import pytest
import torch

import ess_cases

pytestmark = pytest.mark.gpu


def row_floats(S):
    return (S + 63) // 64 * 64


def run(xd, S, n, stride, mode):
    """One call of the C entry points on the device trace xd: rows of n series, `stride` floats apart."""
    from autoreparam_amd import _lib
    L = _lib.lib()
    out = torch.full((n,), -1.0, dtype=torch.float32, device=xd.device)
    if mode == "plain":
        _lib.check(L.arp_ess(_lib.ptr(xd), S, n, stride, _lib.ptr(out), _lib.stream()))
    else:
        need = int(L.arp_ess_workspace_bytes(S, n))
        assert need > 0
        if mode == "rows64":      # the lists and a row area of exactly 64 rows
            need -= ((n + 63) // 64 * 64 - 64) * row_floats(S) * 4
        ws = torch.empty(need, dtype=torch.uint8, device=xd.device)
        _lib.check(L.arp_ess_ws(_lib.ptr(xd), S, n, stride, _lib.ptr(out), _lib.ptr(ws), need, _lib.stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def ratios(got, ref, K):
    """error / allowance per series (0 where both sides are nan, inf where only one is)."""
    got = got.astype(np.float64)
    both_nan = np.isnan(got) & np.isnan(ref.ess)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(got - ref.ess) / (ref.ess * ess_cases.allowance_rel(ref))
    q[both_nan] = 0.0
    q[np.isnan(q)] = np.inf
    assert (both_nan == (K == 0)).all()
    return q


def report(label, q, route):
    per = {}
    for r, v in zip(route, q):
        per[r] = max(per.get(r, 0.0), float(v))
    print("ess-routes %-28s worst %.4f  |  %s" % (label, q.max(), "  ".join("%s %.4f" % kv for kv in sorted(per.items()))))
    bad = np.flatnonzero(~(q <= 1.0))
    assert bad.size == 0, (label, [(int(i), route[i], float(q[i])) for i in bad[:8]])


@pytest.mark.parametrize("name", ess_cases.NAMES)
def test_ess_per_series_at_every_route(gpu, name):
    c, ref = ess_cases.case(name)
    S, n = c.x.shape
    xd = torch.tensor(c.x, device=gpu)
    got = {}
    for mode in c.modes:
        got[mode] = run(xd, S, n, n, mode)
        report("%s/%s" % (name, mode), ratios(got[mode], ref, c.K), ess_cases.plan(S, n, ref.cut, mode).route)
    if "rows64" in got:
        # the listed series in chunks of 64 rows (which series lands in which chunk is the order the waves listed them in):
        # bit for bit the one-chunk result
        assert np.array_equal(got["rows64"].view(np.int32), got["ws"].view(np.int32)), name
    if len(c.modes) == 3:
        # far sweeps and matrix-core tail sum the same products in different orders: within two allowances of each other
        q = np.abs(got["plain"].astype(np.float64) - got["ws"]) / (ref.ess * ess_cases.allowance_rel(ref))
        assert (q <= 2.0).all(), name
    if name.startswith("shadow"):
        # the wave of the last series filled up with finished series instead of shadow lanes: the same stages take it, so the
        # same bits -- shadows that voted would send it through the dense pass (other roundings)
        pad = c.x[:, [i % 3 for i in range(-n % 64)]] if n > 3 else ess_cases.case("shadow_n257")[0].x[:, :63]
        full = np.concatenate([c.x, pad], axis=1)
        assert full.shape[1] % 64 == 0 and ess_cases.plan(S, full.shape[1], ess_cases.ess_direct_ref.ess(full).cut,
                                                          "plain").unfinished[-1] == 1
        filled = run(torch.tensor(full, device=gpu), S, full.shape[1], full.shape[1], "plain")
        assert np.array_equal(filled[:n].view(np.int32), got["plain"].view(np.int32)), name
    again = run(xd, S, n, n, c.modes[-1])
    assert np.array_equal(again.view(np.int32), got[c.modes[-1]].view(np.int32)), name     # the same bits run after run


def test_three_unfinished_series_take_the_cooperative_tail_and_four_the_dense_pass(gpu):
    """The 3 / 4 vote, witnessed by bits.  A series' figure depends on its own samples and on the stages that take it, not
    on its neighbours, and every stage sums in a fixed order: the same series in two waves that take the same route
    gives the same bits, and over 39 series two different routes (cooperative tail from 16 / dense pass, then from 48)
    cannot round to the same float every time.  13 waves, each three unfinished series among 61 finished ones:
        2 and 3 unfinished: the same bits (cooperative tail from 16);  4 and 5: the same bits (dense);  3 and 4: other bits."""
    vote, vref = ess_cases.case("dense_vote")
    retake, rref = ess_cases.case("retake")
    S = vote.x.shape[0]
    pool = [vote.x[:, i] for i in np.flatnonzero(vref.cut > 16)]
    pool += [retake.x[:, i] for i in np.flatnonzero(rref.cut > 16) if i not in retake.expect["retakes"]]
    assert len(pool) == 39
    fill = vote.x[:, [i for i in range(64) if vref.cut[i] <= 16]]
    extra = [vote.x[:, 100], vote.x[:, 127]]                       # a fourth and a fifth unfinished series (cuts 49, 113)

    def trace(k):
        """13 waves with k unfinished series each: k <= 3 of the wave's own triple, then the extras."""
        cols = []
        for w in range(13):
            wave = [fill[:, j % fill.shape[1]] for j in range(64)]
            for q, pos in enumerate((7, 30, 63)[:min(k, 3)]):
                wave[pos] = pool[3 * w + q]
            for q in range(k - 3):
                wave[1 + q] = extra[q]
            cols += wave
        return np.stack(cols, axis=1)

    wit = np.array([64 * w + pos for w in range(13) for pos in (7, 30, 63)])
    res = {}
    for k in (2, 3, 4, 5):
        x = trace(k)
        p = ess_cases.plan(S, x.shape[1], ess_cases.ess_direct_ref.ess(x).cut, "plain")
        assert p.unfinished == [k] * 13 and p.dense == [k > 3] * 13
        res[k] = run(torch.tensor(x, device=gpu), S, x.shape[1], x.shape[1], "plain").view(np.int32)
    two = wit.reshape(13, 3)[:, :2].ravel()
    assert np.array_equal(res[2][two], res[3][two])
    assert np.array_equal(res[4][wit], res[5][wit])
    differ = int((res[3][wit] != res[4][wit]).sum())
    print("ess-routes vote: %d of 39 series round differently through the dense pass" % differ)
    assert differ >= 3


def test_inner_block_of_a_wider_trace_on_the_matrix_core_tail(gpu):
    """util.effective_sample_size on chains 3 .. 10 of a [S, 16, 8] trace, in place (row_stride 128 > n_series 64, first
    series 24): ess_gather_kernel reads rows a wider stride apart.  Bit for bit the block's contiguous copy, and the
    yardstick's figures."""
    from autoreparam_amd import util
    c, ref = ess_cases.case("inner_S2233")
    S, n = c.x.shape
    wide = np.empty((S, 16, 8), np.float32)
    block = c.x.reshape(S, 8, 8)
    wide[:, 3:11] = block
    wide[:, :3] = block[:, ::-1][:, :3] + np.float32(1.0)           # neighbours that differ from the block
    wide[:, 11:] = block[:, ::-1][:, :5] * np.float32(0.5)
    xd = torch.tensor(wide, device=gpu)
    view = xd[:, 3:11, :]
    assert not view.is_contiguous()
    in_place = util.effective_sample_size(view)
    copied = util.effective_sample_size(view.contiguous())
    assert torch.equal(in_place.view(torch.int32), copied.view(torch.int32))
    assert ess_cases.plan(S, n, ref.cut, "ws").listed == c.expect["listed"] > 0
    report("inner_S2233/util view", ratios(in_place.cpu().numpy().reshape(n), ref, c.K),
           ess_cases.plan(S, n, ref.cut, "ws").route)
    # the C entry point with the stride and the offset spelled out
    direct = run(xd.reshape(S, 128)[:, 24:], S, n, 128, "rows64")
    assert np.array_equal(direct.view(np.int32), copied.cpu().numpy().reshape(n).view(np.int32))


def test_wave_family_through_util(gpu):
    """util.effective_sample_size (the product's own caller) on the S = 48 case: the cooperative tail for all 64 series."""
    from autoreparam_amd import util
    c, ref = ess_cases.case("coop_nodense_S48")
    S, n = c.x.shape
    got = util.effective_sample_size(torch.tensor(c.x, device=gpu).reshape(S, 8, 8)).cpu().numpy().reshape(n)
    report("coop_nodense_S48/util", ratios(got, ref, c.K), ess_cases.plan(S, n, ref.cut, "plain").route)


@pytest.mark.parametrize("name", ess_cases.TILE_NAMES)
def test_one_pass_tile_kernel_at_the_same_cuts(gpu, monkeypatch, name):
    """ess_tile_kernel (32 <= S <= 1 024) cuts every series at its own lag, 16 lags per round: the short cases -- cuts at its
    hand-overs 16/17 and 32/33 among them where the case has them -- against the same yardstick and allowance."""
    from autoreparam_amd import util
    c, ref = ess_cases.case(name)
    S, n = c.x.shape
    assert 32 <= S <= 1024 and n >= 2
    xd = torch.tensor(c.x, device=gpu).reshape(S, n, 1)
    monkeypatch.setenv("ARP_DEBUG", "1"); monkeypatch.setenv("ARP_ESS_TILE", "1")
    got = util.effective_sample_size(xd).cpu().numpy().reshape(n)
    monkeypatch.setenv("ARP_ESS_TILE", "0")
    two_sweep = util.effective_sample_size(xd).cpu().numpy().reshape(n)
    rounds = ["tile:first" if k <= 16 else "tile:round%d" % ((k - 17) // 16 + 1) for k in ref.cut]
    report("%s/tile" % name, ratios(got, ref, c.K), rounds)
    assert not np.array_equal(got, two_sweep)                   # (the switch took effect: another kernel, other roundings)
