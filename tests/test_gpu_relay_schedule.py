"""The relay's cut of a launch into segments of unequal length (relay_host.h: relay_schedule; kernels.h: relay_begin reads
HmcParams::seg_start): the schedule's properties through arp_relay_schedule (no device), and on the GPU every cut -- the
library's taper and explicit lists -- against the launch with one workgroup per chain block, bit for bit."""
import numpy as np
import pytest
import torch

import helpers

CHAINS = 520      # x 4 lanes: 9 chain blocks, the last ragged


def _schedule(n_steps, segs, pct):
    from autoreparam_amd import engine
    return engine.Engine.relay_schedule(n_steps, segs, pct)


def _equal_cut(n_steps, segs):
    each = -(-n_steps // segs)
    return [each] * (segs - 1) + [n_steps - (segs - 1) * each]


def test_schedule_properties():
    """For launches of 256 .. 4 096 steps, 2 .. 16 segments and ratios 50 .. 100 %: as many segments as asked, lengths that sum
    to the launch, never increase and are all >= 1, the same on every call; ratio 100 is the equal cut (ceil(n / segs) steps
    each, the last segment what is left)."""
    import __graft_entry__ as ge
    ge.build()
    steps = sorted(set(range(256, 601)) | set(range(600, 4097, 37)) | {1000, 1023, 1024, 1025, 2048, 4095, 4096})
    for n in steps:
        for segs in range(2, 17):
            for pct in range(50, 101, 5 if n > 600 else 1):
                got = _schedule(n, segs, pct)
                assert len(got) == segs, (n, segs, pct)
                assert sum(got) == n, (n, segs, pct, got)
                assert all(a >= b for a, b in zip(got, got[1:])), (n, segs, pct, got)
                assert min(got) >= 1, (n, segs, pct, got)
            assert _schedule(n, segs, 100) == _equal_cut(n, segs), (n, segs)
    for n, segs, pct in ((1024, 8, 70), (300, 4, 50), (4096, 16, 85)):
        assert _schedule(n, segs, pct) == _schedule(n, segs, pct)
    # a taper is one: the first segment is longer than the equal share, the last shorter
    got = _schedule(1024, 8, 70)
    assert got[0] > 128 > got[-1]
    # the library's own ratio (0) is one of the ratios
    assert _schedule(1024, 8, 0) in [_schedule(1024, 8, p) for p in range(1, 101)]


def test_schedule_refuses_what_it_cannot_cut():
    import __graft_entry__ as ge
    ge.build()
    from autoreparam_amd import _lib
    import ctypes as C
    L = _lib.lib()
    out = (C.c_int32 * 4)()
    assert L.arp_relay_schedule(256, 8, 70, out, 4) == 0 and b"arp_relay_schedule" in L.arp_last_error()
    assert L.arp_relay_schedule(3, 4, 70, out, 4) == 0
    assert L.arp_relay_schedule(256, 0, 70, out, 4) == 0
    assert L.arp_relay_schedule(256, 4, 101, out, 4) == 0
    assert L.arp_relay_schedule(256, 4, 70, None, 4) == 0
    assert L.arp_relay_schedule(4, 4, 50, out, 4) == 4 and list(out) == [1, 1, 1, 1]


# ---------------------------------------------------------------------------------------------------------------------
def _cuts(T):
    """(what to set, segments expected): the library's cut at 2, 3 and 8 segments with its own ratio and with a steep one, then
    explicit lists -- for T = 256: 255,1 / 1,255 / 129,127 (a boundary between two thinned rows) / 100,1,57,98 / 8 x 32"""
    cuts = [({"ARP_SEGMENTS": str(s)}, s) for s in (2, 3, 8)]
    cuts += [({"ARP_SEGMENTS": str(s), "ARP_SEGMENT_RATIO": "50"}, s) for s in (2, 3, 8)]
    for lens in ([T - 1, 1], [1, T - 1], [129, T - 129], [100, 1, 57, T - 158], [32] * 7 + [T - 224]):
        cuts.append(({"ARP_SEGMENT_LENS": ",".join(str(v) for v in lens)}, len(lens)))
    return cuts


_SWITCHES = ("ARP_SEGMENTS", "ARP_SEGMENT_RATIO", "ARP_SEGMENT_LENS")


def _set(monkeypatch, env):
    monkeypatch.setenv("ARP_DEBUG", "1")
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _radon_run(eng, sp, q0, gpu, T, thin, with_stats):
    """two interleaved launches of T steps (the second from the first one's state), burn-in ending inside a segment;
    returns the segments of the last launch and every array the launches wrote"""
    from autoreparam_amd import engine, _lib
    e = np.full(sp.D, 0.06, np.float32); e[2] = 0.015
    st = engine.ChainState(torch.as_tensor(q0, device=gpu))
    n_burn = 101
    S = (2 * T - n_burn - 1) // thin + 1
    tr = torch.zeros(S, CHAINS, sp.D, device=gpu)
    a0 = torch.zeros(S, CHAINS, dtype=torch.uint8, device=gpu); a1 = torch.zeros_like(a0)
    extra = dict(stats=torch.zeros(6, CHAINS, sp.D, device=gpu), stats_batch=3, n_samples=S) if with_stats else {}
    for _ in range(2):
        eng.interleaved_run(st, e, e, 4, 4, T, seed=9, adapt_kind=_lib.ADAPT_SIMPLE, n_adapt=150, n_burnin=n_burn, thin=thin,
                            trace=tr, trace_accept0=a0, trace_accept1=a1, trace_centered=False, lanes=4, **extra)
    torch.cuda.synchronize()
    eng.check()
    out = [st.q, st.grad, st.logp, st.adapt, st.adapt1, st.accept_count, st.accept_count1, st.rng, tr, a0, a1]
    if with_stats:
        out.append(extra["stats"])
    return eng.relay_geometry()["segments"], [t.cpu().numpy() for t in out]


@pytest.mark.gpu
@pytest.mark.parametrize("T,thin", [(256, 2), (256, 3), (300, 2), (300, 3)])
def test_every_cut_equals_the_unsegmented_launch(gpu, monkeypatch, T, thin):
    """radon PA interleaved, 520 chains x 4 lanes: states, gradients, log densities, adaptation, counters, generator states,
    trace rows and both acceptance traces of every cut are those of ARP_SEGMENTS=1, bit for bit."""
    from autoreparam_amd import engine
    sp = helpers.spec("radon_PA")
    eng = engine.Engine(sp, gpu)
    eng.set_param(0, "CP"); eng.set_param(1, "NCP")
    q0 = helpers.states(sp, CHAINS, seed=2, scale=0.1)
    _set(monkeypatch, {"ARP_SEGMENTS": "1"})
    segs, ref = _radon_run(eng, sp, q0, gpu, T, thin, False)
    assert segs == 1 and np.isfinite(ref[0]).all() and ref[5].sum() > 0 and ref[9].sum() > 0
    for env, want in _cuts(T):
        _set(monkeypatch, env)
        segs, got = _radon_run(eng, sp, q0, gpu, T, thin, False)
        assert segs == want, (env, segs)
        for k, (x, y) in enumerate(zip(ref, got)):
            assert np.array_equal(x, y, equal_nan=True), (env, k)


@pytest.mark.gpu
def test_cuts_with_in_kernel_statistics(gpu, monkeypatch):
    """The same with the in-kernel statistics on: everything else bit for bit; the accumulators fold their partial batch
    where a segment ends, as they do where a launch ends, so the sums are the same numbers added in another grouping --
    float32 rounding of the sums, the bound test_relay_segments_equal_the_unsegmented_launch holds them to."""
    from autoreparam_amd import engine
    sp = helpers.spec("radon_PA")
    eng = engine.Engine(sp, gpu)
    eng.set_param(0, "CP"); eng.set_param(1, "NCP")
    q0 = helpers.states(sp, CHAINS, seed=2, scale=0.1)
    T, thin = 256, 2
    _set(monkeypatch, {"ARP_SEGMENTS": "1"})
    _, ref = _radon_run(eng, sp, q0, gpu, T, thin, True)
    n = ref[8].shape[0]
    for env, want in (({"ARP_SEGMENTS": "8"}, 8), ({"ARP_SEGMENTS": "8", "ARP_SEGMENT_RATIO": "50"}, 8),
                      ({"ARP_SEGMENT_LENS": "100,1,57,98"}, 4), ({"ARP_SEGMENT_LENS": "129,127"}, 2)):
        _set(monkeypatch, env)
        segs, got = _radon_run(eng, sp, q0, gpu, T, thin, True)
        assert segs == want, (env, segs)
        for k, (x, y) in enumerate(zip(ref[:11], got[:11])):
            assert np.array_equal(x, y, equal_nan=True), (env, k)
        for a_, b_ in zip(engine.stats_summary(torch.as_tensor(ref[11]), n, 3)[:2],
                          engine.stats_summary(torch.as_tensor(got[11]), n, 3)[:2]):
            scale = a_.abs().max(dim=0).values + 1e-3
            assert ((a_ - b_).abs() / scale).max() < 1e-5, env


@pytest.mark.gpu
@pytest.mark.parametrize("mname,kind,chains,lanes", [
    ("election", "NCP", 1030, 4),        # pk_hmc_kernel<ElectionPk<4,13>, NCP>: 17 chain blocks, the last ragged
    ("radon_sd_MN", "NCP", 523, 8),      # the generic hmc_kernel
])
def test_a_ragged_cut_in_a_packed_and_a_generic_kernel(gpu, monkeypatch, mname, kind, chains, lanes):
    from autoreparam_amd import engine, _lib
    sp = helpers.spec(mname)
    eng = engine.Engine(sp, gpu)
    eng.set_param(0, helpers.params(sp, kind, seed=3))
    q0 = helpers.states(sp, chains, seed=4, scale=0.05)
    e = np.full(sp.D, 2e-3, np.float32)
    T = 300

    def run(env):
        _set(monkeypatch, env)
        st = engine.ChainState(torch.as_tensor(q0, device=gpu))
        tr = torch.zeros(T, chains, sp.D, device=gpu)
        a0 = torch.zeros(T, chains, dtype=torch.uint8, device=gpu)
        for _ in range(2):
            eng.hmc_run(st, e, 3, T, seed=21, adapt_kind=_lib.ADAPT_DUAL, n_adapt=350, n_burnin=57, thin=2, trace=tr,
                        trace_accept=a0, lanes=lanes)
        torch.cuda.synchronize()
        eng.check()
        return eng.relay_geometry()["segments"], [t.cpu().numpy() for t in
                                                  (st.q, st.grad, st.logp, st.adapt, st.accept_count, st.rng, tr, a0)]

    segs, ref = run({"ARP_SEGMENTS": "1"})
    assert segs == 1 and np.isfinite(ref[0]).all() and ref[4].sum() > 0
    segs, got = run({"ARP_SEGMENT_LENS": "100,1,57,142"})
    assert segs == 4
    for k, (x, y) in enumerate(zip(ref, got)):
        assert np.array_equal(x, y, equal_nan=True), k


@pytest.mark.gpu
def test_a_list_that_is_not_the_launch_is_refused(gpu, monkeypatch):
    """ARP_SEGMENT_LENS that does not sum to n_steps (or is no list of lengths) is an error of the call; the state is untouched."""
    from autoreparam_amd import engine, _lib
    sp = helpers.spec("radon_PA")
    eng = engine.Engine(sp, gpu)
    eng.set_param(0, "CP"); eng.set_param(1, "NCP")
    q0 = helpers.states(sp, CHAINS, seed=2, scale=0.1)
    e = np.full(sp.D, 0.06, np.float32)
    for lens, what in (("100,100", "sum to 200"), ("200,57", "sum to 257"), ("256,0", "lengths >= 1"), ("128,x", "lengths >= 1")):
        _set(monkeypatch, {"ARP_SEGMENT_LENS": lens})
        st = engine.ChainState(torch.as_tensor(q0, device=gpu))
        with pytest.raises(RuntimeError, match=what):
            eng.interleaved_run(st, e, e, 4, 4, 256, seed=9, adapt_kind=_lib.ADAPT_SIMPLE, lanes=4)
        torch.cuda.synchronize()
        assert np.array_equal(st.q.cpu().numpy(), q0)


@pytest.mark.gpu
def test_a_forced_cut_and_the_record_belong_to_one_launch_of_one_thread(gpu, monkeypatch):
    """What a launch is asked to cut with travels with that call alone, and arp_relay_geometry is the calling thread's last
    chain launch.  radon PA interleaved, 32 768 chains at the default 4 lanes per chain: 512 chain blocks, one round of two
    resident workgroups per CU -- the smallest launch the library segments on its own (test_gpu_hmc.py: test_relay_rule).  An
    explicit cut gives 3 segments; the same launch without the switch gives the library's 4, the same bits; another thread's
    small launch on a handle of its own reports {1, its blocks, 0} there and leaves this thread's record alone; a launch of
    255 steps then stays whole."""
    import threading
    from autoreparam_amd import engine, _lib
    sp = helpers.spec("radon_PA")
    eng = engine.Engine(sp, gpu)
    eng.set_param(0, "CP"); eng.set_param(1, "NCP")
    chains = 32768
    q0 = helpers.states(sp, chains, seed=1, scale=0.05)
    e = np.full(sp.D, 1e-3, np.float32)

    def run(T):
        st = engine.ChainState(torch.as_tensor(q0, device=gpu))
        eng.interleaved_run(st, e, e, 1, 1, T, seed=1, adapt_kind=_lib.ADAPT_SIMPLE, n_adapt=0)
        torch.cuda.synchronize()
        eng.check()
        return eng.relay_geometry(), [t.cpu().numpy() for t in (st.q, st.grad, st.logp, st.adapt, st.adapt1, st.accept_count,
                                                                 st.accept_count1, st.rng)]

    _set(monkeypatch, {"ARP_SEGMENT_LENS": "100,100,100"})
    g, forced = run(300)
    assert g["segments"] == 3 and g["chain_blocks"] == 512
    _set(monkeypatch, {})
    g, own = run(300)
    assert g == {"segments": 4, "chain_blocks": 512, "workgroups_per_cu": 2}
    assert np.isfinite(own[0]).all() and own[5].sum() > 0
    for k, (x, y) in enumerate(zip(forced, own)):
        assert np.array_equal(x, y, equal_nan=True), k

    other = {}

    def small_launch():
        try:
            gsp = helpers.spec("german")
            geng = engine.Engine(gsp, gpu)                  # a handle of that thread's own
            with torch.cuda.stream(torch.cuda.Stream(device=gpu)):
                st = engine.ChainState(torch.as_tensor(helpers.states(gsp, 64, seed=2, scale=0.05), device=gpu))
                geng.hmc_run(st, np.full(gsp.D, 1e-3, np.float32), 1, 8, seed=2, lanes=4)
                torch.cuda.current_stream().synchronize()
            other["geometry"] = geng.relay_geometry()
        except Exception as exc:                            # noqa: BLE001 -- reported below, in the main thread
            other["error"] = repr(exc)

    t = threading.Thread(target=small_launch)
    t.start(); t.join(timeout=120)
    assert not t.is_alive() and "error" not in other, other
    assert other["geometry"] == {"segments": 1, "chain_blocks": 1, "workgroups_per_cu": 0}      # 64 chains x 4 lanes: one block
    assert eng.relay_geometry() == g

    g, _ = run(255)
    assert g["segments"] == 1 and g["chain_blocks"] == 512
