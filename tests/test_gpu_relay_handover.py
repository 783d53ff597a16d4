"""The relay's hand-over forms (kernels.h: relay_begin / relay_end; relay_host.h: ARP_RELAY_PUBLISH, ARP_RELAY_ACQUIRE):
the release-fence and the write-through publish, the per-wave and the per-workgroup acquire, in all four combinations, against
the launch with one workgroup per chain block -- bit for bit.  The launches are short (64 steps) and cut 1,1,30,1,31, so that
some hand-overs follow each other directly; two launches in a row, so that the second starts from handed-over state."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers

T = 64
LENS = "1,1,30,1,31"
FORMS = [(p, a) for p in ("fence", "through") for a in ("wave", "group")]
_SWITCHES = ("ARP_SEGMENTS", "ARP_SEGMENT_RATIO", "ARP_SEGMENT_LENS", "ARP_RELAY_PUBLISH", "ARP_RELAY_ACQUIRE")


def _set(monkeypatch, env):
    monkeypatch.setenv("ARP_DEBUG", "1")
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _cut(publish, acquire):
    return {"ARP_SEGMENT_LENS": LENS, "ARP_RELAY_PUBLISH": publish, "ARP_RELAY_ACQUIRE": acquire}


def _run(eng, sp, q0, gpu, sampler, lanes, e, with_stats=False, with_rec=False):
    """two launches of T steps; the segments of the last one and every array the launches wrote: q, grad, logp, both adapt
    arrays, both counters, the generator state, the trace, both acceptance traces (then statistics / recorded counters)"""
    from autoreparam_amd import engine, _lib
    chains = q0.shape[0]
    st = engine.ChainState(torch.as_tensor(q0, device=gpu))
    n_burn, thin = 5, 2
    S = (2 * T - n_burn - 1) // thin + 1
    tr = torch.zeros(S, chains, sp.D, device=gpu)
    a0 = torch.zeros(S, chains, dtype=torch.uint8, device=gpu); a1 = torch.zeros_like(a0)
    extra = {}
    if with_stats:
        extra.update(stats=torch.zeros(6, chains, sp.D, device=gpu), stats_batch=3, n_samples=S)
    r0 = torch.zeros(chains, dtype=torch.int32, device=gpu); r1 = torch.zeros_like(r0)
    for _ in range(2):
        if sampler == "hmc":
            if with_rec:
                extra.update(rec_accept=r0)
            eng.hmc_run(st, e, 3, T, seed=21, adapt_kind=_lib.ADAPT_DUAL, n_adapt=90, n_burnin=n_burn, thin=thin, trace=tr,
                        trace_accept=a0, lanes=lanes, **extra)
        else:
            if with_rec:
                extra.update(rec_accept0=r0, rec_accept1=r1)
            eng.interleaved_run(st, e, e, 4, 4, T, seed=9, adapt_kind=_lib.ADAPT_SIMPLE, n_adapt=90, n_burnin=n_burn, thin=thin,
                                trace=tr, trace_accept0=a0, trace_accept1=a1, trace_centered=False, lanes=lanes, **extra)
    torch.cuda.synchronize()
    eng.check()
    out = [st.q, st.grad, st.logp, st.adapt, st.adapt1, st.accept_count, st.accept_count1, st.rng, tr, a0, a1, r0, r1]
    if with_stats:
        out.append(extra["stats"])
    return eng.relay_geometry()["segments"], [t.cpu().numpy() for t in out]


def _case(mname, sampler, kind, chains, gpu):
    from autoreparam_amd import engine
    sp = helpers.spec(mname)
    eng = engine.Engine(sp, gpu)
    if sampler == "hmc":
        eng.set_param(0, helpers.params(sp, kind, seed=3))
    else:
        eng.set_param(0, "CP"); eng.set_param(1, "NCP")
    q0 = helpers.states(sp, chains, seed=2, scale=0.1 if mname == "radon_PA" else 0.05)
    if mname == "radon_PA":
        e = np.full(sp.D, 0.06, np.float32); e[2] = 0.015
    else:
        e = np.full(sp.D, 2e-3, np.float32)
    return sp, eng, q0, e


@pytest.mark.gpu
@pytest.mark.parametrize("mname,sampler,kind,chains,lanes", [
    ("radon_PA", "interleaved", None, 1000, 4),      # radon_interleaved_kernel: 16 chain blocks, a ragged last wave
    ("radon_PA", "interleaved", None, 130, 4),       # a partial last block
    ("radon_PA", "interleaved", None, 4097, 8),      # 8 lanes per chain (padding slices), one chain in the last block
    ("electric", "interleaved", None, 520, 0),       # the generic interleaved_kernel
    ("election", "hmc", "NCP", 1000, 4),             # pk_hmc_kernel<ElectionPk<4,13>, NCP>
])
def test_every_hand_over_form_equals_the_unsegmented_launch(gpu, monkeypatch, mname, sampler, kind, chains, lanes):
    sp, eng, q0, e = _case(mname, sampler, kind, chains, gpu)
    _set(monkeypatch, {"ARP_SEGMENTS": "1"})
    segs, ref = _run(eng, sp, q0, gpu, sampler, lanes, e)
    assert segs == 1 and np.isfinite(ref[0]).all() and ref[5].sum() > 0 and ref[9].sum() > 0
    for publish, acquire in FORMS:
        _set(monkeypatch, _cut(publish, acquire))
        segs, got = _run(eng, sp, q0, gpu, sampler, lanes, e)
        assert segs == 5, (publish, acquire, segs)
        for k, (x, y) in enumerate(zip(ref, got)):
            assert np.array_equal(x, y, equal_nan=True), (publish, acquire, k)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["stats", "rec_accept"])
def test_write_through_asked_with_planes_or_counters_takes_the_fence_form(gpu, monkeypatch, what):
    """Statistics planes and rec_accept counters are read-modify-written inside the step loop with plain stores, so a launch
    with either keeps the release fence whatever ARP_RELAY_PUBLISH asks (kernels.h: relay_through): everything bit for bit the
    unsegmented launch's, the statistics to the float32 rounding of sums added in another grouping (the bound
    test_relay_segments_equal_the_unsegmented_launch holds them to)."""
    from autoreparam_amd import engine
    sp, eng, q0, e = _case("radon_PA", "interleaved", None, 1000, gpu)
    kw = dict(with_stats=what == "stats", with_rec=what == "rec_accept")
    _set(monkeypatch, {"ARP_SEGMENTS": "1"})
    segs, ref = _run(eng, sp, q0, gpu, "interleaved", 4, e, **kw)
    assert segs == 1 and np.isfinite(ref[0]).all()
    if what == "rec_accept":
        assert ref[11].sum() > 0 and ref[12].sum() > 0
    for acquire in ("wave", "group"):
        _set(monkeypatch, _cut("through", acquire))
        segs, got = _run(eng, sp, q0, gpu, "interleaved", 4, e, **kw)
        assert segs == 5
        for k, (x, y) in enumerate(zip(ref[:13], got[:13])):
            assert np.array_equal(x, y, equal_nan=True), (acquire, k)
        if what == "stats":
            n = ref[8].shape[0]
            for a_, b_ in zip(engine.stats_summary(torch.as_tensor(ref[13]), n, 3)[:2],
                              engine.stats_summary(torch.as_tensor(got[13]), n, 3)[:2]):
                scale = a_.abs().max(dim=0).values + 1e-3
                assert ((a_ - b_).abs() / scale).max() < 1e-5, acquire


@pytest.mark.gpu
def test_an_unknown_form_is_refused(gpu, monkeypatch):
    """ARP_RELAY_PUBLISH / ARP_RELAY_ACQUIRE set to something else is an error of the call; the state is untouched."""
    from autoreparam_amd import _lib
    sp, eng, q0, e = _case("radon_PA", "interleaved", None, 130, gpu)
    from autoreparam_amd import engine
    for env, what in (({"ARP_RELAY_PUBLISH": "sc1"}, "ARP_RELAY_PUBLISH"), ({"ARP_RELAY_ACQUIRE": "block"}, "ARP_RELAY_ACQUIRE"),
                      ({"ARP_RELAY_PUBLISH": "through", "ARP_RELAY_ACQUIRE": "Group"}, "ARP_RELAY_ACQUIRE")):
        _set(monkeypatch, dict(env, ARP_SEGMENT_LENS=LENS))
        st = engine.ChainState(torch.as_tensor(q0, device=gpu))
        with pytest.raises(RuntimeError, match=what):
            eng.interleaved_run(st, e, e, 4, 4, T, seed=9, adapt_kind=_lib.ADAPT_SIMPLE, lanes=4)
        torch.cuda.synchronize()
        assert np.array_equal(st.q.cpu().numpy(), q0) and not st.rng.any()


def test_an_unknown_form_is_refused_without_a_device(monkeypatch):
    """The same through a handle without a device (the argument-validation hook of arp_api.hip): the switches are read before
    anything is allocated or launched, so the call fails with their message, and the arrays it was given are untouched."""
    if torch.cuda.is_available():
        pytest.skip("host-only handles are for machines without a GPU: with one, a call that passes would launch on host memory")
    import __graft_entry__ as ge
    ge.build()
    from autoreparam_amd import _lib
    _set(monkeypatch, {"ARP_HOST_ONLY": "1"})
    L = _lib.lib()
    sp = helpers.spec("radon_PA")
    ds, keep = sp.dataset()
    h = C.c_void_p(0)
    assert L.arp_model_create(C.byref(ds), C.byref(h)) == 0, L.arp_last_error()
    a, b = sp.ab_from_reparam("CP")
    assert L.arp_model_set_param(h, 0, a.ctypes.data_as(_lib._f32p), b.ctypes.data_as(_lib._f32p)) == 0
    a1, b1 = sp.ab_from_reparam("NCP")
    assert L.arp_model_set_param(h, 1, a1.ctypes.data_as(_lib._f32p), b1.ctypes.data_as(_lib._f32p)) == 0
    chains = 130
    bufs = {"q": np.ones((chains, sp.D), np.float32), "grad": np.zeros((chains, sp.D), np.float32),
            "logp": np.zeros(chains, np.float32), "adapt": np.zeros((chains, 4), np.float32),
            "adapt1": np.zeros((chains, 4), np.float32), "rng": np.zeros((chains, _lib.RNG_SLOTS, 4), np.int32),
            "acc": np.zeros(chains, np.int32), "acc1": np.zeros(chains, np.int32), "eps": np.full(sp.D, 0.01, np.float32)}
    before = {k: v.copy() for k, v in bufs.items()}
    p = {k: v.ctypes.data for k, v in bufs.items()}      # host memory stands in for the device's: nothing gets to a launch
    cfg = _lib.HmcConfig()
    cfg.n_chains, cfg.n_leapfrog, cfg.n_steps, cfg.lanes_per_chain, cfg.thin = chains, 4, T, 4, 1
    cfg.adapt_kind, cfg.adapt_target, cfg.adapt_rate = _lib.ADAPT_SIMPLE, 0.75, 0.05
    io = _lib.InterleavedIO()
    for name, key in (("q", "q"), ("grad", "grad"), ("logp", "logp"), ("adapt", "adapt"), ("rng", "rng"),
                      ("accept_count", "acc"), ("eps0", "eps")):
        setattr(io.k0, name, p[key])
    io.adapt1, io.accept_count1, io.eps0_1 = p["adapt1"], p["acc1"], p["eps"]
    for env, what in (({"ARP_RELAY_PUBLISH": "sc1"}, b"ARP_RELAY_PUBLISH"), ({"ARP_RELAY_ACQUIRE": "block"}, b"ARP_RELAY_ACQUIRE")):
        _set(monkeypatch, dict(env, ARP_HOST_ONLY="1", ARP_SEGMENT_LENS=LENS))
        assert L.arp_interleaved_run(h, C.byref(cfg), 4, C.byref(io), None) != 0
        assert what in L.arp_last_error(), L.arp_last_error()
        for k, v in bufs.items():
            assert np.array_equal(v, before[k]), k
    assert L.arp_model_destroy(h) == 0
    del keep
