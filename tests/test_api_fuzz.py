"""CPU: argument validation of every arp_* entry point, driven without a GPU.

Under ARP_DEBUG=1 ARP_HOST_ONLY=1 (a test hook of csrc/arp_api.hip that announces itself) arp_model_create builds a
handle whose tables live in host memory, so the host side of the library -- sufficient statistics, lane selection,
argument checks, work-list and workspace sizing -- runs here for every model.  Nothing can be computed with such a
handle: a call that gets past validation fails with HIP's own "no device" error.  The property held over a few thousand
randomised calls: NEVER a crash, and every call either returns 0 for a documented no-op (n_steps == 0) or returns
non-zero with a message in arp_last_error()."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_lib():
    import torch
    if torch.cuda.is_available():
        # with a device present a call that passes validation would LAUNCH on the stand-in pointers
        pytest.skip("argument fuzzing with host-only handles runs on GPU-less machines only")
    import __graft_entry__ as ge
    ge.build()
    from autoreparam_amd import _lib
    old = {k: os.environ.get(k) for k in ("ARP_DEBUG", "ARP_HOST_ONLY")}
    os.environ["ARP_DEBUG"] = "1"
    os.environ["ARP_HOST_ONLY"] = "1"
    yield _lib
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _handle(_lib, name):
    sp = helpers.spec(name)
    ds, keep = sp.dataset()
    h = C.c_void_p(0)
    rc = _lib.lib().arp_model_create(C.byref(ds), C.byref(h))
    assert rc == 0, _lib.lib().arp_last_error()
    return sp, h, keep


MODELS = ["8schools", "radon_MN", "radon_PA", "election", "german", "radon_sd_MN", "funnel", "electric", "time_series"]


@pytest.mark.parametrize("name", MODELS)
def test_host_only_handles_build_and_validate(host_lib, name):
    L = host_lib.lib()
    sp, h, keep = _handle(host_lib, name)
    assert L.arp_model_dim(h) == sp.D
    assert np.isfinite(L.arp_model_logp_const(h, 0))
    a = np.full(sp.D, 0.5, np.float32)
    f32p = host_lib._f32p
    assert L.arp_model_set_param(h, 0, a.ctypes.data_as(f32p), a.ctypes.data_as(f32p)) == 0
    assert L.arp_model_set_param(h, 2, a.ctypes.data_as(f32p), a.ctypes.data_as(f32p)) != 0
    assert L.arp_model_set_param(h, 0, None, a.ctypes.data_as(f32p)) != 0
    # options: german_math on german credit only (the reference's data have 7 columns that need three bf16 pieces: every
    # value is accepted); unknown keys, values, NULLs and other models fail with a message
    if name == "german":
        for v in (b"f32", b"bf16x3", b"auto"):
            assert L.arp_model_set_option(h, b"german_math", v) == 0
        assert L.arp_model_set_option(h, b"german_math", b"fp8") != 0 and b"german_math" in L.arp_last_error()
    else:
        assert L.arp_model_set_option(h, b"german_math", b"f32") != 0
    assert L.arp_model_set_option(h, b"no_such_key", b"1") != 0 and len(L.arp_last_error()) > 0
    assert L.arp_model_set_option(h, None, b"1") != 0 and L.arp_model_set_option(None, b"german_math", b"f32") != 0
    assert L.arp_model_destroy(h) == 0


def _fake(n_bytes):
    """An address range of our own to hand over as a `device` pointer (never dereferenced: no launch succeeds)."""
    buf = np.zeros(max(8, n_bytes), np.uint8)
    return buf, C.c_void_p(buf.ctypes.data)


def test_randomised_calls_never_crash_and_always_explain(host_lib):
    L = host_lib.lib()
    rnd = random.Random(20261002)
    handles = {n: _handle(host_lib, n) for n in MODELS}
    calls = failures = 0
    keepalive = []

    def ptr(ok_p=0.8, n=1 << 16):
        if rnd.random() < ok_p:
            b, p = _fake(n)
            keepalive.append(b)
            return p
        return C.c_void_p(0)

    def err():
        return L.arp_last_error()

    for it in range(3000):
        name = rnd.choice(MODELS)
        sp, h, _ = handles[name]
        hh = h if rnd.random() < 0.9 else C.c_void_p(0)
        kind = rnd.choice(["logp", "transform", "hmc", "inter", "vi", "ess", "adapt", "clock"])
        del keepalive[:]
        L.arp_model_set_param(h, 0, np.ones(sp.D, np.float32).ctypes.data_as(host_lib._f32p),
                              np.ones(sp.D, np.float32).ctypes.data_as(host_lib._f32p))
        if kind == "logp":
            rc = L.arp_logp_grad(hh, rnd.choice([0, 1, -1, 2]), ptr(), rnd.choice([0, -5, 1, 7, 4096]), ptr(), ptr(),
                                 rnd.choice([0, 1, 2, 3, 4, 8, 16, 32, -1]), None)
        elif kind == "transform":
            rc = L.arp_transform(hh, rnd.choice([0, 1, 5]), rnd.choice([0, 1, 2, -1]), ptr(), rnd.choice([0, 1, 100]), ptr(), None)
        elif kind in ("hmc", "inter"):
            cfg = host_lib.HmcConfig()
            cfg.n_chains = rnd.choice([0, -1, 1, 64, 70, 4096])
            cfg.n_leapfrog = rnd.choice([0, 1, 4, -2])
            cfg.n_steps = rnd.choice([-1, 0, 1, 16])
            cfg.step_base = rnd.choice([0, 5, -1])
            cfg.adapt_kind = rnd.choice([0, 1, 2, 3, -1])
            cfg.n_adapt = rnd.choice([0, 10])
            cfg.adapt_target = rnd.choice([0.75, 0.0, 1.0, 1.5, -0.1])
            cfg.adapt_rate = rnd.choice([0.05, 0.0, -1.0])
            cfg.thin = rnd.choice([0, 1, 2, -1])
            cfg.n_samples = rnd.choice([0, 10])
            cfg.lanes_per_chain = rnd.choice([0, 1, 2, 4, 8, 16, 3, 64, -4])
            cfg.stats_batch = rnd.choice([0, 1, 8, -1])
            cfg.trace_chains = rnd.choice([0, 1, 10 ** 6, -3])        # more than n_chains: clamped, never an overrun
            io = host_lib.HmcIO()
            io.q, io.grad, io.logp, io.adapt = ptr(), ptr(), ptr(), ptr()
            io.rng, io.accept_count, io.eps0 = ptr(), ptr(), ptr()
            io.trace, io.trace_accept, io.stats, io.rec_accept_count = ptr(0.3), ptr(0.3), ptr(0.3), ptr(0.3)
            if kind == "hmc":
                rc = L.arp_hmc_run(hh, rnd.choice([0, 1, 2]), C.byref(cfg) if rnd.random() < 0.95 else None,
                                   C.byref(io) if rnd.random() < 0.95 else None, None)
                if rc == 0:
                    assert cfg.n_steps == 0, "a launch cannot have succeeded without a device"
            else:
                io2 = host_lib.InterleavedIO()
                io2.k0 = io
                io2.adapt1, io2.accept_count1, io2.eps0_1 = ptr(), ptr(), ptr()
                io2.trace_accept1, io2.rec_accept_count1 = ptr(0.3), ptr(0.3)
                rc = L.arp_interleaved_run(hh, C.byref(cfg), rnd.choice([0, 4, -1]), C.byref(io2), None)
                if rc == 0:
                    assert cfg.n_steps == 0
        elif kind == "vi":
            cfg = host_lib.ViConfig()
            cfg.n_lr = rnd.choice([0, 1, 5, -1, 600])
            cfg.n_steps = rnd.choice([0, 1, 100])
            cfg.n_mc = rnd.choice([0, 1, 37, 256, 4096, 4097, -8])
            cfg.learn_a = rnd.choice([0, 1])
            cfg.tied_b = rnd.choice([0, 1])
            cfg.a_prior = rnd.choice([0, 1])
            io = host_lib.ViIO()
            io.lr, io.loc, io.rho, io.w, io.wb = ptr(), ptr(), ptr(), ptr(0.5), ptr(0.3)
            io.elbo, io.prior = ptr(), ptr(0.3)
            rc = L.arp_vi_run(hh, rnd.choice([0, 1, 3]), C.byref(cfg), C.byref(io), None)
        elif kind == "ess":
            S = rnd.choice([0, 1, 100, 2300, 5000, 10 ** 7])
            n = rnd.choice([0, 1, 25, 64, 1000, 1 << 31])
            need = L.arp_ess_workspace_bytes(S, n)
            assert need >= 0
            ws_bytes = rnd.choice([0, 1024, max(0, need - 64), need])
            wsb, wsp = _fake(min(ws_bytes, 1 << 20))
            keepalive.append(wsb)
            if rnd.random() < 0.3:
                wsp = C.c_void_p(wsp.value + 4)                        # misaligned workspace
            rc = L.arp_ess_ws(ptr(), S, n, rnd.choice([n, n - 1, 2 * n + 3]), ptr(),
                              wsp if ws_bytes else None, ws_bytes, None)
        elif kind == "adapt":
            cfg = host_lib.HmcConfig()
            cfg.n_steps = rnd.choice([-1, 0, 4])
            cfg.adapt_kind = rnd.choice([0, 1, 2, 7])
            cfg.adapt_target = rnd.choice([0.75, 2.0])
            cfg.adapt_rate = rnd.choice([0.05, -0.5])
            rc = L.arp_adapt_probe(C.byref(cfg), ptr(), rnd.choice([0, 3]), ptr(), ptr(0.5), None)
        else:
            rc = L.arp_clock_probe(rnd.choice([0, -1, 5]), ptr(0.5), ptr(0.5))
        calls += 1
        if rc != 0:
            failures += 1
            assert len(err()) > 0, (kind, name)
    assert failures >= 0.95 * calls            # all but the n_steps == 0 no-ops
    for n_, (sp, h, _) in handles.items():
        assert L.arp_model_destroy(h) == 0


# (a, b) of the four parameterisation kinds arp_model_set_param tells apart: centred, non-centred, "a free, b = 1", general
PARAM_KINDS = [(1.0, 1.0), (0.0, 0.0), (0.5, 1.0), (0.5, 0.5)]
# chain launches test_every_launcher_table_slot_is_filled makes: per model, over lanes_per_chain 0 / 4 / 8 / 16 where the
# family has an instantiation for the test dataset.  Counted on the commit before the launcher tables were split (where
# the same walk passes) and unchanged by the split: 6 per served lanes_per_chain.
TABLE_WALK_CALLS = {"8schools": 18, "radon_MN": 24, "radon_PA": 24, "election": 24, "german": 24, "radon_sd_MN": 18,
                    "funnel": 6, "electric": 18, "time_series": 24}     # 180 in all


@pytest.mark.parametrize("name", MODELS)
def test_every_launcher_table_slot_is_filled(host_lib, name):
    """Every chain slot of the launcher table an instantiation exports (csrc/host_common.h: LaneOps::hmc by the four
    parameterisation kinds, LaneOps::interleaved by (CP, NCP) pair or any other) is called once through the C API, with
    one step.  Without a device each call must come back with HIP's own launch error: an empty slot would be a call
    through a null pointer, a validation message would mean the slot was never reached."""
    L = host_lib.lib()
    sp, h, keep = _handle(host_lib, name)
    f32p = host_lib._f32p
    bufs = []

    def ptr():
        b, p = _fake(1 << 16)
        bufs.append(b)
        return p

    def set_param(which, ab):
        a, b = (np.full(sp.D, v, np.float32) for v in ab)
        assert L.arp_model_set_param(h, which, a.ctypes.data_as(f32p), b.ctypes.data_as(f32p)) == 0

    def launched(rc, what):
        err = L.arp_last_error()
        assert rc != 0 and err.startswith(b"launched: ") and len(err) > len(b"launched: "), (what, rc, err)

    cfg = host_lib.HmcConfig()
    cfg.n_chains, cfg.n_leapfrog, cfg.n_steps, cfg.thin, cfg.stats_batch = 64, 2, 1, 1, 1
    io = host_lib.HmcIO()
    io.q, io.grad, io.logp, io.adapt, io.rng, io.accept_count, io.eps0 = (ptr() for _ in range(7))
    io2 = host_lib.InterleavedIO()
    io2.k0 = io
    io2.adapt1, io2.accept_count1, io2.eps0_1 = ptr(), ptr(), ptr()
    calls = 0
    for K in (0, 4, 8, 16):
        cfg.lanes_per_chain = K
        set_param(0, PARAM_KINDS[0])
        if L.arp_hmc_run(h, 0, C.byref(cfg), C.byref(io), None) != 0 and L.arp_last_error().startswith(b"no kernel instantiation"):
            assert K != 0, "every family serves its default lanes per chain"
            continue
        for ab in PARAM_KINDS:
            set_param(0, ab)
            launched(L.arp_hmc_run(h, 0, C.byref(cfg), C.byref(io), None), ("hmc", K, ab))
            calls += 1
        for ab0, ab1 in ((PARAM_KINDS[0], PARAM_KINDS[1]), (PARAM_KINDS[3], PARAM_KINDS[3])):
            set_param(0, ab0)
            set_param(1, ab1)
            launched(L.arp_interleaved_run(h, C.byref(cfg), 2, C.byref(io2), None), ("interleaved", K, ab0, ab1))
            calls += 1
    print("%s: %d chain launches" % (name, calls))
    assert calls == TABLE_WALK_CALLS[name]
    assert L.arp_model_destroy(h) == 0


_LISTING = """\
\t.type\t_Zgone,@function
_Zgone:                                 ; @_Zgone
\ts_branch .LBB0_1
.LBB0_1:
\ts_endpgm
.Lfunc_end0:
\t.type\t_Zkept,@function
_Zkept:                                 ; @_Zkept
; %bb.0:
\ts_cbranch_scc1 .LBB1_2
\ts_getpc_b64 s[0:1]
.Ltmp7:
\ts_add_u32 s0, s0, .LBB1_2-.Ltmp7
.LBB1_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel _Zkept
\t\t.amdhsa_group_segment_fixed_size 1024
\t\t.amdhsa_next_free_vgpr 20
\t.end_amdhsa_kernel
\t.text
.Lfunc_end1:
\t.size\t_Zkept, .Lfunc_end1-_Zkept
\t.type\t_Zedited,@function
_Zedited:
\tv_add_f32_e32 v0, v1, v2
\ts_endpgm
.Lfunc_end2:
\t.type\tsome_table,@object
some_table:
\t.long\t1
"""


def test_listing_diff_by_kernel_sees_through_renumbered_labels():
    """tools/listing_diff.py --by-kernel on two hand-written listings: this tree's lost its first function, which
    renumbers the local labels of the next (and its `.Ltmp`), and has one instruction changed in the third -- one function
    only in the parent, one differing, one equal.  A changed descriptor line alone makes a kernel differ too."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("listing_diff", os.path.join(ROOT, "tools", "listing_diff.py"))
    ld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ld)
    this = _LISTING[_LISTING.index("\t.type\t_Zkept"):]
    for old, new in ((".LBB1_", ".LBB0_"), (".Lfunc_end1", ".Lfunc_end0"), (".Lfunc_end2", ".Lfunc_end1"), (".Ltmp7", ".Ltmp3"),
                     ("v_add_f32_e32 v0, v1, v2", "v_add_f32_e32 v0, v2, v1")):
        assert old in this
        this = this.replace(old, new)
    assert set(ld.cut_functions(_LISTING)) == {"_Zgone", "_Zkept", "_Zedited"}
    assert ld.cut_functions(_LISTING)["_Zkept"][1] == (".amdhsa_group_segment_fixed_size 1024", ".amdhsa_next_free_vgpr 20")
    assert ld.by_kernel(_LISTING, this) == (["_Zgone"], [], ["_Zedited"], ["_Zkept"])
    assert ld.by_kernel(this, _LISTING) == ([], ["_Zgone"], ["_Zedited"], ["_Zkept"])
    lds = this.replace("fixed_size 1024", "fixed_size 2048")
    assert ld.by_kernel(this, lds) == ([], [], ["_Zkept"], ["_Zedited"])


def test_ess_workspace_size_is_a_whole_number_of_row_blocks(host_lib):
    """include/autoreparam.h: arp_ess_workspace_bytes sizes the workspace at which every listed series fits at once --
    64-row blocks, at least one (a single german-credit chain has 125 series, one parameter block of it 25)."""
    L = host_lib.lib()
    assert L.arp_ess_workspace_bytes(1000, 10 ** 6) == 0
    for S in (2400, 5000, 50000):
        sizes = [L.arp_ess_workspace_bytes(S, n) for n in (1, 25, 63, 64, 65, 128)]
        assert sizes[0] > 64 * 4 * S                                   # one whole 64-row block even for one series
        assert sizes[4] - sizes[3] >= 64 * 4 * S                       # the 65th series opens a second block
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
