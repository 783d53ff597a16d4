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


def _fake_aligned(n_bytes, off=0):
    """The same with the address rounded up to 256 bytes (what the workspaces ask for), plus `off`."""
    buf = np.zeros(max(8, n_bytes) + 512, np.uint8)
    return buf, C.c_void_p(((buf.ctypes.data + 255) & ~255) + off)


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

    def workspace(need):
        """(pointer or None, bytes) as the `ess` kind draws them: absent, one byte short, whole; misaligned by 4"""
        ws_bytes = rnd.choice([0, max(0, need - 1), need, need])
        wsb, wsp = _fake_aligned(min(ws_bytes, 1 << 20), 4 if rnd.random() < 0.3 else 0)
        keepalive.append(wsb)
        return (wsp if ws_bytes else None), ws_bytes

    for it in range(4500):
        name = rnd.choice(MODELS)
        sp, h, _ = handles[name]
        hh = h if rnd.random() < 0.9 else C.c_void_p(0)
        kind = rnd.choice(["logp", "transform", "hmc", "inter", "vi", "ess", "adapt", "clock", "moments", "fold", "rank", "mcess"])
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
        elif kind in ("moments", "rank", "mcess"):
            S = rnd.choice([0, -3, 1, 7, 100, 1000, 50000, (1 << 21) + 2, 1 << 31, 10 ** 12])
            Cn = rnd.choice([0, -1, 1, 4, 64, 1 << 15, 1 << 31])
            D = rnd.choice([0, -2, 1, 7, 125, 300, 1 << 30])
            stride = rnd.choice([Cn * D, Cn * D - 1, 2 * Cn * D + 3])
            flag = rnd.choice([0, 1])                                  # split / fold
            if kind == "moments":
                need = L.arp_moments_workspace_bytes(S, Cn * D, flag)
                assert need >= 0
                wsp, ws_bytes = workspace(need)
                rc = L.arp_split_moments(ptr(), S, Cn * D, stride, flag, ptr(), ptr(), wsp, ws_bytes, None)
            elif kind == "rank":
                need = L.arp_rank_workspace_bytes(S, Cn, D, flag)
                assert need >= 0 and (need > 0 or len(err()) > 0)
                wsp, ws_bytes = workspace(need)
                n_probs = rnd.choice([0, 0, 2, -1])
                probs = (C.c_double * 2)(0.05, 0.95) if rnd.random() < 0.8 else None
                rc = L.arp_rank_normalize(ptr(), S, Cn, D, stride, flag, ptr(), ptr(0.3), ptr(0.5), probs, n_probs, ptr(0.7),
                                          wsp, ws_bytes, None)
            else:
                need = L.arp_ess_multichain_workspace_bytes(S, Cn, D, flag)
                assert need >= 0 and (need > 0 or len(err()) > 0)
                wsp, ws_bytes = workspace(need)
                rc = L.arp_ess_multichain(ptr(), S, Cn, D, stride, flag, ptr(0.3), ptr(), ptr(0.5), ptr(0.5),
                                          rnd.choice([0, 0, 3, -1]), wsp, ws_bytes, None)
        elif kind == "fold":
            rc = L.arp_moments_fold(ptr(), ptr(), rnd.choice([0, -1, 5, 1 << 40]), rnd.choice([0, -1, 1, 125]), ptr(), None)
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


# arp_*_workspace_bytes of the diagnostics by (S, C, D): rank, multichain (split 1, split 0), moments (n = C D, split 1),
# ess (n = C D).  A zero in the rank and multichain columns is a refusal (with a message).
DIAG_WORKSPACE_BYTES = {
    (1000, 4, 7): (238848, 3072, 2048, 2048, 0),
    (33, 9, 200): (886272, 450048, 230912, 0, 0),
    (50000, 16, 125): (825216512, 301568, 163840, 3211264, 410050304),
    (5, 1, 1): (2816, 1024, 1024, 0, 0),
    (65536, 32768, 5): (0, 0, 0, 335544320, 42954260736),
}


def test_diagnostics_refusals_and_workspace_sizes(host_lib, monkeypatch):
    """The diagnostics entry points (csrc/diag.hip, rank.hip, mcess.hip, ess.hip) on arguments they must refuse: which
    check fires and its exact words in arp_last_error(); and the workspace sizes they ask for.  A call that gets past
    validation fails, without a device, with HIP's own words (which quote the failing expression: not pinned)."""
    L = host_lib.lib()
    keep = []

    def p(n=1 << 12):
        b, ptr = _fake(n)
        keep.append(b)
        return ptr

    def ws(off=0):
        b, ptr = _fake_aligned(1 << 12, off)
        keep.append(b)
        return ptr

    for shape, (rank, mc1, mc0, mom, ess) in DIAG_WORKSPACE_BYTES.items():
        S, Cn, D = shape
        assert L.arp_rank_workspace_bytes(S, Cn, D, 0) == rank == L.arp_rank_workspace_bytes(S, Cn, D, 1), shape
        assert L.arp_ess_multichain_workspace_bytes(S, Cn, D, 1) == mc1, shape
        assert L.arp_ess_multichain_workspace_bytes(S, Cn, D, 0) == mc0, shape
        assert L.arp_moments_workspace_bytes(S, Cn * D, 1) == mom, shape
        assert L.arp_ess_workspace_bytes(S, Cn * D) == ess, shape
    assert L.arp_rank_workspace_bytes(65536, 32768, 5, 0) == 0
    assert L.arp_last_error() == b"arp_rank_workspace_bytes: at most 2^31 - 1 draws per element (n_samples * n_chains)"
    assert L.arp_ess_multichain_workspace_bytes(65536, 32768, 5, 1) == 0
    assert L.arp_last_error() == b"arp_ess_multichain_workspace_bytes: at most 2^31 - 1 draws per element (n_samples * n_chains)"

    S, Cn, D = 1000, 4, 7
    n = Cn * D
    RANK, MC = 238848, 3072                       # their workspaces at this shape (above)
    LS, LN = 50000, 2000                          # a trace of long series: the workspace routes of moments and ess
    MOM, ESS = 3211264, 410050304
    probs = (C.c_double * 2)(0.05, 0.95)

    def moments(trace=True, S_=S, n_=n, stride=None, w=None, wb=0):
        return L.arp_split_moments(p() if trace else None, S_, n_, n_ if stride is None else stride, 1, p(), p(), w, wb, None)

    def fold(mean=True, n_rows=8, D_=D, sums=True):
        return L.arp_moments_fold(p() if mean else None, p(), n_rows, D_, p() if sums else None, None)

    def rank(trace=True, shape=(S, Cn, D), stride=None, w="ok", wb=RANK, z=True, pr=None, n_probs=0, q=False):
        S_, C_, D_ = shape
        return L.arp_rank_normalize(p() if trace else None, S_, C_, D_, C_ * D_ if stride is None else stride, 0,
                                    p() if z else None, None, None, pr, n_probs, p() if q else None,
                                    ws() if w == "ok" else w, wb, None)

    def mcess(trace=True, shape=(S, Cn, D), stride=None, split=1, w="ok", wb=MC, ess=True, rho=False, n_rho=0):
        S_, C_, D_ = shape
        return L.arp_ess_multichain(p() if trace else None, S_, C_, D_, C_ * D_ if stride is None else stride, split, None,
                                    p() if ess else None, None, p() if rho else None, n_rho, ws() if w == "ok" else w, wb, None)

    def ess_ws(trace=True, S_=LS, n_=LN, stride=None, w=None, wb=0):
        return L.arp_ess_ws(p() if trace else None, S_, n_, n_ if stride is None else stride, p(), w, wb, None)

    MOMENTS_ARGS = b"arp_split_moments: trace/mean/var, n_samples > 0, n_series > 0 and row_stride >= n_series are required"
    FOLD_ARGS = b"arp_moments_fold: sums, D > 0, n_rows >= 0 and (with rows) mean/var are required"
    RANK_ARGS = b"arp_rank_normalize: trace, z and row_stride >= n_chains * D are required"
    MC_ARGS = b"arp_ess_multichain: trace, ess and row_stride >= n_chains * D are required"
    ESS_ARGS = b"arp_ess: trace/ess, n_samples > 0, n_series > 0 and row_stride >= n_series are required"
    SHAPE = b": n_samples > 0, n_chains > 0 and D > 0 are required"
    DRAWS = b": at most 2^31 - 1 draws per element (n_samples * n_chains)"
    VALUES = b": at most 2^35 values per call"
    RANK_SMALL = b"arp_rank_normalize: workspace too small (see arp_rank_workspace_bytes)"
    RANK_ALIGN = b"arp_rank_normalize: the workspace must be 256-byte aligned"
    MC_SMALL = b"arp_ess_multichain: workspace too small (see arp_ess_multichain_workspace_bytes)"
    MC_ALIGN = b"arp_ess_multichain: the workspace must be 256-byte aligned"
    MC_ROW = b"arp_ess_multichain: at most 2^20 draws per row (n_samples, or n_samples / 2 with split)"
    ESS_SMALL = b"arp_ess_ws: workspace too small (the work lists and at least 64 series rows: see arp_ess_workspace_bytes)"
    ESS_ALIGN = b"arp_ess_ws: the workspace must be 256-byte aligned"
    two31 = (1 << 31, 1, 1)
    two35 = (1 << 20, 1 << 10, 33)

    table = [
        # a null pointer
        ("moments null", lambda: moments(trace=False), MOMENTS_ARGS),
        ("fold null sums", lambda: fold(sums=False), FOLD_ARGS),
        ("fold null mean", lambda: fold(mean=False), FOLD_ARGS),
        ("rank null trace", lambda: rank(trace=False), RANK_ARGS),
        ("rank null z", lambda: rank(z=False), RANK_ARGS),
        ("mcess null trace", lambda: mcess(trace=False), MC_ARGS),
        ("mcess null ess", lambda: mcess(ess=False), MC_ARGS),
        ("ess null", lambda: ess_ws(trace=False), ESS_ARGS),
        # a short stride
        ("moments stride", lambda: moments(stride=n - 1), MOMENTS_ARGS),
        ("rank stride", lambda: rank(stride=n - 1), RANK_ARGS),
        ("mcess stride", lambda: mcess(stride=n - 1), MC_ARGS),
        ("ess stride", lambda: ess_ws(stride=LN - 1), ESS_ARGS),
        # a workspace too small, or none
        ("rank short ws", lambda: rank(wb=RANK - 1), RANK_SMALL),
        ("rank no ws", lambda: rank(w=None), RANK_SMALL),
        ("mcess short ws", lambda: mcess(wb=MC - 1), MC_SMALL),
        ("mcess no ws", lambda: mcess(w=None), MC_SMALL),
        ("ess short ws", lambda: ess_ws(w=ws(), wb=1024), ESS_SMALL),
        # a misaligned workspace; where it is also too small, which of the two is said
        ("rank misaligned", lambda: rank(w=ws(4)), RANK_ALIGN),
        ("rank misaligned + short", lambda: rank(w=ws(4), wb=RANK - 1), RANK_SMALL),
        ("mcess misaligned", lambda: mcess(w=ws(4)), MC_ALIGN),
        ("mcess misaligned + short", lambda: mcess(w=ws(4), wb=MC - 1), MC_SMALL),
        ("ess misaligned", lambda: ess_ws(w=ws(4), wb=ESS), ESS_ALIGN),
        ("ess misaligned + short", lambda: ess_ws(w=ws(4), wb=1024), ESS_ALIGN),
        ("moments misaligned", lambda: moments(S_=LS, n_=LN, w=ws(4), wb=MOM), b"arp_split_moments: the workspace must be 256-byte aligned"),
        # 2^31 draws per element, 2^35 values, 2^20 draws per row: before anything else, pointers included
        ("rank shape", lambda: rank(shape=(S, 0, D)), b"arp_rank_normalize" + SHAPE),
        ("mcess shape", lambda: mcess(shape=(S, Cn, -1)), b"arp_ess_multichain" + SHAPE),
        ("rank 2^31", lambda: rank(trace=False, shape=two31), b"arp_rank_normalize" + DRAWS),
        ("rank 2^31 product", lambda: rank(shape=(65536, 32768, 5)), b"arp_rank_normalize" + DRAWS),
        ("mcess 2^31", lambda: mcess(trace=False, shape=two31), b"arp_ess_multichain" + DRAWS),
        ("rank 2^35", lambda: rank(shape=two35, w=None), b"arp_rank_normalize" + VALUES),
        ("mcess 2^35", lambda: mcess(shape=two35, w=None), b"arp_ess_multichain" + VALUES),
        ("rank bytes 2^35", lambda: int(L.arp_rank_workspace_bytes(*two35, 0) == 0), b"arp_rank_workspace_bytes" + VALUES),
        ("mcess bytes 2^35", lambda: int(L.arp_ess_multichain_workspace_bytes(*two35, 1) == 0),
         b"arp_ess_multichain_workspace_bytes" + VALUES),
        ("mcess 2^20 split", lambda: mcess(trace=False, shape=((1 << 21) + 2, 4, 7)), MC_ROW),
        ("mcess 2^20 whole", lambda: mcess(shape=((1 << 20) + 1, 4, 7), split=0), MC_ROW),
        ("mcess bytes 2^20", lambda: int(L.arp_ess_multichain_workspace_bytes((1 << 20) + 1, 4, 7, 0) == 0),
         b"arp_ess_multichain_workspace_bytes: at most 2^20 draws per row (n_samples, or n_samples / 2 with split)"),
        ("mcess 2^20 draws per row fit", lambda: mcess(shape=((1 << 21) + 1, 1, 1), w=None), MC_SMALL),
        ("moments 2^30", lambda: moments(n_=1 << 30), b"arp_split_moments: at most 2^30 - 1 series per call"),
        ("ess 2^30", lambda: ess_ws(n_=1 << 30), b"arp_ess: at most 2^30 - 1 series per call (32-bit lane offsets)"),
        # n_rho without rho; quantiles without probs (after the pointers, before the workspace)
        ("mcess n_rho", lambda: mcess(n_rho=3, w=None), b"arp_ess_multichain: n_rho >= 0, and rho where n_rho > 0"),
        ("mcess n_rho < 0", lambda: mcess(rho=True, n_rho=-1), b"arp_ess_multichain: n_rho >= 0, and rho where n_rho > 0"),
        ("mcess n_rho, null trace", lambda: mcess(trace=False, n_rho=3), MC_ARGS),
        ("rank probs", lambda: rank(q=True, n_probs=2, w=None), b"arp_rank_normalize: quantiles need n_probs >= 0 and probs"),
        # arp_moments_fold with D = 0
        ("fold D = 0", lambda: fold(D_=0), FOLD_ARGS),
        ("fold n_rows < 0", lambda: fold(n_rows=-1), FOLD_ARGS),
        # past validation: no device
        ("moments", lambda: moments(), None),
        ("moments, long route", lambda: moments(S_=LS, n_=LN, w=ws(), wb=MOM), None),
        ("moments, workspace too small: the wide route", lambda: moments(S_=LS, n_=LN, w=ws(), wb=MOM - 1), None),
        ("fold", lambda: fold(), None),
        ("fold, no rows", lambda: fold(mean=False, n_rows=0), None),
        ("rank", lambda: rank(pr=probs, n_probs=2, q=True), None),
        ("mcess", lambda: mcess(rho=True, n_rho=3), None),
        ("mcess, three draws per row", lambda: mcess(shape=(7, 4, 7)), None),
        ("ess", lambda: ess_ws(S_=S, n_=n), None),
        ("ess, workspace", lambda: ess_ws(w=ws(), wb=ESS), None),
        ("ess, long series without a workspace", lambda: ess_ws(), None),
    ]
    for what, call, message in table:
        rc = call()
        got = L.arp_last_error()
        assert rc != 0 and len(got) > 0, what
        if message is not None:
            assert got == message, (what, got)
        del keep[:]
    # the long route of arp_split_moments forced (an experiment switch): only then is a workspace too small refused
    monkeypatch.setenv("ARP_MOMENTS_ROUTE", "long")
    assert moments(S_=LS, n_=LN, w=ws(), wb=MOM - 1) != 0
    assert L.arp_last_error() == b"arp_split_moments: workspace too small (see arp_moments_workspace_bytes)"
    assert moments(S_=LS, n_=LN, w=ws(4), wb=MOM - 1) != 0
    assert L.arp_last_error() == b"arp_split_moments: workspace too small (see arp_moments_workspace_bytes)"
