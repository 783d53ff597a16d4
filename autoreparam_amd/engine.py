"""Device-side handle around the C ABI: one Engine per (process, GPU, model).

torch is used only for device memory and streams; every number on the hot path is
produced by the HIP kernels in libautoreparam_hip.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


class ChainState(object):
    """Per-chain persistent state of a run (the reference's kernel_results)."""

    def __init__(self, q):
        C_, D = q.shape
        dev = q.device
        self.q = q.contiguous().clone()
        self.grad = torch.zeros_like(self.q)
        self.logp = torch.zeros(C_, dtype=torch.float32, device=dev)
        self.adapt = torch.zeros(C_, 4, dtype=torch.float32, device=dev)
        self.rng = torch.zeros(C_, _lib.RNG_SLOTS, 4, dtype=torch.int32, device=dev)
        self.accept_count = torch.zeros(C_, dtype=torch.int32, device=dev)
        # second inner kernel of the interleaved sampler
        self.adapt1 = torch.zeros(C_, 4, dtype=torch.float32, device=dev)
        self.accept_count1 = torch.zeros(C_, dtype=torch.int32, device=dev)
        self.step = 0  # transitions done


def _hmc_config(state, n_leapfrog, n_steps, seed, chain_offset, adapt_kind, n_adapt, adapt_target, adapt_rate, n_burnin,
                thin, trace, trace_accept, trace_centered, lanes, stats_batch, n_samples, trace_chains):
    """The arp_hmc_config of one launch (Engine.hmc_run, Engine.interleaved_run).  `n_samples` falls back to the rows of
    whichever recording buffer is given."""
    cfg = _lib.HmcConfig()
    cfg.n_chains, cfg.n_leapfrog, cfg.n_steps, cfg.step_base = state.q.shape[0], int(n_leapfrog), int(n_steps), int(state.step)
    cfg.chain_offset, cfg.seed, cfg.lanes_per_chain = int(chain_offset), int(seed), int(lanes)
    cfg.adapt_kind, cfg.n_adapt, cfg.adapt_target, cfg.adapt_rate = int(adapt_kind), int(n_adapt), float(adapt_target), float(adapt_rate)
    cfg.n_burnin, cfg.thin, cfg.stats_batch, cfg.trace_chains = int(n_burnin), int(thin), int(stats_batch), int(trace_chains)
    cfg.n_samples = int(n_samples) if n_samples is not None else (int(trace.shape[0]) if trace is not None else (
        int(trace_accept.shape[0]) if trace_accept is not None else 0))
    cfg.trace_centered = 1 if trace_centered else 0
    return cfg


class Engine(object):
    def __init__(self, spec, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("autoreparam_amd.Engine needs a GPU (gfx950); there is no CPU fallback")
        self.spec = spec
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self._L = _lib.lib()
        self._h = C.c_void_p(0)
        ds, keep = spec.dataset()
        with torch.cuda.device(self.device):
            _lib.check(self._L.arp_model_create(C.byref(ds), C.byref(self._h)))
        del keep
        for key, value in getattr(spec, "options", ()):
            self.set_option(key, value)
        self.D = self._L.arp_model_dim(self._h)
        assert self.D == spec.D, (self.D, spec.D)
        self._ab = [None, None]
        self._cache = {}

    def __del__(self):
        try:
            if self._h:
                self._L.arp_model_destroy(self._h)
                self._h = C.c_void_p(0)
        except Exception:
            pass

    # -- parameterisations ------------------------------------------------
    def set_param(self, which, reparam):
        """reparam: 'CP', 'NCP', a dict of ``<rv>_a``/``<rv>_b`` values, or an (a, b) pair of [D] arrays."""
        if isinstance(reparam, tuple):
            a, b = (np.ascontiguousarray(v, np.float32) for v in reparam)
        else:
            a, b = self.spec.ab_from_reparam(reparam)
        assert a.shape == (self.D,) and b.shape == (self.D,)
        with torch.cuda.device(self.device):
            _lib.check(self._L.arp_model_set_param(self._h, which, a.ctypes.data_as(_lib._f32p),
                                                   b.ctypes.data_as(_lib._f32p)))
        self._ab[which] = (a, b)

    def logp_const(self, which=0):
        return self._L.arp_model_logp_const(self._h, which)

    def _dev_cached(self, key, x):
        """Device copy of a small host array that is re-used while its contents do not change (the base step
        sizes of consecutive launches): no host-to-device copy, and no host synchronisation, per launch."""
        a = np.ascontiguousarray(x, np.float32)
        hit = self._cache.get(key)
        if hit is None or hit[0].shape != a.shape or not np.array_equal(hit[0], a):
            hit = (a.copy(), self._dev(a))
            self._cache[key] = hit
        return hit[1]

    # -- density / converters --------------------------------------------
    def _dev(self, x):
        t = torch.as_tensor(x, dtype=torch.float32)
        return t.to(self.device).contiguous()

    def logp_grad(self, x, which=0, lanes=0):
        x = self._dev(x)
        n = x.shape[0]
        logp = torch.empty(n, dtype=torch.float32, device=self.device)
        grad = torch.empty_like(x)
        _lib.call(self.device, self._L.arp_logp_grad, self._h, which, _lib.ptr(x), n, _lib.ptr(logp), _lib.ptr(grad), lanes)
        return logp, grad

    def transform(self, x, which=0, to_centered=True):
        x = self._dev(x)
        out = torch.empty_like(x)
        _lib.call(self.device, self._L.arp_transform, self._h, which, 0 if to_centered else 1, _lib.ptr(x), x.shape[0],
                  _lib.ptr(out))
        return out

    def energy_probe(self, x, eps0, n_leapfrog, which=0, kappa=None, seed=0, row_offset=0, lanes=0, want_p=False,
                     want_q=False):
        """One fresh-momentum trajectory from every row of `x` [N, D] (parameterisation `which`) with the steps
        eps0[d] * kappa[row] and `n_leapfrog` leapfrog steps (arp_energy_probe): returns out [N, 4] float32 =
        (logp, kinetic energy) at the start and at the end, then the drawn momenta (want_p) and the end states (want_q),
        [N, D] each.  Not a replay of a transition the sampler took; `x` is not changed.  The momenta depend on `lanes`."""
        x, eps, kap = self._probe_args(x, eps0, kappa)
        n = x.shape[0]
        out = torch.empty(n, 4, dtype=torch.float32, device=self.device)
        p = torch.empty_like(x) if want_p else None
        q = torch.empty_like(x) if want_q else None
        _lib.call(self.device, self._L.arp_energy_probe, self._h, int(which), _lib.ptr(x), n, int(n_leapfrog), _lib.ptr(eps),
                  _lib.ptr(kap), int(seed) & 0xFFFFFFFFFFFFFFFF, int(row_offset), _lib.ptr(out), _lib.ptr(p), _lib.ptr(q),
                  int(lanes))
        extra = tuple(t for t in (p, q) if t is not None)
        return (out,) + extra if extra else out

    def _probe_args(self, x, eps0, kappa):
        x = self._dev(x)
        eps = eps0.to(self.device, torch.float32).contiguous() if torch.is_tensor(eps0) else self._dev(np.asarray(eps0, np.float32))
        assert x.dim() == 2 and x.shape[1] == self.D and eps.shape == (self.D,)
        kap = None if kappa is None else self._dev(kappa)
        assert kap is None or kap.shape == (x.shape[0],)
        return x, eps, kap

    def trajectory_probe(self, x, eps0, n_leapfrog_max, which=0, kappa=None, seed=0, row_offset=0, lanes=0, want_path=True,
                         path_centred=False, want_p=False):
        """energy_probe's trajectory with every step recorded (arp_trajectory_probe): from every row of `x` [N, D]
        (parameterisation `which`) one fresh-momentum trajectory of `n_leapfrog_max` steps of eps0[d] * kappa[row].
        Returns energy [Lmax + 1, N, 2] float32 = (logp, kinetic energy) at l = 0 ... Lmax, then path [Lmax, N, D]
        (want_path: the state after step l, centred or in the sampler's coordinates) and the drawn momenta [N, D]
        (want_p: energy_probe's, bit for bit, for equal seed, offset and lanes).  Not a replay of a transition the sampler
        took; `x` is not changed."""
        x, eps, kap = self._probe_args(x, eps0, kappa)
        n, Lmax = x.shape[0], int(n_leapfrog_max)
        energy = torch.empty(max(Lmax, 0) + 1, n, 2, dtype=torch.float32, device=self.device)
        path = torch.empty(max(Lmax, 0), n, self.D, dtype=torch.float32, device=self.device) if want_path else None
        p = torch.empty_like(x) if want_p else None
        _lib.call(self.device, self._L.arp_trajectory_probe, self._h, int(which), _lib.ptr(x), n, Lmax, _lib.ptr(eps),
                  _lib.ptr(kap), int(seed) & 0xFFFFFFFFFFFFFFFF, int(row_offset), _lib.ptr(energy), _lib.ptr(path),
                  1 if path_centred else 0, _lib.ptr(p), int(lanes))
        extra = tuple(t for t in (path, p) if t is not None)
        return (energy,) + extra if extra else energy

    def trajectory_sums(self, x, eps0, n_leapfrog_max, which=0, kappa=None, seed=0, row_offset=0, lanes=0,
                        max_path_bytes=1 << 30):
        """The jump sums of a trajectory profile (arp_jump_sums over arp_trajectory_probe): returns (sums [Lmax, 5 + D]
        float64, energy [Lmax + 1, N, 2] float32) on the device.  sums[l - 1] = rows, divergent, nonfinite, sum of alpha,
        left_out, then per element the sum of alpha (x_l - x_0)^2 in centred coordinates, for a trajectory of l steps
        (diagnostics.profile_from_sums reads them).  The rows are cut into chunks whose path buffer fits `max_path_bytes`;
        a row's momentum stream is keyed by row_offset + its index, so the cut is invisible in every per-row output, and
        the chunks' sums are added in order.  (With lanes = 0 the library chooses the lanes per chain by the row count of
        a launch, and the momenta depend on them: name `lanes` where chunked and whole calls must agree bit for bit.)"""
        x, eps, kap = self._probe_args(x, eps0, kappa)
        n, Lmax, D = x.shape[0], int(n_leapfrog_max), self.D
        sums = torch.zeros(max(Lmax, 0), 5 + D, dtype=torch.float64, device=self.device)
        energy = torch.empty(max(Lmax, 0) + 1, n, 2, dtype=torch.float32, device=self.device)
        if n == 0:
            return sums, energy
        chunk = max(1, min(n, int(max_path_bytes) // max(1, 4 * D * max(Lmax, 1))))
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            xs = x[lo:hi]
            x0 = self.transform(xs, which=which, to_centered=True)
            e, path = self.trajectory_probe(xs, eps, Lmax, which=which, kappa=None if kap is None else kap[lo:hi], seed=seed,
                                            row_offset=int(row_offset) + lo, lanes=lanes, want_path=True, path_centred=True)
            energy[:, lo:hi] = e
            part = torch.empty_like(sums)
            _lib.call(self.device, self._L.arp_jump_sums, _lib.ptr(x0), _lib.ptr(path), _lib.ptr(e), hi - lo, D, Lmax,
                      _lib.ptr(part), workspace=self._L.arp_jump_workspace_bytes(hi - lo, D, Lmax))
            sums += part
            del path
        return sums, energy

    # -- HMC ----------------------------------------------------------------
    def hmc_run(self, state, eps0, n_leapfrog, n_steps, which=0, seed=0, chain_offset=0,
                adapt_kind=_lib.ADAPT_NONE, n_adapt=0, adapt_target=0.75, adapt_rate=0.05,
                n_burnin=0, thin=1, trace=None, trace_accept=None, trace_centered=True, lanes=0,
                stats=None, stats_batch=1, n_samples=None, trace_chains=0, rec_accept=None):
        """Advance `state` by n_steps transitions (one kernel launch).

        `stats` ([6, C, D] float32, zeroed before the first call) accumulates the streaming statistics of the
        recorded samples inside the kernel (`stats_summary`), `rec_accept` ([C] int32) the accepted recorded
        transitions; with them a run needs no trace, or only one of the first `trace_chains` chains
        (`trace` is then [S, trace_chains, D]).  `n_samples` = recorded samples of the whole run when no
        trace buffer gives it."""
        cfg = _hmc_config(state, n_leapfrog, n_steps, seed, chain_offset, adapt_kind, n_adapt, adapt_target, adapt_rate, n_burnin,
                          thin, trace, trace_accept, trace_centered, lanes, stats_batch, n_samples, trace_chains)
        io = _lib.HmcIO()
        io.q, io.grad, io.logp = _lib.ptr(state.q), _lib.ptr(state.grad), _lib.ptr(state.logp)
        io.adapt, io.rng, io.accept_count = _lib.ptr(state.adapt), _lib.ptr(state.rng), _lib.ptr(state.accept_count)
        self._eps0 = eps0 if torch.is_tensor(eps0) else self._dev_cached("eps0", eps0)
        io.eps0 = _lib.ptr(self._eps0)
        io.trace, io.trace_accept, io.stats = _lib.ptr(trace), _lib.ptr(trace_accept), _lib.ptr(stats)
        io.rec_accept_count = _lib.ptr(rec_accept)
        _lib.call(self.device, self._L.arp_hmc_run, self._h, which, C.byref(cfg), C.byref(io))
        state.step += int(n_steps)
        return state


    def interleaved_run(self, state, eps0_0, eps0_1, n_leapfrog_0, n_leapfrog_1, n_steps, seed=0,
                        chain_offset=0, adapt_kind=_lib.ADAPT_SIMPLE, n_adapt=0, adapt_target=0.75,
                        adapt_rate=0.05, n_burnin=0, thin=1, trace=None, trace_accept0=None,
                        trace_accept1=None, trace_centered=True, lanes=0, stats=None, stats_batch=1, n_samples=None,
                        trace_chains=0, rec_accept0=None, rec_accept1=None):
        """Advance `state` by n_steps interleaved steps (parameterisation 0 then 1 per step);
        stats / rec_accept* / trace_chains / n_samples as in hmc_run."""
        cfg = _hmc_config(state, n_leapfrog_0, n_steps, seed, chain_offset, adapt_kind, n_adapt, adapt_target, adapt_rate, n_burnin,
                          thin, trace, trace_accept0, trace_centered, lanes, stats_batch, n_samples, trace_chains)
        io = _lib.InterleavedIO()
        io.k0.q = _lib.ptr(state.q)
        io.k0.grad, io.k0.logp = _lib.ptr(state.grad), _lib.ptr(state.logp)   # carried gradient / log density
        io.k0.adapt, io.k0.rng, io.k0.accept_count = _lib.ptr(state.adapt), _lib.ptr(state.rng), _lib.ptr(state.accept_count)
        self._eps0 = eps0_0 if torch.is_tensor(eps0_0) else self._dev_cached("eps0", eps0_0)
        self._eps1 = eps0_1 if torch.is_tensor(eps0_1) else self._dev_cached("eps1", eps0_1)
        io.k0.eps0 = _lib.ptr(self._eps0)
        io.k0.trace, io.k0.trace_accept = _lib.ptr(trace), _lib.ptr(trace_accept0)
        io.k0.stats, io.k0.rec_accept_count, io.rec_accept_count1 = _lib.ptr(stats), _lib.ptr(rec_accept0), _lib.ptr(rec_accept1)
        io.adapt1, io.accept_count1 = _lib.ptr(state.adapt1), _lib.ptr(state.accept_count1)
        io.eps0_1 = _lib.ptr(self._eps1)
        io.trace_accept1 = _lib.ptr(trace_accept1)
        _lib.call(self.device, self._L.arp_interleaved_run, self._h, C.byref(cfg), int(n_leapfrog_1), C.byref(io))
        state.step += int(n_steps)
        return state


    # -- mean-field VI ----------------------------------------------------------
    def vi_run(self, lr, loc, rho, n_steps, n_mc, which=0, w=None, tied_b=False, wb=None, seed=0, a_prior=False,
               a_group=None, b_group=None, return_prior=False):
        """Run len(lr) independent Adam optimisations of the mean-field ELBO in one launch.

        loc, rho (and w, the unconstrained VIP parameter, when given) are [n_lr, D]
        device tensors updated in place; returns the ELBO timeline [n_lr, n_steps] (and, with return_prior,
        the per-step log prior of the learnable parameters).  a_group / b_group ([D] int leader indices) make
        untied parameterisation variables shared over a part (arp_vi_io.a_group)."""
        lr_t = self._dev(np.asarray(lr, np.float32))
        n_lr = lr_t.shape[0]
        assert loc.shape == (n_lr, self.D) and rho.shape == (n_lr, self.D)
        elbo = torch.empty(n_lr, int(n_steps), dtype=torch.float32, device=self.device)
        cfg = _lib.ViConfig()
        cfg.n_lr, cfg.n_steps, cfg.n_mc = n_lr, int(n_steps), int(n_mc)
        cfg.learn_a = 1 if w is not None else 0
        cfg.tied_b = 1 if tied_b else 0
        cfg.a_prior = 1 if a_prior else 0   # --discrete_prior on the learnable parameters
        cfg.seed = int(seed)
        io = _lib.ViIO()
        io.lr, io.loc, io.rho, io.w, io.elbo = _lib.ptr(lr_t), _lib.ptr(loc), _lib.ptr(rho), _lib.ptr(w), _lib.ptr(elbo)
        io.wb = _lib.ptr(wb)
        prior = torch.zeros(n_lr, int(n_steps), dtype=torch.float32, device=self.device) if return_prior else None
        io.prior = _lib.ptr(prior)
        ag = torch.as_tensor(np.asarray(a_group, np.int32), device=self.device) if a_group is not None else None
        bg = torch.as_tensor(np.asarray(b_group, np.int32), device=self.device) if b_group is not None else None
        io.a_group, io.b_group = _lib.ptr(ag), _lib.ptr(bg)
        _lib.call(self.device, self._L.arp_vi_run, self._h, which, C.byref(cfg), C.byref(io))
        return (elbo, prior) if return_prior else elbo


    def set_option(self, key, value):
        """Per-handle option (arp_model_set_option), e.g. ("german_math", "f32" | "bf16x3" | "auto")."""
        _lib.check(self._L.arp_model_set_option(self._h, key.encode(), value.encode()))

    def check(self):
        """Deferred status of this handle's asynchronous chain launches (arp_model_check): raises if a relay hand-over
        inside one of them timed out.  Call it after synchronising the stream the launches went to."""
        _lib.check(self._L.arp_model_check(self._h))

    def relay_geometry(self):
        """What this thread's last hmc_run / interleaved_run launch did (arp_relay_geometry): relay segments, chain blocks,
        workgroups of the kernel per CU."""
        out = (C.c_int32 * 3)()
        _lib.check(self._L.arp_relay_geometry(out))
        return dict(zip(("segments", "chain_blocks", "workgroups_per_cu"), [int(v) for v in out]))

    @staticmethod
    def relay_schedule(n_steps, segs, ratio_pct=0):
        """Segment lengths the library cuts a launch of n_steps into `segs` relay segments with (arp_relay_schedule):
        proportional to (ratio_pct / 100)^s; ratio_pct 0: the library's own ratio.  Needs no device."""
        out = (C.c_int32 * max(int(segs), 1))()
        if _lib.lib().arp_relay_schedule(int(n_steps), int(segs), int(ratio_pct), out, len(out)) != int(segs) or segs < 1:
            _lib.check(1)
        return [int(v) for v in out]

    def vi_attempts(self):
        """Launches this thread's last vi_run needed (arp_vi_attempts): 1 unless a hand-off ran into its bound and the fit was retaken."""
        out = (C.c_int32 * 1)()
        _lib.check(self._L.arp_vi_attempts(out))
        return int(out[0])

    def vi_geometry(self):
        """Shape of this thread's last vi_run launch (arp_vi_geometry): threads per workgroup, sample groups G and row
        parts R per learning rate, learning rates per launch, workgroups resident together, workgroups one CU holds."""
        out = (C.c_int32 * 6)()
        _lib.check(self._L.arp_vi_geometry(out))
        keys = ("threads_per_workgroup", "sample_groups", "row_parts", "learning_rates_per_launch", "workgroups_resident",
                "workgroups_per_cu")
        return dict(zip(keys, [int(v) for v in out]))

    def adapt_probe(self, log_accept, adapt, kind, n_adapt, step_base=0, target=0.75, rate=0.05):
        """Test hook (arp_adapt_probe): the kernels' step-size recurrence on scripted log acceptance ratios
        `log_accept` [n_steps, n]; `adapt` [n, 4] is updated in place; returns the multipliers [n_steps, n]."""
        la = self._dev(log_accept)
        n_steps, n = la.shape
        out = torch.empty(n_steps, n, dtype=torch.float32, device=self.device)
        cfg = _lib.HmcConfig()
        cfg.n_steps, cfg.step_base = int(n_steps), int(step_base)
        cfg.adapt_kind, cfg.n_adapt = int(kind), int(n_adapt)
        cfg.adapt_target, cfg.adapt_rate = float(target), float(rate)
        _lib.call(self.device, self._L.arp_adapt_probe, C.byref(cfg), _lib.ptr(la), n, _lib.ptr(adapt), _lib.ptr(out))
        return out


def clock_probe(device, ms=10.0):
    """GHz the chip holds under a vector-bound load (arp_clock_probe: packed FMAs on every SIMD for ~`ms` milliseconds, one
    wave reading s_memtime / s_memrealtime around its loop).  A measurement hook for bench.py: every roofline figure assumes
    a clock, and the boxes differ in the one they hold."""
    dev = torch.device(device)
    out = torch.zeros(3, dtype=torch.int64, device=dev)
    iters = max(1, int(ms * 1e-3 / (64 * 2 * 4.43 / 2.4e9)))       # 64 packed FMAs per iteration, two waves per SIMD
    _lib.call(dev, _lib.lib().arp_clock_probe, iters, _lib.ptr(out))
    torch.cuda.synchronize(dev)
    cyc, ticks = int(out[0].item()), int(out[1].item())
    return (cyc / ticks) * 0.1 if ticks > 0 else None


def stats_summary(stats, n, batch):
    """(mean, var, ess) [C, D] float64 tensors from an `arp_hmc_io.stats` buffer after `n` recorded samples:
    mean = ref + s1/n, var = (s2 - s1^2/n)/(n-1), ESS by batch means, n var / (batch var(batch means)), capped at n.
    Accuracy of the float32 planes against the float64 statistics of the same samples, measured at n = 16 384 with batch
    2 048 and 64 (tests/test_gpu_stats.py; DESIGN.md has the table): plane-per-sample route mean within 3.4e-7 (max|x| + 1),
    variance within 2.4e-7 (max|x| + 1)^2 (1.1e-5 relative), ESS within 1.5e-5, the same for first recorded samples < 1,
    1 - 3 and 3 - 10 sd from the mean (3 - 10 sd: mean 2.3e-6 sd, variance 1.1e-5, ESS 1.2e-5 relative); at 10 sd the float32
    restatement reads 3.7e-7 (max|x| + 1)^2 and ESS 9.2e-4.  LDS route: mean 4.8e-7, variance 7.7e-8, ESS 6.3e-4 at batch 2 048
    (2e-6 at batch 64)."""
    ref, s1, s2, _, sb1, sb2 = (stats[k].to(torch.float64) for k in range(6))
    mean = ref + s1 / n
    var = ((s2 - s1 * s1 / n) / max(n - 1, 1)).clamp_min(0)
    nb = n // batch
    if nb < 2:
        raise ValueError("batch-means ESS needs at least two complete batches")
    vb = ((sb2 - sb1 * sb1 / nb) / (nb - 1)).clamp_min(0)
    ess = torch.minimum(n * var / (batch * vb), torch.full_like(var, float(n)))
    return mean, var, ess


# ---------------------------------------------------------------------------
# State converters with the reference's calling convention (models.py:56-128):
# callables on lists of [C, *event] arrays, evaluated on the device.
# ---------------------------------------------------------------------------
_engines = {}


def engine_for(spec, device=None):
    """One cached Engine per (model spec, device); device defaults to FLAGS.device."""
    from .flags import FLAGS
    dev = torch.device(device if device is not None else FLAGS.device)
    key = (id(spec), str(dev))
    if key not in _engines:
        _engines[key] = Engine(spec, dev)
    return _engines[key]


def release(spec):
    """Forget the cached Engines of `spec` (every device): their model handles are destroyed once nothing else holds them.
    For a caller that makes many specs in one process (sbc.run_sbc: one per replicate); _engines is keyed by id(spec) and
    would otherwise keep every handle alive."""
    for key in [key for key in _engines if key[0] == id(spec)]:
        del _engines[key]


def _convert(spec, reparam, to_centered):
    def fn(state_parts):
        eng = engine_for(spec)
        eng.set_param(1, reparam)
        flat = spec.pack([np.asarray(p, np.float32).reshape(1, *np.shape(p)) if np.ndim(p) == len(s) else p
                          for p, s in zip(state_parts, spec.part_shapes)])
        single = all(np.ndim(p) == len(s) for p, s in zip(state_parts, spec.part_shapes))
        out = eng.transform(flat, which=1, to_centered=to_centered).cpu().numpy()
        parts = spec.unpack(out)
        return [p[0] for p in parts] if single else parts
    return fn


def build_make_to_centered(spec):
    def make_to_centered(**centering_kwargs):
        return _convert(spec, centering_kwargs, True)
    return make_to_centered


def build_make_to_partially_noncentered(spec):
    def make_to_partially_noncentered(**centering_kwargs):
        return _convert(spec, centering_kwargs, False)
    return make_to_partially_noncentered
