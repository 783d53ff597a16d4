#!/usr/bin/env python3
"""German credit under its two scale priors in one process (arp_model_set_option "german_prior": lognormal for
german_credit_lognormalcentered, gamma for german_credit_gammascale): the fused HMC launch, NCP, 4 lanes per chain,
16 384 chains, L = 4, both matrix-core likelihoods; leapfrog-steps/s from HIP events (best of 5 launches), and the VI
fit (5 learning rates x 3 000 steps x 256 draws, the reference's defaults) per sweep.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/german_prior_bench.py` for the per-kernel times.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoreparam_amd import engine, models  # noqa: E402

dev = torch.device("cuda", 0)
C, L, n_steps = 16384, 4, int(os.environ.get("GPB_STEPS", "200"))
VI_LRS, VI_STEPS, VI_MC = [0.02, 0.05, 0.1, 0.2, 0.4], 3000, 256


def timed(fn, reps):
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best


sp = models._spec_german()
eng = engine.Engine(sp, dev)          # one handle, the prior switched per measurement
rs = np.random.RandomState(0)
q0 = torch.as_tensor((0.1 * rs.randn(C, sp.D)).astype(np.float32), device=dev)
eps0 = np.full(sp.D, 0.01, np.float32)
rates = {}
for math in ("bf16x3", "f32"):
    for prior in ("lognormal", "gamma"):
        eng.set_option("german_math", math)
        eng.set_option("german_prior", prior)
        eng.set_param(0, "NCP")
        st = engine.ChainState(q0)
        eng.hmc_run(st, eps0, L, 20, seed=1, lanes=4)   # warm-up
        ms = timed(lambda: eng.hmc_run(st, eps0, L, n_steps, seed=1, lanes=4), 5)
        rate = C * L * n_steps / (ms * 1e-3)
        rates[(math, prior)] = rate
        acc = st.accept_count.double().mean().item() / st.step
        print("hmc  %-7s %-9s NCP L=%d C=%d: %8.3f ms / %d transitions  %.4g leapfrog-steps/s  acceptance %.2f" % (
            math, prior, L, C, ms, n_steps, rate, acc), flush=True)
    print("hmc  %-7s gamma / lognormal rate: %.4f" % (math, rates[(math, "gamma")] / rates[(math, "lognormal")]), flush=True)
eng.set_option("german_math", "auto")
for prior in ("lognormal", "gamma"):
    eng.set_option("german_prior", prior)
    eng.set_param(0, (np.full(sp.D, 0.5, np.float32), np.ones(sp.D, np.float32)))

    def fit():
        r = np.random.RandomState(0)
        loc = torch.as_tensor((1e-2 * r.randn(len(VI_LRS), sp.D)).astype(np.float32), device=dev)
        rho = torch.full((len(VI_LRS), sp.D), -2.0, device=dev)
        w = torch.zeros(len(VI_LRS), sp.D, device=dev)
        fit.elbo = eng.vi_run(VI_LRS, loc, rho, VI_STEPS, VI_MC, w=w, seed=1)
    ms = timed(fit, 3)
    print("vi   %-9s cVIP %d lrs x %d steps x %d draws: %8.2f ms per sweep  finite=%s" % (
        prior, len(VI_LRS), VI_STEPS, VI_MC, ms, bool(torch.isfinite(fit.elbo).all())), flush=True)
