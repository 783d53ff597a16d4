#!/usr/bin/env python3
"""GPU box: arp_split_moments (+ arp_moments_fold) next to arp_ess on the two traces that matter -- the headline
sampler's [1 000][65 536 x 85] (18.6 GB when D = 71 .. 22.3 GB at D = 85; the wide route) and config 3's kept
[50 000][1 024 x 125] (25.6 GB; the long route) -- filled with AR(1) series (rho 0.75 on three elements, 0.3 elsewhere:
arp_ess's time depends on the mixing, arp_split_moments' does not).  Warm, medians over N launches by stream events;
run it under `rocprofv3 --kernel-trace --stats` for the per-kernel figures.

    python tools/moments_bench.py [headline|config3] [launches]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoreparam_amd import diagnostics, util  # noqa: E402

dev = torch.device("cuda:0")
which = sys.argv[1] if len(sys.argv) > 1 else "headline"
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 20
S, C, D = (1000, 65536, int(os.environ.get("BENCH_D", "85"))) if which == "headline" else (50000, 1024, 125)


def median_ms(fn, n):
    fn(); fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


x = torch.empty(S, C, D, dtype=torch.float32, device=dev)
rho = torch.full((D,), 0.3, device=dev); rho[:3] = 0.75
prev = torch.randn(C, D, device=dev)
for t in range(S):
    prev = rho * prev + torch.sqrt(1 - rho * rho) * torch.randn(C, D, device=dev)
    x[t] = prev
x += torch.linspace(-50, 50, D, device=dev)
gb = x.numel() * 4 / 1e9
print("%s trace [%d][%d x %d]: %.1f GB" % (which, S, C, D, gb), flush=True)
for split in (True, False):
    ms, lo = median_ms(lambda: diagnostics.split_moments(x, split), launches)
    print("arp_split_moments split=%d : median %.3f ms (min %.3f)  %.2f TB/s" % (split, ms, lo, gb / ms), flush=True)
mean, var = diagnostics.split_moments(x, True)
ms, lo = median_ms(lambda: diagnostics.fold(mean, var), launches)
print("arp_moments_fold [%d][%d]  : median %.3f ms (min %.3f)" % (2 * C, D, ms, lo), flush=True)
ms, lo = median_ms(lambda: util.effective_sample_size(x), launches if which == "headline" else 3)
print("arp_ess                    : median %.3f ms (min %.3f)  %.2f TB/s (one pass)" % (ms, lo, gb / ms), flush=True)
r = diagnostics.rhat_from_sums(diagnostics.fold(mean, var), S // 2)
print("split rhat max %.5f over %d rows" % (np.nanmax(r.rhat), int(r.rows[0])))
