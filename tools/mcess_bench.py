#!/usr/bin/env python3
"""GPU box: arp_ess_multichain (split = 1) on the rank-normalised z trace of the traces that matter -- the CLI's kept
[1 000][1 024 x 71], the headline sampler's [1 000][65 536 x 71] (18.6 GB) and config 3's kept [50 000][1 024 x 125]
(25.6 GB), AR(1) with rho = 0.3 (three elements 0.75) -- next to arp_ess on the same trace, and the same again with one
slow element (rho = 0.99).  Warm, medians over N launches by stream events; the workspace is allocated once, outside the
timed region.  Trace passes are counted from where every element was cut: block 0 reads every row twice (the mean, then
lags 0 - 15), block b >= 1 reads the rows of the elements still open twice (leading and lagged stream) from draw 16 b on.

    python tools/mcess_bench.py [small|headline|config3] [launches] [slow]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoreparam_amd import _lib, diagnostics, util  # noqa: E402

dev = torch.device("cuda:0")
which = sys.argv[1] if len(sys.argv) > 1 else "small"
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 5
slow = len(sys.argv) > 3 and sys.argv[3] == "slow"
S, Cn, D = {"small": (1000, 1024, 71), "headline": (1000, 65536, 71), "config3": (50000, 1024, 125)}[which]


def median_ms(fn, n, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


x = torch.empty(S, Cn, D, dtype=torch.float32, device=dev)
rho = torch.full((D,), 0.3, device=dev); rho[:3] = 0.75
if slow:
    rho[D // 2] = 0.99
prev = torch.randn(Cn, D, device=dev)
for t in range(S):
    prev = rho * prev + torch.sqrt(1 - rho * rho) * torch.randn(Cn, D, device=dev)
    x[t] = prev
x += torch.linspace(-50, 50, D, device=dev)
del prev
z = diagnostics.rank_normalize(x, fold=False)[0]
del x
torch.cuda.empty_cache()
gb = z.numel() * 4 / 1e9
print("%s%s z trace [%d][%d x %d]: %.2f GB" % (which, " + one element at rho 0.99" if slow else "", S, Cn, D, gb), flush=True)

L = _lib.lib()
need = int(L.arp_ess_multichain_workspace_bytes(S, Cn, D, 1))
ws = torch.empty(need, dtype=torch.uint8, device=dev)
ess = torch.empty(D, dtype=torch.float32, device=dev)
max_t = torch.empty(D, dtype=torch.int32, device=dev)
print("workspace %.3f GB (%.1f %% of the trace)" % (need / 1e9, 100.0 * need / (gb * 1e9)), flush=True)


def native():
    _lib.check(L.arp_ess_multichain(C.c_void_p(z.data_ptr()), S, Cn, D, Cn * D, 1, None, C.c_void_p(ess.data_ptr()),
                                    C.c_void_p(max_t.data_ptr()), None, 0, C.c_void_p(ws.data_ptr()), need,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))


ms, lo = median_ms(native, launches)
cut = max_t.cpu().numpy().astype(np.int64)
n = S // 2
blocks = (2 * ((n - 6) // 2) + 2) // 16 + 1
passes = 2.0
for b in range(1, int(cut.max()) // 16 + 1):
    passes += 2.0 * float((cut >= 16 * b).mean()) * (1.0 - 16.0 * b / n)
print("arp_ess_multichain split=1 : median %.3f ms (min %.3f); cut lags min %d, median %d, max %d; %d blocks enqueued, "
      "%d with work; %.2f trace passes, %.2f TB/s" % (ms, lo, cut.min(), int(np.median(cut)), cut.max(), blocks,
                                                      int(cut.max()) // 16 + 1, passes, passes * gb / ms), flush=True)
e = ess.cpu().numpy()
print("    bulk-ESS / N: min %.4f, median %.4f" % (e.min() / (S * Cn), float(np.median(e)) / (S * Cn)), flush=True)
del ws
ms2, lo2 = median_ms(lambda: util.effective_sample_size(z), launches)
print("arp_ess (per chain) : median %.3f ms (min %.3f)  %.2f TB/s for one pass; multi-chain / per-chain = %.2f" % (
    ms2, lo2, gb / ms2, ms / ms2), flush=True)
