#!/usr/bin/env python3
"""GPU box: arp_nested_step_sums next to arp_split_moments (split = 0) on the same trace in the same process -- both read
the trace once, so the existing kernel is the yardstick -- on the headline sampler's [1 000][65 536 x 71] (18.6 GB) or the
CLI's kept [1 000][1 024 x 71]; and arp_moments_fold_nested next to arp_moments_fold on the [C][71] per-chain moments.
Warm (three launches of every shape first); a timed window is a BATCH of launches between two stream events, sized to
about 0.2 s from the warm-up's own time, and the figure is the median over N windows of the time per launch; workspaces
are allocated once, outside the timed region.

    python tools/nested_rhat_bench.py [small|headline] [windows, default 7] [superchain sizes, default 64]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoreparam_amd import _lib, diagnostics  # noqa: E402

dev = torch.device("cuda:0")
which = sys.argv[1] if len(sys.argv) > 1 else "small"
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 7
WINDOW_MS = 200.0
sizes = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [64]
S, Cn, D = {"small": (1000, 1024, 71), "headline": (1000, 65536, 71)}[which]


def median_ms(fn, n, warm=3):
    """(median, min) milliseconds per launch over n windows of `batch` back-to-back launches each."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    batch = int(max(1, min(10000, WINDOW_MS / max(a.elapsed_time(b), 1e-3))))
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / batch)
    return float(np.median(ts)), float(np.min(ts))


x = torch.empty(S, Cn, D, dtype=torch.float32, device=dev)
for t in range(S):
    x[t].normal_()
x += torch.linspace(-50, 50, D, device=dev)
gb = x.numel() * 4 / 1e9
print("%s trace [%d][%d x %d]: %.2f GB" % (which, S, Cn, D, gb), flush=True)

L = _lib.lib()
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)

mean = torch.empty(1, Cn, D, dtype=torch.float32, device=dev)
var = torch.empty(1, Cn, D, dtype=torch.float32, device=dev)
need_m = int(L.arp_moments_workspace_bytes(S, Cn * D, 0))
ws_m = torch.empty(need_m, dtype=torch.uint8, device=dev) if need_m > 0 else None
ms_m, lo_m = median_ms(lambda: _lib.check(L.arp_split_moments(p(x), S, Cn * D, Cn * D, 0, p(mean), p(var), p(ws_m), need_m, st())),
                       launches)
print("arp_split_moments split=0   : median %.3f ms (min %.3f)  %.2f TB/s" % (ms_m, lo_m, gb / ms_m), flush=True)

for M in sizes:
    need = int(L.arp_nested_step_workspace_bytes(S, Cn, D, M))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need > 0 else None
    sums4 = torch.empty(4, S, D, dtype=torch.float64, device=dev)
    ms, lo = median_ms(lambda: _lib.check(L.arp_nested_step_sums(p(x), S, Cn, D, Cn * D, M, p(sums4), p(ws), need, st())), launches)
    r = diagnostics.nested_rhat_by_step(sums4)
    print("arp_nested_step_sums M=%-5d: median %.3f ms (min %.3f)  %.2f TB/s; workspace %.1f MB; %.2f x arp_split_moments; "
          "B / W x M: mean %.4f (1 when stationary)" % (M, ms, lo, gb / ms, need / 1e6, ms / ms_m,
                                                        float(np.nanmean(r ** 2 - 1.0)) * M), flush=True)
    del ws

sums5 = torch.empty(5, D, dtype=torch.float64, device=dev)
ms_f, lo_f = median_ms(lambda: _lib.check(L.arp_moments_fold(p(mean), p(var), Cn, D, p(sums5), st())), launches)
print("arp_moments_fold [%d][%d]        : median %.3f ms (min %.3f)" % (Cn, D, ms_f, lo_f), flush=True)
for M in sizes:
    sums6 = torch.empty(6, D, dtype=torch.float64, device=dev)
    ms, lo = median_ms(lambda: _lib.check(L.arp_moments_fold_nested(p(mean), p(var), Cn, D, M, p(sums6), st())), launches)
    print("arp_moments_fold_nested M=%-5d: median %.3f ms (min %.3f); %.2f x arp_moments_fold" % (M, ms, lo, ms / ms_f), flush=True)
