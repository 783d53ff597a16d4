#!/usr/bin/env python3
"""GPU box: arp_rank_normalize (fold = 0 and fold = 1) on the traces that matter -- the CLI's kept [1 000][1 024 x 71], the
headline sampler's [1 000][65 536 x 71] (18.6 GB) and config 3's kept [50 000][1 024 x 125] (25.6 GB) -- next to the same
result composed from torch.sort + torch.searchsorted on the device (one element at a time: the composition needs the
pool contiguous and three arrays of its size) and to arp_split_moments on the same trace.  Warm, medians over N launches
by stream events; the workspace is allocated once, outside the timed region.

    python tools/rank_bench.py [small|headline|config3] [launches]
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
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 5
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
prev = torch.randn(Cn, D, device=dev)
for t in range(S):
    prev = rho * prev + torch.sqrt(1 - rho * rho) * torch.randn(Cn, D, device=dev)
    x[t] = prev
x += torch.linspace(-50, 50, D, device=dev)
del prev
N = S * Cn
gb = x.numel() * 4 / 1e9
print("%s trace [%d][%d x %d]: %.2f GB, N = %d draws per element" % (which, S, Cn, D, gb, N), flush=True)

L = _lib.lib()
need = int(L.arp_rank_workspace_bytes(S, Cn, D, 1))
ws = torch.empty(need, dtype=torch.uint8, device=dev)
z = torch.empty_like(x)
med = torch.empty(D, dtype=torch.float32, device=dev)
print("workspace %.2f GB" % (need / 1e9), flush=True)


def native(fold):
    _lib.check(L.arp_rank_normalize(C.c_void_p(x.data_ptr()), S, Cn, D, Cn * D, fold, C.c_void_p(z.data_ptr()), None,
                                    C.c_void_p(med.data_ptr()), None, 0, None, C.c_void_p(ws.data_ptr()), need,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))


for fold in (0, 1):
    ms, lo = median_ms(lambda: native(fold), launches)
    print("arp_rank_normalize fold=%d : median %.2f ms (min %.2f)  %.2f G values/s" % (fold, ms, lo, x.numel() / ms / 1e6), flush=True)
z_native = z[:, :, 0].clone()
del ws


def composed(fold, out):
    """The same z from torch.sort + torch.searchsorted, element by element (float64 normal scores through erfinv)."""
    for d in range(D):
        col = x[:, :, d].reshape(-1)
        srt = torch.sort(col).values
        if fold:
            m = 0.5 * (srt[(N - 1) // 2] + srt[N // 2])
            col = (col - m).abs()
            srt = torch.sort(col).values
        r2 = torch.searchsorted(srt, col, right=False) + torch.searchsorted(srt, col, right=True)
        p = (4 * r2 + 1).to(torch.float64) / (8 * N + 2)
        out[:, :, d] = (2.0 ** 0.5 * torch.erfinv(2 * p - 1)).to(torch.float32).reshape(S, Cn)


for fold in (0, 1):
    ms, lo = median_ms(lambda: composed(fold, z), max(1, launches // 2))
    print("torch.sort + searchsorted fold=%d : median %.2f ms (min %.2f)" % (fold, ms, lo), flush=True)
composed(1, z)
print("max |z native - z composed| on element 0 (fold = 1): %.3g" % float((z[:, :, 0] - z_native).abs().max()), flush=True)
for split in (True,):
    ms, lo = median_ms(lambda: diagnostics.split_moments(x, split), launches)
    print("arp_split_moments split=%d : median %.3f ms (min %.3f)  %.2f TB/s" % (split, ms, lo, gb / ms), flush=True)
