#!/usr/bin/env python3
"""GPU box: arp_gram_sums next to arp_split_moments (split = 0) on the same trace in the same process -- both read the
same bytes once, so the existing kernel is the yardstick -- on the headline sampler's [1 000][65 536 x 71] (18.6 GB) or
the CLI's kept [1 000][1 024 x 71]; on a D = 125 trace; and on that trace's 250-column [u, v] companion (what
diagnostics.scale_coupling hands the kernel).  Warm (three launches of every shape first); a timed window is a BATCH of
launches between two stream events, sized to about 0.2 s from the warm-up's own time, and the figure is the median over N
windows of the time per launch; workspaces are allocated once, outside the timed region.  TFLOP/s: `useful` counts the
D (D + 1) / 2 entries of the upper triangle at 2 flops a row, `issued` the 32 x 32 blocks the matrix cores compute.

    python tools/geometry_bench.py [small|headline] [windows, default 7]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoreparam_amd import _lib  # noqa: E402

dev = torch.device("cuda:0")
which = sys.argv[1] if len(sys.argv) > 1 else "small"
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 7
WINDOW_MS = 200.0
SHAPES = {"small": [(1000, 1024, 71), (1000, 512, 125), (1000, 512, 250)],
          "headline": [(1000, 65536, 71), (1000, 8192, 125), (1000, 8192, 250)]}[which]


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


L = _lib.lib()
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)

for S, Cn, D in SHAPES:
    x = torch.empty(S, Cn, D, dtype=torch.float32, device=dev)
    for t in range(S):
        x[t].normal_()
    centre = torch.linspace(-50, 50, D, device=dev)
    x += centre
    gb = x.numel() * 4 / 1e9
    rows = S * Cn
    print("trace [%d][%d x %d]: %.2f GB" % (S, Cn, D, gb), flush=True)

    mean = torch.empty(1, Cn, D, dtype=torch.float32, device=dev)
    var = torch.empty(1, Cn, D, dtype=torch.float32, device=dev)
    need_m = int(L.arp_moments_workspace_bytes(S, Cn * D, 0))
    ws_m = torch.empty(need_m, dtype=torch.uint8, device=dev) if need_m > 0 else None
    ms_m, lo_m = median_ms(lambda: _lib.check(L.arp_split_moments(p(x), S, Cn * D, Cn * D, 0, p(mean), p(var), p(ws_m), need_m,
                                                                  st())), launches)
    print("  arp_split_moments split=0: median %.3f ms (min %.3f)  %.2f TB/s" % (ms_m, lo_m, gb / ms_m), flush=True)

    need = int(L.arp_gram_workspace_bytes(S, Cn, D))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    sums = torch.empty(D + 2, D, dtype=torch.float64, device=dev)
    shift = centre.contiguous()
    ms, lo = median_ms(lambda: _lib.check(L.arp_gram_sums(p(x), S, Cn, D, Cn * D, p(shift), p(sums), p(ws), need, st())), launches)
    nb = (D + 31) // 32
    useful = rows * D * (D + 1) / 1e9 / ms
    issued = rows * nb * (nb + 1) * 1024.0 / 1e9 / ms
    n = float(sums[D + 1, 0])
    var_max = float(((sums[:D].diagonal() - sums[D] ** 2 / n) / (n - 1)).max())
    print("  arp_gram_sums            : median %.3f ms (min %.3f)  %.2f TB/s  %.1f TFLOP/s useful, %.1f issued; workspace "
          "%.1f MB; %.2f x arp_split_moments; rows %d, largest variance %.4f (1 expected)" % (
              ms, lo, gb / ms, useful, issued, need / 1e6, ms / ms_m, int(n), var_max), flush=True)
    del x, ws, ws_m, mean, var
