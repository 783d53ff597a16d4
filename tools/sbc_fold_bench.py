#!/usr/bin/env python3
"""GPU box: arp_sbc_fold at N = 1 024 replicates of L = 1 024 draws and Q = 89 quantities -- 373 MB read once, 1.5 MB
written -- next to a torch.clone of the same buffer in the same process: a plain read-and-write of the same bytes.  The
fold reads the bytes once and writes almost nothing, so it should not take longer than the copy.  prior_bench.py's
method: one process, device events around batches of about 0.2 s after three warm passes, median of 7 windows with
min - max; the two windows alternate.  The buffer is larger than the 256 MiB Infinity Cache.

    python tools/sbc_fold_bench.py [windows] [N] [L] [Q]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoreparam_amd import _lib  # noqa: E402

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 7
N, L, Q = (int(sys.argv[k]) if len(sys.argv) > k else v for k, v in ((2, 1024), (3, 1024), (4, 89)))
dev = torch.device("cuda:0")


def batch_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def calibrate(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return max(1, int(200.0 / max(batch_ms(fn, 3), 1e-3)))


lib = _lib.lib()
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = _lib.ptr
gen = torch.Generator(device=dev).manual_seed(1)
draws = torch.randn(N, L, Q, dtype=torch.float32, device=dev, generator=gen)
truth = torch.randn(N, Q, dtype=torch.float32, device=dev, generator=gen)
counts = torch.empty(N, Q, 2, dtype=torch.int32, device=dev)
sums = torch.empty(N, Q, 2, dtype=torch.float64, device=dev)
left_out = torch.empty(N, dtype=torch.uint8, device=dev)
n_left_out = torch.zeros((), dtype=torch.int64, device=dev)


def fold():
    _lib.check(lib.arp_sbc_fold(p(draws), N, L, Q, L * Q, Q, p(truth), Q, p(counts), p(sums), p(left_out), p(n_left_out), st()))


def clone():
    torch.clone(draws)       # (the caching allocator hands the same block back after the first call)


names, fns = ["arp_sbc_fold", "torch.clone of the same buffer"], [fold, clone]
reps = [calibrate(fn) for fn in fns]
ts = [[] for _ in fns]
for _ in range(windows):
    for j, fn in enumerate(fns):
        ts[j].append(batch_ms(fn, reps[j]))
nbytes = 4.0 * N * L * Q
print("N = %d replicates, L = %d draws, Q = %d quantities: %.0f MB" % (N, L, Q, nbytes / 1e6), flush=True)
for j, t in enumerate(ts):
    moved = nbytes * (1 if j == 0 else 2)
    print("%-36s %9.4f ms (%.4f - %.4f)  %.0f GB/s moved  [%d calls per window]" % (
        names[j], np.median(t), min(t), max(t), moved / np.median(t) / 1e6, reps[j]), flush=True)
print("fold / copy = %.2f; %d replicates left out; a uniform rank's mean %.4f (1/2)" % (
    float(np.median(ts[0]) / np.median(ts[1])), int(n_left_out.item()),
    float(((counts[:, :, 0].double() + 0.5) / (L + 1)).mean().item())), flush=True)
