#!/usr/bin/env python3
"""GPU box: arp_weighted_moments and arp_affine_rows at the shape moment matching takes them -- 65 536 draws of D = 10, 88
and 255 synthetic N(0, 1) elements, 1 and 8 targets -- next to arp_site_logprior (a synthetic table of independent Normal
sites, one group) and arp_gram_sums over the same matrix in the same process.  prior_bench.py's method: device events
around batches of about 0.2 s after three warm passes, median of 7 windows with min - max; the entry points' windows
alternate.  The wrappers are timed as the report calls them (their output and workspace allocations included).

    python tools/mmatch_bench.py [windows] [draws]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoreparam_amd import diagnostics, models  # noqa: E402

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 7
R = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
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


def report(names, fns):
    reps = [calibrate(fn) for fn in fns]
    ts = [[] for _ in fns]
    for _ in range(windows):
        for j, fn in enumerate(fns):
            ts[j].append(batch_ms(fn, reps[j]))
    for j, t in enumerate(ts):
        print("%-44s %9.3f ms (%.3f - %.3f)  [%d calls per window]" % (names[j], np.median(t), min(t), max(t), reps[j]), flush=True)
    return [float(np.median(t)) for t in ts]


for D in (10, 88, 255):
    gen = torch.Generator(device=dev).manual_seed(D)
    x = torch.randn(R, D, generator=gen, device=dev).contiguous()
    zi, zf = np.zeros((D, models.SITE_TERMS), np.int32), np.zeros((D, models.SITE_TERMS), np.float32)
    sites = diagnostics.upload_site_table(models.SiteTable(np.zeros(D, np.int32), zi, zf, np.zeros(D, np.float32), zi, zf,
                                                           np.zeros(D, np.float32), np.zeros(D, np.float32), np.zeros(D, np.int32)),
                                          D, dev)
    centre = torch.zeros(D, dtype=torch.float32, device=dev)
    print("D = %d, %d draws" % (D, R), flush=True)
    names, fns = [], []
    for B in (1, 8):
        lw = (2.0 * torch.randn(B, R, generator=gen, device=dev)).to(torch.float64).contiguous()
        m, s, u = (torch.randn(B, D, generator=gen, device=dev).contiguous() for _ in range(3))
        out = torch.empty(B, R, D, dtype=torch.float32, device=dev)
        names += ["arp_weighted_moments, %d target(s)" % B, "arp_affine_rows, %d target(s)" % B]
        fns += [lambda lw=lw: diagnostics.weighted_moments(x, lw, centre),
                lambda m=m, s=s, u=u, out=out: diagnostics.affine_rows(x, m, s, u, -1, out=out)]
    names += ["arp_site_logprior, one group", "arp_gram_sums"]
    fns += [lambda: diagnostics.site_logprior(x[None], sites), lambda: diagnostics.gram_sums(x, centre)]
    t = report(names, fns)
    moved = [R * D * 4 + R * 8, R * D * 8, R * D * 4 + 8 * R * 8, R * D * 4 * 9]
    print("    bytes read and written per call: %s" % ", ".join("%.0f MB -> %.0f GB/s" % (b / 1e6, b / s / 1e6)
                                                               for b, s in zip(moved, t[:4])), flush=True)
