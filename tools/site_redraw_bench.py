#!/usr/bin/env python3
"""GPU box: arp_site_redraw at the shape the mixed predictive check takes it -- 65 536 recorded draws as a [256, 256, D]
block of a centred trace -- next to arp_site_prior_draws at the same R and D in the same process (the kernel it shares its
drawing code with; the redraw differs by one read of the unflagged part of the block) and next to arp_split_moments over
the same block (one streaming read of it: what that read should cost on this box).  8 schools with theta redrawn
(D = 10), radon MN with m redrawn (D = 88) and the synthetic chain of the tests with its tail redrawn (D = 255, every
form, the rejection loop).  prior_draw_bench.py's method: device events around batches of about 0.2 s after three warm
passes, median of 7 windows with min - max; the entry points' windows alternate.

    python tools/site_redraw_bench.py [windows] [draws]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from autoreparam_amd import _lib, diagnostics, models  # noqa: E402

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 7
R = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
dev = torch.device("cuda:0")
SEED = 0x50504D58


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
    """Median, min and max ms per call over `windows` batches of every fn; the fns' windows alternate."""
    reps = [calibrate(fn) for fn in fns]
    ts = [[] for _ in fns]
    for _ in range(windows):
        for j, fn in enumerate(fns):
            ts[j].append(batch_ms(fn, reps[j]))
    for j, t in enumerate(ts):
        print("%-52s %9.4f ms (%.4f - %.4f)  [%d calls per window]" % (names[j], np.median(t), min(t), max(t), reps[j]), flush=True)
    return [float(np.median(t)) for t in ts]


def synthetic():
    from test_prior_draw_host import synthetic_chain
    return "synthetic chain", synthetic_chain(255), 255, (np.arange(255) >= 100).astype(np.uint8)


def model(spec, parts):
    return spec.name, spec.site_table(), spec.D, diagnostics.redraw_selection(spec.site_table(), spec.part_names, parts)


L = _lib.lib()
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = _lib.ptr
S = 256 if R % 256 == 0 else 1
Cn = R // S
for name, table, D, flags in (model(models._spec_eight_schools(), ["theta"]), model(models._spec_radon("MN"), ["m"]), synthetic()):
    sites = diagnostics.upload_site_table(table, D, dev)
    cols = [p(getattr(sites, c)) for c in ("form", "loc_idx", "loc_w", "loc0", "scale_idx", "scale_w", "log_scale0")]
    x = torch.empty(R, D, dtype=torch.float32, device=dev)
    out = torch.empty(R, D, dtype=torch.float32, device=dev)
    undrawn = torch.empty(R, dtype=torch.uint8, device=dev)
    dflags = torch.as_tensor(flags, device=dev)
    every = torch.ones(D, dtype=torch.uint8, device=dev)
    print("%s: D = %d, %d elements redrawn, %d draws as [%d, %d, D]" % (name, D, int(flags.sum()), R, S, Cn), flush=True)

    def prior():
        _lib.check(L.arp_site_prior_draws(D, *cols, R, SEED, 0, p(x), D, p(undrawn), st()))

    def redraw(which):
        return lambda: _lib.check(L.arp_site_redraw(p(x), S, Cn, D, Cn * D, *cols, p(which), SEED, 0, p(out), D, p(undrawn), st()))

    trace = x.view(S, Cn, D)

    def moments():
        diagnostics.split_moments(trace, split=False)

    prior()
    torch.cuda.synchronize()
    fns = [prior, redraw(dflags), redraw(every)] + ([moments] if S > 1 else [])
    names = ["arp_site_prior_draws", "arp_site_redraw, the selection", "arp_site_redraw, every element flagged"]
    t = report(names + (["arp_split_moments over the block (wrapper)"] if S > 1 else []), fns)
    torch.cuda.synchronize()
    block = R * D * 4
    read = int((flags == 0).sum()) * R * 4
    print("    redraw of the selection: %.0f MB read + %.0f MB written -> %.0f GB/s; prior draws: %.0f MB written -> %.0f GB/s%s" % (
        read / 1e6, block / 1e6, (read + block) / t[1] / 1e6, block / 1e6, block / t[0] / 1e6,
        "; the block streamed once by arp_split_moments: %.0f GB/s" % (block / t[3] / 1e6) if S > 1 else ""), flush=True)
    del x, out
