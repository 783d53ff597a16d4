#!/usr/bin/env python3
"""GPU box: arp_site_prior_draws at the shape the prior predictive report takes it -- 65 536 ancestral draws from the real
site tables of German credit with Gamma scales (the log-Gamma form, its rejection loop) and of election (the widest of
the Normal tables), with and without undrawn -- next to arp_site_logprior over the draws just made (groups = parts), the
kernel that reads what this one writes.  prior_bench.py's method: one process, device events around batches of about
0.2 s after three warm passes, median of 7 windows with min - max; the entry points' windows alternate.

    python tools/prior_draw_bench.py [windows] [draws]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoreparam_amd import _lib, diagnostics, models  # noqa: E402

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 7
R = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
dev = torch.device("cuda:0")
SEED = 0x5052494F


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
        print("%-52s %9.3f ms (%.3f - %.3f)  [%d calls per window]" % (names[j], np.median(t), min(t), max(t), reps[j]), flush=True)
    return [float(np.median(t)) for t in ts]


L = _lib.lib()
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = _lib.ptr
for spec in (models._spec_german_gammascale(), models._spec_election()):
    D = spec.D
    sites = diagnostics.upload_site_table(spec.site_table(), D, dev)
    G = sites.P
    x = torch.empty(R, D, dtype=torch.float32, device=dev)
    undrawn = torch.empty(R, dtype=torch.uint8, device=dev)
    group_lp = torch.empty(R, G, dtype=torch.float64, device=dev)
    mask = torch.empty(R, dtype=torch.uint8, device=dev)
    count = torch.zeros((), dtype=torch.int64, device=dev)
    forms = np.bincount(np.asarray(sites.host.form), minlength=3)
    print("%s: D = %d (%d Normal, %d softplus, %d log-Gamma elements), %d draws" % (spec.name, D, forms[0], forms[1], forms[2], R),
          flush=True)

    def draw(flags):
        return lambda: _lib.check(L.arp_site_prior_draws(
            D, p(sites.form), p(sites.loc_idx), p(sites.loc_w), p(sites.loc0), p(sites.scale_idx), p(sites.scale_w),
            p(sites.log_scale0), R, SEED, 0, p(x), D, p(flags), st()))

    def logprior():
        _lib.check(L.arp_site_logprior(
            p(x), 1, R, D, R * D, p(sites.form), p(sites.loc_idx), p(sites.loc_w), p(sites.loc0), p(sites.scale_idx),
            p(sites.scale_w), p(sites.log_scale0), p(sites.norm), p(sites.part), G, p(group_lp), p(None), p(mask), p(count), st()))

    t = report(["arp_site_prior_draws", "arp_site_prior_draws, undrawn = NULL", "arp_site_logprior of those draws, groups = parts"],
               [draw(undrawn), draw(None), logprior])
    torch.cuda.synchronize()
    print("    %.4f ns per element drawn; %.0f MB written per call -> %.0f GB/s; %d draws undrawn, %d masked by the twin" % (
        t[0] * 1e6 / (R * D), R * D * 4 / 1e6, R * D * 4 / t[0] / 1e6, int(undrawn.sum().item()), int(count.item())), flush=True)
    del x, group_lp
