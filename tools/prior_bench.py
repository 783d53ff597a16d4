#!/usr/bin/env python3
"""GPU box: arp_site_logprior at the shape the sensitivity report takes it -- the real site tables of German credit
(D = 125, the 3 parts as groups) and time_series (D = 123, 123 parts) at 65 536 draws as 64 steps of 1 024 chains, states
N(0, 0.5), without and with elem_lp -- next to arp_pointwise_loglik over the model's whole observation table on the same
draws.  psens_bench.py's method: one process, device events around batches of about 0.2 s after three warm passes,
median of 7 windows with min - max; the two entry points' windows alternate.

    python tools/prior_bench.py [windows] [draws]
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
draws = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
dev = torch.device("cuda:0")
Cn = min(1024, draws)
S = draws // Cn
R = S * Cn


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
for spec in (models._spec_german(), models._spec_time_series()):
    D = spec.D
    sites = diagnostics.upload_site_table(spec.site_table(), D, dev)
    table = diagnostics.upload_table(spec.observation_table(), D, dev)
    G = sites.P
    x = (0.5 * torch.randn(S, Cn, D, generator=torch.Generator(device=dev).manual_seed(1), device=dev)).contiguous()
    group_lp = torch.empty(R, G, dtype=torch.float64, device=dev)
    elem_lp = torch.empty(R, D, dtype=torch.float32, device=dev)
    ll = torch.empty(table.N, R, dtype=torch.float32, device=dev)
    mask = torch.empty(R, dtype=torch.uint8, device=dev)
    count = torch.zeros((), dtype=torch.int64, device=dev)
    print("%s: D = %d, G = %d parts, %d observations (T = %d), %d draws as [%d][%d x %d]" % (
        spec.name, D, G, table.N, table.T, R, S, Cn, D), flush=True)

    def site(elements):
        return lambda: _lib.check(L.arp_site_logprior(
            p(x), S, Cn, D, Cn * D, p(sites.form), p(sites.loc_idx), p(sites.loc_w), p(sites.loc0), p(sites.scale_idx),
            p(sites.scale_w), p(sites.log_scale0), p(sites.norm), p(sites.part), G, p(group_lp), p(elements), p(mask), p(count),
            st()))

    def loglik():
        _lib.check(L.arp_pointwise_loglik(p(x), S, Cn, D, Cn * D, table.kind, p(table.idx), p(table.w), table.T, p(table.y),
                                          p(table.scale_idx), p(table.log_scale), 0, table.N, p(ll), R, p(mask), p(count), st()))

    t = report(["arp_site_logprior, groups = parts", "arp_site_logprior, with elem_lp", "arp_pointwise_loglik, all observations"],
               [site(None), site(elem_lp), loglik])
    moved = (R * D * 4 + R * G * 8, R * D * 4 + R * G * 8 + R * D * 4, R * D * 4 + table.N * R * 4)
    print("    bytes read and written per call: %s GB/s" % ", ".join("%.0f MB -> %.0f" % (b / 1e6, b / s / 1e6) for b, s in zip(moved, t)),
          flush=True)
    del x, group_lp, elem_lp, ll
