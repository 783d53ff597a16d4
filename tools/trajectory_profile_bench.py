#!/usr/bin/env python3
"""GPU box: what a trajectory profile costs.  arp_trajectory_probe (with the centred path) and arp_jump_sums next to
arp_energy_probe at n_leapfrog = Lmax on the same rows in the same process, at the headline shape (radon PA, 65 536 rows,
Lmax = 8 and 32) and German credit (16 384 rows); and the fold's achieved bytes/s (path + start states + energies, read
once) next to arp_split_moments reading the same number of bytes.  Warm (three launches of every shape first); a timed
window is a BATCH of launches between two stream events, sized to about 0.2 s from the warm-up's own time, and the figure
is the median over N windows of the time per launch; buffers and workspaces are allocated once, outside the timed region.

    python tools/trajectory_profile_bench.py [windows, default 7] [shapes, default radon_PA:65536:8,radon_PA:65536:32,german:16384:8,german:16384:32]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoreparam_amd import _lib, engine, models  # noqa: E402

dev = torch.device("cuda:0")
windows = int(sys.argv[1]) if len(sys.argv) > 1 else 7
shapes = (sys.argv[2] if len(sys.argv) > 2 else "radon_PA:65536:8,radon_PA:65536:32,german:16384:8,german:16384:32").split(",")
WINDOW_MS = 200.0
SPECS = {"radon_PA": lambda: models._spec_radon("PA"), "german": lambda: models._spec_german()}


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
engines = {}
for shape in shapes:
    name, n, Lmax = shape.split(":")
    n, Lmax = int(n), int(Lmax)
    if name not in engines:
        engines[name] = engine.Engine(SPECS[name](), dev)
        engines[name].set_param(0, "NCP")
    eng = engines[name]
    D = eng.D
    x = 0.1 * torch.randn(n, D, device=dev)
    eps = torch.full((D,), 0.01, device=dev)
    kappa = 0.5 + torch.rand(n, device=dev)
    out4 = torch.empty(n, 4, device=dev)
    energy = torch.empty(Lmax + 1, n, 2, device=dev)
    path = torch.empty(Lmax, n, D, device=dev)
    sums = torch.empty(Lmax, 5 + D, dtype=torch.float64, device=dev)
    need = int(L.arp_jump_workspace_bytes(n, D, Lmax))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need > 0 else None
    x0 = eng.transform(x, which=0, to_centered=True)
    ms_e, lo_e = median_ms(lambda: _lib.check(L.arp_energy_probe(eng._h, 0, p(x), n, Lmax, p(eps), p(kappa), 1, 0, p(out4), None,
                                                                 None, 0, st())), windows)
    ms_n, lo_n = median_ms(lambda: _lib.check(L.arp_trajectory_probe(eng._h, 0, p(x), n, Lmax, p(eps), p(kappa), 1, 0, p(energy),
                                                                     None, 0, None, 0, st())), windows)
    ms_p, lo_p = median_ms(lambda: _lib.check(L.arp_trajectory_probe(eng._h, 0, p(x), n, Lmax, p(eps), p(kappa), 1, 0, p(energy),
                                                                     p(path), 1, None, 0, st())), windows)
    ms_f, lo_f = median_ms(lambda: _lib.check(L.arp_jump_sums(p(x0), p(path), p(energy), n, D, Lmax, p(sums), p(ws), need, st())),
                           windows)
    gb = (path.numel() + Lmax * x0.numel() + Lmax * 4 * n) * 4 / 1e9     # what the fold's workgroups ask for (x0 once per step)
    # arp_split_moments over a trace of the same number of bytes: S = Lmax + 1 rows of n * D floats
    trace = torch.randn(Lmax + 1, n * D, device=dev)
    mean = torch.empty(1, n * D, device=dev)
    var = torch.empty(1, n * D, device=dev)
    need_m = int(L.arp_moments_workspace_bytes(Lmax + 1, n * D, 0))
    ws_m = torch.empty(need_m, dtype=torch.uint8, device=dev) if need_m > 0 else None
    ms_m, lo_m = median_ms(lambda: _lib.check(L.arp_split_moments(p(trace), Lmax + 1, n * D, n * D, 0, p(mean), p(var), p(ws_m), need_m,
                                                                  st())), windows)
    gb_m = trace.numel() * 4 / 1e9
    print("%s rows=%d D=%d Lmax=%d" % (name, n, D, Lmax), flush=True)
    print("  arp_energy_probe n_leapfrog=%d        : median %.4f ms (min %.4f)" % (Lmax, ms_e, lo_e), flush=True)
    print("  arp_trajectory_probe, energies only    : median %.4f ms (min %.4f)  %.2f x the energy probe" % (ms_n, lo_n, ms_n / ms_e), flush=True)
    print("  arp_trajectory_probe, centred path     : median %.4f ms (min %.4f)  %.2f x the energy probe; writes %.3f GB, %.2f TB/s" % (
        ms_p, lo_p, ms_p / ms_e, path.numel() * 4 / 1e9, path.numel() * 4 / 1e9 / ms_p), flush=True)
    print("  arp_jump_sums                          : median %.4f ms (min %.4f)  %.3f GB read, %.2f TB/s; workspace %.2f MB" % (
        ms_f, lo_f, gb, gb / ms_f, need / 1e6), flush=True)
    print("  arp_split_moments on %.3f GB          : median %.4f ms (min %.4f)  %.2f TB/s" % (gb_m, ms_m, lo_m, gb_m / ms_m), flush=True)
    print("  probe + fold                           : %.4f ms = %.2f x the energy probe" % (ms_p + ms_f, (ms_p + ms_f) / ms_e), flush=True)
    del x, path, energy, trace, ws, ws_m
