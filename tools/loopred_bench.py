#!/usr/bin/env python3
"""GPU box: arp_loo_predictive next to arp_pointwise_loglik and arp_predictive_check on the same draws in the same
process, by the method of tools/ppc_bench.py, at the shapes DESIGN.md section 6 quotes for the predictive reports --
German credit (1 000 observations, T = 62, D = 125), election (11 566 observations, T = 3, D = 55) and radon MN (919
observations, Normal data) -- each with its real observation table at 65 536 draws, states N(0, 0.5).  Every entry point
walks the observations in the tiles the CLI uses for it (main.loo_tile_rows for the log-likelihood matrix,
main.ppc_tile_rows for the predictive check's workspace, main.loo_tile_rows at a third of the budget for the
leave-one-out report, whose float64 log weights sit next to the log-likelihoods); a figure is the time of ALL tiles of a
shape.  The log weights are synthetic, -|N(0, 3^2)| with a tenth of them -inf, in one buffer that every tile reads: the
kernel's time does not depend on where they came from, and the Pareto fits are not what is timed here.  Warm (three
passes first); a timed window is a batch of passes between two stream events, sized to about 0.2 s from the warm-up's own
time; the figure is the median over N windows of the time per pass.  Buffers and workspaces are allocated once, outside
the timed region.

    python tools/loopred_bench.py [windows, default 7] [draws, default 65536]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoreparam_amd import _lib, diagnostics, main, models  # noqa: E402

dev = torch.device("cuda:0")
windows = int(sys.argv[1]) if len(sys.argv) > 1 else 7
R = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
WINDOW_MS = 200.0


def median_ms(fn, n, warm=3):
    """(median, min, max) milliseconds per pass over n windows of `batch` back-to-back passes each."""
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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


L = _lib.lib()
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)

for name, spec in (("german_credit_lognormalcentered", models._spec_german()), ("election", models._spec_election()),
                   ("radon MN", models._spec_radon("MN"))):
    D = int(spec.D)
    t = diagnostics.upload_table(spec.observation_table(), D, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = (0.5 * torch.randn(1, R, D, device=dev, generator=gen)).contiguous()
    N = t.N
    rows_ll = main.loo_tile_rows(N, R)
    rows_pc = main.ppc_tile_rows(N, R, diagnostics.predictive_workspace_bytes)
    rows_lp = main.loo_tile_rows(N, R, main.LOO_CHUNK_BYTES // 3)
    ll = torch.empty(rows_ll, R, dtype=torch.float32, device=dev)
    lw = -(3.0 * torch.randn(rows_lp, R, dtype=torch.float64, device=dev, generator=gen)).abs()
    lw[torch.rand(rows_lp, R, device=dev, generator=gen) < 0.1] = float("-inf")
    mask = torch.empty(R, dtype=torch.uint8, device=dev)
    cnt = torch.zeros((), dtype=torch.int64, device=dev)
    need_pc = diagnostics.predictive_workspace_bytes(min(rows_pc, N), R)
    need_lp = diagnostics.loo_predictive_workspace_bytes(min(rows_lp, N), R)
    ws_pc = torch.empty(need_pc, dtype=torch.uint8, device=dev)
    ws_lp = torch.empty(need_lp, dtype=torch.uint8, device=dev)
    ds = torch.empty(R, 8, dtype=torch.float64, device=dev)
    obs = torch.empty(N, 4, dtype=torch.float64, device=dev)
    sums = torch.empty(N, 6, dtype=torch.float64, device=dev)
    table = (p(t.idx), p(t.w), t.T, p(t.y), p(t.scale_idx), p(t.log_scale))

    def loglik():
        for n0 in range(0, N, rows_ll):
            _lib.check(L.arp_pointwise_loglik(p(x), 1, R, D, R * D, t.kind, *table, n0, min(N, n0 + rows_ll), p(ll), R, p(mask),
                                              p(cnt), st()))

    def check():
        for n0 in range(0, N, rows_pc):
            n1 = min(N, n0 + rows_pc)
            _lib.check(L.arp_predictive_check(p(x), 1, R, D, R * D, t.kind, *table, n0, n1, 12345, 0, p(ds), p(obs[n0:n1]), None, 0,
                                              p(mask), p(cnt), p(ws_pc), need_pc, st()))

    def loopred():
        for n0 in range(0, N, rows_lp):
            n1 = min(N, n0 + rows_lp)
            _lib.check(L.arp_loo_predictive(p(x), 1, R, D, R * D, t.kind, *table, n0, n1, p(lw), R, p(sums[n0:n1]), p(ws_lp),
                                            need_lp, st()))

    print("%s: %d observations x %d draws, T = %d, D = %d, kind %d; tiles of %d (loglik), %d (check) and %d (loo predictive) "
          "observations; workspace %.1f MB (check), %.1f MB (loo predictive)" % (
              name, N, R, t.T, D, t.kind, rows_ll, rows_pc, rows_lp, need_pc / 1e6, need_lp / 1e6), flush=True)
    ms_l = median_ms(loglik, windows)
    print("  arp_pointwise_loglik: median %.3f ms (%.3f - %.3f)" % ms_l, flush=True)
    ms_c = median_ms(check, windows)
    print("  arp_predictive_check: median %.3f ms (%.3f - %.3f)  %.2f x loglik; %.1f G (n, r) / s" % (
        ms_c + (ms_c[0] / ms_l[0], N * R / 1e6 / ms_c[0])), flush=True)
    ms_p = median_ms(loopred, windows)
    print("  arp_loo_predictive:   median %.3f ms (%.3f - %.3f)  %.2f x loglik, %.2f x check; %.1f G (n, r) / s" % (
        ms_p + (ms_p[0] / ms_l[0], ms_p[0] / ms_c[0], N * R / 1e6 / ms_p[0])), flush=True)
    del x, ll, lw, ws_pc, ws_lp, ds, obs, sums
