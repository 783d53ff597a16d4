#!/usr/bin/env python3
"""GPU box: the device pieces of the power-scaling sensitivity report at the shape the report takes them -- radon's real
observation table (PA by default) at 65 536 draws as 64 steps of 1 024 chains, states N(0, 0.5), synthetic smooth log
weights (five rows, as the report folds) -- next to arp_rank_normalize (fold = 0) on the same draws, the keys-only sort
arp_element_order's pair sort is measured against.  One process; device events around batches of about 0.2 s after three
warm passes, median of 7 windows with min - max.  --rank_lib PATH: a second library with arp_rank_normalize (another build
of csrc/rank.hip), timed in windows that alternate with this build's.

    python tools/psens_bench.py [windows] [draws] [dataset] [--rank_lib PATH]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoreparam_amd import _lib, diagnostics, main as cli, models  # noqa: E402

argv = list(sys.argv[1:])
rank_lib = None
if "--rank_lib" in argv:
    at = argv.index("--rank_lib")
    rank_lib = argv[at + 1]
    del argv[at:at + 2]
windows = int(argv[0]) if len(argv) > 0 else 7
draws = int(argv[1]) if len(argv) > 1 else 65536
dataset = argv[2] if len(argv) > 2 else "PA"
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


def report(name, fns):
    """Median, min and max ms per call over `windows` batches of every fn; the fns' windows alternate."""
    reps = [calibrate(fn) for fn in fns]
    ts = [[] for _ in fns]
    for _ in range(windows):
        for j, fn in enumerate(fns):
            ts[j].append(batch_ms(fn, reps[j]))
    for j, t in enumerate(ts):
        print("%-44s %9.3f ms (%.3f - %.3f)  [%d calls per window]" % (name[j], np.median(t), min(t), max(t), reps[j]), flush=True)
    return [float(np.median(t)) for t in ts]


spec = models.get_model_by_name("radon", dataset).model
D = spec.D
table = diagnostics.upload_table(spec.observation_table(), D, dev)
x = (0.5 * torch.randn(S, Cn, D, generator=torch.Generator(device=dev).manual_seed(1), device=dev)).contiguous()
print("radon %s: D = %d, %d observations, %d draws as [%d][%d x %d]" % (dataset, D, table.N, R, S, Cn, D), flush=True)

L = _lib.lib()
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

# arp_loglik_total on a tile of the report
rows = cli.loo_tile_rows(table.N, R)
tiles = -(-table.N // rows)
ll, _, _ = diagnostics.pointwise_loglik(x, table, 0, min(rows, table.N))
total = torch.zeros(R, dtype=torch.float64, device=dev)
t_total, = report(["arp_loglik_total, a tile of %d observations" % ll.shape[0]], [lambda: diagnostics.loglik_total(ll, total)])
print("    %d tile(s) of at most %d observations; %.2f GB of log-likelihoods per report, %.0f GB/s" % (
    tiles, rows, table.N * R * 4 / 1e9, ll.shape[0] * R * 4 / t_total / 1e6), flush=True)
del ll

# arp_element_order against the keys-only sort of arp_rank_normalize
need = int(L.arp_element_order_workspace_bytes(S, Cn, D))
ws = torch.empty(need, dtype=torch.uint8, device=dev)
order = torch.empty(D, R, dtype=torch.int32, device=dev)
values = torch.empty(D, R, dtype=torch.float32, device=dev)
need_r = int(L.arp_rank_workspace_bytes(S, Cn, D, 0))
ws_r = torch.empty(need_r, dtype=torch.uint8, device=dev)
z = torch.empty_like(x)


def element_order():
    _lib.check(L.arp_element_order(_lib.ptr(x), S, Cn, D, Cn * D, _lib.ptr(order), _lib.ptr(values), _lib.ptr(ws), need, st()))


def rank_normalize(lib):
    return lambda: _lib.check(lib.arp_rank_normalize(_lib.ptr(x), S, Cn, D, Cn * D, 0, _lib.ptr(z), None, None, None, 0, None,
                                                     _lib.ptr(ws_r), need_r, st()))


names, fns = ["arp_element_order (order and sorted)", "arp_rank_normalize fold=0 (this build)"], [element_order, rank_normalize(L)]
if rank_lib:
    other = C.CDLL(rank_lib)
    other.arp_rank_normalize.argtypes = L.arp_rank_normalize.argtypes
    other.arp_rank_normalize.restype = C.c_int
    z_here = z.clone()
    rank_normalize(L)()
    z_here.copy_(z)
    z.zero_()
    rank_normalize(other)()
    print("z of the two builds bitwise equal: %s" % bool(torch.equal(z.view(torch.int32), z_here.view(torch.int32))), flush=True)
    del z_here
    names.append("arp_rank_normalize fold=0 (%s)" % os.path.basename(rank_lib))
    fns.append(rank_normalize(other))
t = report(names, fns)
print("    element_order / rank_normalize: %.2f; workspace %.2f GB against %.2f GB; %.2f G values/s" % (
    t[0] / t[1], need / 1e9, need_r / 1e9, D * R / t[0] / 1e6), flush=True)
del ws_r, z

# arp_cjs_sums, the report's five rows
element_order()
lw = 0.01 * torch.randn(5, R, dtype=torch.float64, device=dev)
lw[4] = 0.0
shift = x.reshape(R, D).mean(dim=0).contiguous()
for K in (1, 5):
    t_cjs, = report(["arp_cjs_sums, K = %d rows" % K], [lambda: diagnostics.cjs_sums(values, order, lw[:K], shift)])
    print("    %.2f G (row, element, draw) / s" % (K * D * R / t_cjs / 1e6), flush=True)
