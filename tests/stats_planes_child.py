"""Child process of tests/test_gpu_stats.py (not collected as a test): repeats the packed kernels' statistics cases with
the library's statistics switch forced to the plane-per-sample route (ARP_DEBUG=1 ARP_STATS_LDS=0 in the environment; the
library reads the switch once per process, hence a process of its own).

    python stats_planes_child.py IN.npz OUT.npz

IN holds the step sizes of every case ("eps/<case>"), OUT receives "planes/<case>/<batch>", "q/..." and "rng/...".
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import stats_cases  # noqa: E402


def main(src, dst):
    if os.environ.get("ARP_DEBUG") != "1" or os.environ.get("ARP_STATS_LDS") != "0":
        sys.exit("stats_planes_child.py: needs ARP_DEBUG=1 ARP_STATS_LDS=0")
    gpu = torch.device("cuda:0")
    inp = np.load(src)
    out = {}
    for name in stats_cases.CHILD:
        c = stats_cases.CASES[name]
        for batch in c["batches"]:
            planes, q, rng = stats_cases.stats_run(c, inp["eps/" + name], batch, gpu)
            key = "%s/%d" % (name, batch)
            out["planes/" + key], out["q/" + key], out["rng/" + key] = planes, q, rng
    np.savez(dst, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
