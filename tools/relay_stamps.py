#!/usr/bin/env python3
"""Where a relay launch's wave slots stand empty: reads the stamps a library built with -DARP_EXP_RELAY_STAMPS wrote for its
last relay launch (ARP_DEBUG=1 ARP_RELAY_STAMPS_OUT=file; kernels.h: relay_stamp) and prints one table.

    tools/build_variants.sh stamps=-DARP_EXP_RELAY_STAMPS
    ARP_DEBUG=1 ARP_LIB_PATH=$PWD/autoreparam_amd/libautoreparam_hip_stamps.so ARP_RELAY_STAMPS_OUT=/tmp/stamps.bin \\
        python bench.py --steps 20 --warmup 5
    tools/relay_stamps.py /tmp/stamps.bin [label]

Per workgroup (ticket) the file holds the 100 MHz clock at kernel entry, after the ticket wait, at the first step, after the
last step and before exit, and the hardware id (HW_ID, XCC_ID) of the wave that wrote them.  Workgroups are grouped by CU
and dealt to the CU's slots in order of entry (a workgroup takes the slot that was given up last before it entered).

(a) tail: per slot, from its last exit to the launch's last exit
(b) hand-over: entry -> first step (without the wait), last step -> exit, exit -> next entry of the slot
(c) wait: entry -> after the ticket wait, segments behind the first (the ticket draw and a barrier are in it)"""
import sys

import numpy as np

TICK_US = 0.01


def load(path):
    w = np.fromfile(path, dtype=np.uint64)
    segs, blocks, k = int(w[0]), int(w[1]), int(w[2])
    return segs, blocks, w[3:3 + segs * blocks * k].reshape(segs * blocks, k)


def slots_of(st):
    """[(cu key, [workgroup indices in order])] -- one entry per slot"""
    hw = st[:, 5]
    cu = ((hw >> np.uint64(32)) & np.uint64(0xF)) << np.uint64(8) | ((hw >> np.uint64(8)) & np.uint64(0xFF))   # XCC, SE, SH, CU
    out = []
    for key in np.unique(cu):
        idx = np.nonzero(cu == key)[0]
        idx = idx[np.argsort(st[idx, 0], kind="stable")]
        slots = []
        for i in idx:
            free = [s for s in slots if st[s[-1], 4] <= st[i, 0]]
            if free:
                max(free, key=lambda s: st[s[-1], 4]).append(i)
            else:
                slots.append([i])
        out += [(int(key), s) for s in slots]
    return out


def summary(path, label=""):
    segs, blocks, st = load(path)
    st = st.astype(np.int64)
    t_first, t_last = st[:, 0].min(), st[:, 4].max()
    span = (t_last - t_first) * TICK_US
    slots = slots_of(st.astype(np.uint64))
    tails = np.array([(t_last - st[s[-1], 4]) * TICK_US for _, s in slots])
    heads = np.array([(st[s[0], 0] - t_first) * TICK_US for _, s in slots])
    gaps = np.array([(st[b, 0] - st[a, 4]) * TICK_US for _, s in slots for a, b in zip(s, s[1:])])
    seg = np.arange(len(st)) // blocks
    wait = (st[:, 1] - st[:, 0]) * TICK_US
    prologue = (st[:, 2] - st[:, 1]) * TICK_US
    epilogue = (st[:, 4] - st[:, 3]) * TICK_US
    steps = (st[:, 3] - st[:, 2]) * TICK_US
    busy = ((st[:, 4] - st[:, 0]) * TICK_US).sum()
    w = wait[seg > 0]
    lines = [
        "%s: %d segments x %d chain blocks, %d CUs, %d slots" % (label or path, segs, blocks, len({k for k, _ in slots}), len(slots)),
        "  launch, first entry -> last exit                 %9.1f us" % span,
        "  slots occupied (entry -> exit), share of launch  %9.4f" % (busy / (len(slots) * span)),
        "  (a) tail per slot        mean %8.1f us (%.2f %% of the launch)  median %8.1f  max %8.1f" %
        (tails.mean(), 100 * tails.mean() / span, np.median(tails), tails.max()),
        "      first entry per slot mean %8.1f us" % heads.mean(),
        "  (b) hand-over            entry->first step %6.1f us + last step->exit %6.1f us + exit->next entry %6.1f us = %6.1f us" %
        (prologue.mean(), epilogue.mean(), gaps.mean() if len(gaps) else 0.0,
         prologue.mean() + epilogue.mean() + (gaps.mean() if len(gaps) else 0.0)),
        "      step loop per segment (us): " + " ".join("%.0f" % steps[seg == s].mean() for s in range(segs)),
        "  (c) wait for the flag    mean %8.1f us  median %8.1f  p99 %8.1f  max %8.1f   sum per slot %8.1f us (%.2f %% of the launch)" %
        (w.mean(), np.median(w), np.percentile(w, 99), w.max(), w.sum() / len(slots), 100 * w.sum() / len(slots) / span),
        "      per segment (us): " + " ".join("%.1f" % wait[seg == s].mean() for s in range(1, segs)),
    ]
    return "\n".join(lines)


if __name__ == "__main__":
    print(summary(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""))
