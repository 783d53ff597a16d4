"""The shapes and the closed-form case the moment-matching tests share (tests/test_mmatch_host.py, test_gpu_mmatch.py)."""
import math

import numpy as np

# the walks of csrc/mmatch.hip: chunks of 256 rows (arp_weighted_moments), tiles of 64 rows (arp_affine_rows), 256 / D row
# lanes per column, groups of 8 targets
ROWS = (1, 2, 63, 64, 65, 257, 4099)
COLUMNS = (1, 2, 63, 64, 65, 255)
TARGETS = (1, 3, 17)
AFFINE_TARGETS = (1, 5)

# ---- the closed-form case: posterior N(0, I_4), left-out term Normal(y | theta_0, variance) ----
DRAWS, DIM = 4096, 4
SEEDS = (0, 1, 2, 3)
HIGH = (2.0, 1.3)                   # (y, variance): the plain k-hat is above the threshold
LOW = (1.0, 2.0)                    # ... and below it


def draws(seed):
    return np.random.default_rng(seed).standard_normal((DRAWS, DIM)).astype(np.float32)


def logp(rows):
    rows = np.asarray(rows, np.float64)
    return -0.5 * (rows * rows).sum(axis=1)


def loglik(case, rows):
    y, var = case
    rows = np.asarray(rows, np.float64)
    return -0.5 * (y - rows[:, 0]) ** 2 / var - 0.5 * math.log(2.0 * math.pi * var)


def exact_elpd(case):
    """log Normal(y | m, v + variance) with the leave-out posterior of theta_0 Normal(m, v): v = 1 / (1 - 1 / variance),
    m = -v y / variance."""
    y, var = case
    v = 1.0 / (1.0 - 1.0 / var)
    m = -v * y / var
    return -0.5 * (y - m) ** 2 / (v + var) - 0.5 * math.log(2.0 * math.pi * (v + var))


def moments_case(R, D, B, seed, spread=1.0e4, far=0.0):
    """(x [R, D] float32, lw [B, R] float64, centre [D] float32) for arp_weighted_moments: log weights spread over
    +-`spread` in the first target and over a few units in the others (so that many draws carry weight), a centre `far`
    away from the data."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((R, D)) * 3.0 + rng.standard_normal(D)[None]).astype(np.float32)
    lw = rng.standard_normal((B, R)) * 2.0
    lw[0] = rng.uniform(-spread, spread, R)
    if B > 2:
        lw[2] += 5.0e3                                   # a large common offset cancels
    centre = (x.astype(np.float64).mean(axis=0) + far).astype(np.float32)
    return x, lw, centre
