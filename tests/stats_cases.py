"""The runs behind tests/test_gpu_stats.py, shared by the test module and by the child process that repeats the packed
kernels' cases on the plane-per-sample route (tests/stats_planes_child.py).  Not collected as a test.

A case is one sampler run described by a dict; `trace_run` records its whole [S, C, D] trace, `stats_run` repeats it from
the same seeds with the in-kernel statistics instead, cut into the case's launches."""
import numpy as np
import torch

import helpers

L_HMC = 3


def case(mname, lanes, C, S, batches, kind="NCP", burn=5, thin=3, centered=True, interleaved=False, cuts=None, frac=0.05):
    return dict(mname=mname, lanes=lanes, C=C, S=S, batches=tuple(batches), kind=kind, burn=burn, thin=thin, centered=centered,
                interleaved=interleaved, cuts=cuts, frac=frac)


def total_steps(c):
    return 1 + c["burn"] + c["thin"] * (c["S"] - 1)


def launches(c, batch):
    """The launch lengths of a statistics run.  Without `cuts`, the schedule edges in one run (burn-in 5, every third
    transition): a first launch that ends inside burn-in, one that ends on the step that completes the first batch, one of
    two steps that records nothing, and the rest."""
    total = total_steps(c)
    if c["cuts"] is not None:
        cuts = list(c["cuts"])
    else:
        assert c["burn"] >= 4 and c["thin"] == 3
        end = 1 + c["burn"] + (batch - 1) * c["thin"]       # transitions up to the sample that completes the first batch
        cuts = [3, end, end + 2]
    out, done = [], 0
    for t in cuts + [total]:
        assert done < t <= total
        out.append(t - done); done = t
    return out


def recorded_per_launch(c, batch):
    """how many samples each launch of `launches` records"""
    out, done = [], 0
    for n in launches(c, batch):
        steps = np.arange(done, done + n)                   # 0-based transition indices of this launch
        r = steps - c["burn"]
        out.append(int(((r >= 0) & (r % c["thin"] == 0) & (r // c["thin"] < c["S"])).sum()))
        done += n
    return out


# B1: production batch lengths.  64 chains make C * D a multiple of 4 for every model: the 16-byte paths of the plane walks.
S1 = 16384
B1 = {
    "b1-8schools": case("8schools", 2, 64, S1, (S1 // 8, 64), burn=300, thin=1, cuts=(4099, 11000), frac=0.1),
    "b1-german": case("german", 4, 64, S1, (S1 // 8, 64), burn=300, thin=1, cuts=(4099, 11000), frac=0.1),
    "b1-radon_PA": case("radon_PA", 4, 64, S1, (S1 // 8, 64), burn=300, thin=1, cuts=(4099, 11000), frac=0.1),
}

# B2: shapes and schedule edges (every case runs the edge schedule of `launches`), S <= 40
B2 = {}
for _m, _l in (("8schools", 2), ("radon_PA", 4), ("election", 4)):
    B2["b2-%s-c64-ragged" % _m] = case(_m, _l, 64, 38, (4,))                      # whole waves, aligned; S % batch = 2
    B2["b2-%s-c68-batch1" % _m] = case(_m, _l, 68, 40, (1,), centered=False)      # aligned, ragged last wave
    B2["b2-%s-c75-half" % _m] = case(_m, _l, 75, 40, (20,))                       # unaligned; batch = S // 2
    B2["b2-%s-c68-ragged-raw" % _m] = case(_m, _l, 68, 37, (5,), centered=False)
    # launches that end after the first sample and in the middle of the first batch: the LDS route's first fold is one sample
    B2["b2-%s-c68-first-batch-cut" % _m] = case(_m, _l, 68, 26, (8,), cuts=(6, 15, 40))
for _m, _l, _k in (("electric", 16, "NCP"), ("time_series", 4, "NCP"), ("radon_sd_MN", 8, "NCP"), ("funnel", 1, "NCP"),
                   ("german", 8, "NCP"), ("german", 16, "NCP"), ("german_gammascale", 4, "NCP"), ("election", 4, "VIP"),
                   ("radon_PA", 4, "VIP")):
    B2["b2-%s-%d-%s" % (_m, _l, _k)] = case(_m, _l, 68, 26, (4,), kind=_k)
for _m, _l in (("radon_PA", 4), ("election", 8), ("8schools", 2)):
    B2["b2-interleaved-%s" % _m] = case(_m, _l, 68, 26, (4,), centered=False, interleaved=True)

CASES = dict(B1); CASES.update(B2)

# B3: what the child process repeats with the packed kernels' statistics forced down the plane-per-sample route
CHILD = ["b1-radon_PA"] + [k for k in B2 if k.startswith("b2-radon_PA-c") or k.startswith("b2-election-c")] + \
        ["b2-interleaved-radon_PA", "b2-interleaved-election"]


def spec(mname):
    if mname == "german_gammascale":
        from autoreparam_amd import models
        if mname not in helpers._cache:
            helpers._cache[mname] = models._spec_german_gammascale()
        return helpers._cache[mname]
    return helpers.spec(mname)


def params(c):
    return helpers.params(spec(c["mname"]), c["kind"], seed=3)


def start(c):
    return helpers.states(spec(c["mname"]), c["C"], seed=4, scale=0.1)


def eps_from_oracle(oracle_lib, c):
    """a stable per-element step: frac / sqrt(|diag Hessian| + 1) from finite differences of the oracle's gradient (the
    interleaved cases take a flat 1e-3 for both parameterisations, as tests/test_gpu_hmc.py does)"""
    sp = spec(c["mname"])
    if c["interleaved"]:
        return np.full(sp.D, 1e-3, np.float32)
    if c["mname"] == "german_gammascale":          # the C oracle has no Gamma-prior form: its float64 restatement
        import gammascale_ref
        orc = gammascale_ref.GermanRef(sp.raw["X"], sp.raw["y"])
    else:
        orc = oracle_lib.OracleModel(sp)
    a, b = params(c)
    x0 = start(c)[:1].astype(np.float64)
    _, g0 = orc.logp_grad(x0, a, b)
    h = 1e-4
    diag = np.zeros(sp.D)
    for d in range(sp.D):
        xp = x0.copy(); xp[0, d] += h
        diag[d] = -(orc.logp_grad(xp, a, b)[1][0, d] - g0[0, d]) / h
    return (c["frac"] / np.sqrt(np.abs(diag) + 1.0)).astype(np.float32)


_engines = {}


def engine_for(c, gpu):
    from autoreparam_amd import engine
    key = (c["mname"], c["kind"], c["interleaved"])
    if key not in _engines:
        eng = engine.Engine(spec(c["mname"]), gpu)
        if c["interleaved"]:
            eng.set_param(0, "CP"); eng.set_param(1, "NCP")
        else:
            eng.set_param(0, params(c))
        _engines[key] = eng
    return _engines[key]


def _run(eng, c, st, eps, n, **extra):
    kw = dict(seed=8, n_burnin=c["burn"], thin=c["thin"], trace_centered=c["centered"], lanes=c["lanes"])
    kw.update(extra)
    if c["interleaved"]:
        eng.interleaved_run(st, eps, eps, 2, 2, n, **kw)
    else:
        eng.hmc_run(st, eps, L_HMC, n, **kw)


def trace_run(c, eps, gpu):
    """(trace [S, C, D] on the device, final q, final rng): one launch, the whole trace"""
    from autoreparam_amd import engine
    eng = engine_for(c, gpu)
    st = engine.ChainState(torch.as_tensor(start(c), device=gpu))
    tr = torch.zeros(c["S"], c["C"], spec(c["mname"]).D, device=gpu)
    _run(eng, c, st, eps, total_steps(c), trace=tr)
    torch.cuda.synchronize()
    return tr, st.q.cpu().numpy(), st.rng.cpu().numpy()


def stats_run(c, eps, batch, gpu):
    """(planes [6, C, D] float32, final q, final rng): the same run with the in-kernel statistics, cut into launches"""
    from autoreparam_amd import engine
    eng = engine_for(c, gpu)
    st = engine.ChainState(torch.as_tensor(start(c), device=gpu))
    planes = torch.zeros(6, c["C"], spec(c["mname"]).D, device=gpu)
    for n in launches(c, batch):
        _run(eng, c, st, eps, n, stats=planes, stats_batch=batch, n_samples=c["S"])
    torch.cuda.synchronize()
    return planes.cpu().numpy(), st.q.cpu().numpy(), st.rng.cpu().numpy()
