"""CPU: german_credit_gammascale on the host side -- the float64 restatement (tests/gammascale_ref.py) against torch
autograd of the log joint written with torch.distributions, its HMC and random-stream layout against the oracle (with
the log-normal prior switched in, the model the oracle covers), and the model spec: parts, option, the parameterisation
dicts of its fixed part and the learned_reparam keys."""
import collections

import numpy as np
import pytest
import torch

import gammascale_ref
import helpers
from autoreparam_amd import models


@pytest.fixture(scope="module")
def spec():
    return models._spec_german_gammascale()


def _log_joint_torch(X, y, a, b, q):
    """log p of the model under (a, b) in sampler coordinates q, float64, with torch.distributions; the Jacobian of
    the VIP maps is included as the reference's interceptor writes them (the latent is drawn in its own coordinates)"""
    D = torch.distributions
    F = X.shape[1]
    a = torch.as_tensor(np.float32(a), dtype=torch.float64); b = torch.as_tensor(np.float32(b), dtype=torch.float64)
    ot, bls, bt = q[0], q[1:1 + F], q[1 + F:]
    # ols ~ N(0, 10): ot ~ N(a * 0, 10^b), ols = 0 + 10^(1-b) (ot - 0)
    lp = D.Normal(0.0, 10.0 ** b[0]).log_prob(ot)
    ols = 10.0 ** (1.0 - b[0]) * ot
    # bls = log g, g ~ Gamma(0.5, 0.5): density of the log, Jacobian exp(bls)
    lp = lp + (D.Gamma(torch.tensor(0.5, dtype=torch.float64), torch.tensor(0.5, dtype=torch.float64)).log_prob(torch.exp(bls)) + bls).sum()
    s = ols + bls
    bb = b[1 + F:]
    lp = lp + D.Normal(0.0, torch.exp(bb * s)).log_prob(bt).sum()
    beta = torch.exp((1.0 - bb) * s) * bt
    lp = lp + D.Bernoulli(logits=torch.as_tensor(X) @ beta).log_prob(torch.as_tensor(y)).sum()
    return lp


@pytest.mark.parametrize("kind", ["CP", "NCP", "VIP"])
def test_restated_gradient_matches_autograd(spec, kind):
    X = spec.raw["X"].astype(np.float64); y = spec.raw["y"].astype(np.float64)
    ref = gammascale_ref.GermanRef(spec.raw["X"], spec.raw["y"])
    a, b = helpers.params(spec, kind)
    q = helpers.states(spec, 5, seed=3, scale=0.3).astype(np.float64)
    lp, g = ref.logp_grad(q, a, b)
    for c in range(q.shape[0]):
        qt = torch.tensor(q[c], dtype=torch.float64, requires_grad=True)
        lt = _log_joint_torch(X, y, a, b, qt)
        lt.backward()
        assert abs(lp[c] + ref.logp_const(b) - lt.item()) < 1e-9 * max(1.0, abs(lt.item())), (kind, c)
        np.testing.assert_allclose(g[c], qt.grad.numpy(), rtol=1e-9, atol=1e-9)


def test_logp_const_is_the_lognormal_models(spec, oracle_lib):
    """0.5 log 0.5 - lgamma(0.5) = -0.5 log(2 pi): the constant the engine drops for the Gamma prior of a log scale is the
    one N(ols, 1) drops, and arp_model_logp_const is the same for both priors"""
    from math import lgamma, log, pi
    assert abs((0.5 * log(0.5) - lgamma(0.5)) - (-0.5 * log(2 * pi))) < 1e-15
    ref = gammascale_ref.GermanRef(spec.raw["X"], spec.raw["y"])
    for kind in ("CP", "NCP", "VIP"):
        a, b = helpers.params(spec, kind)
        orc = oracle_lib.OracleModel(helpers.spec("german"))
        assert abs(ref.logp_const(b) - orc.logp_const(b)) < 1e-9


def test_restated_converters_and_dparam(spec):
    ref = gammascale_ref.GermanRef(spec.raw["X"], spec.raw["y"])
    a, b = helpers.params(spec, "VIP", seed=4)
    q = helpers.states(spec, 4, seed=5).astype(np.float64)
    x = ref.to_centered(q, a, b)
    np.testing.assert_allclose(ref.from_centered(x, a, b), q, rtol=1e-12, atol=1e-12)
    F = spec.raw["X"].shape[1]
    np.testing.assert_array_equal(x[:, 1:1 + F], q[:, 1:1 + F])                      # bls maps to itself
    # dparam is d logp / d(a, b) at fixed sampler coordinates: central differences of logp in b (a is inert)
    _, g = ref.logp_grad(q, a, b)
    da, db = ref.dparam(q, g, a, b)
    assert not da.any()
    for d in (0, 3, 1 + F + 7, 1 + F + F - 1):   # ols, a bls (inert), two betas
        bp, bm = b.copy(), b.copy()              # (a, b) are float32: the step taken is what float32 holds
        bp[d] += np.float32(1e-4); bm[d] -= np.float32(1e-4)
        num = (ref.logp_grad(q, a, bp)[0] - ref.logp_grad(q, a, bm)[0]) / (float(bp[d]) - float(bm[d]))
        if d == 0:   # the top-level scale's -b log 10 lives in the dropped constant
            num = num - np.log(10.0)
        np.testing.assert_allclose(db[:, d], num, rtol=1e-5, atol=1e-5)
    assert not db[:, 1:1 + F].any()


def test_restated_hmc_reproduces_the_oracle_with_the_lognormal_prior(oracle_lib):
    """the momenta / uniforms this module draws from the oracle's exported streams are the ones the oracle's own HMC
    (and the kernels) use: same chain step by step on german_credit_lognormalcentered"""
    sp = helpers.spec("german")
    ref = gammascale_ref.GermanRef(sp.raw["X"], sp.raw["y"], prior="lognormal")
    orc = oracle_lib.OracleModel(sp)
    decisions = []
    for kind, lanes, step in (("NCP", 4, 0.01), ("CP", 8, 0.05)):
        a, b = helpers.params(sp, kind)
        q0 = helpers.states(sp, 6, seed=2, scale=0.1)
        lp_o, g_o = orc.logp_grad(q0, a, b)
        lp_r, g_r = ref.logp_grad(q0, a, b)
        np.testing.assert_allclose(lp_r, lp_o, rtol=1e-12, atol=1e-9)
        np.testing.assert_allclose(g_r, g_o, rtol=1e-12, atol=1e-9)
        eps = np.full(sp.D, step, np.float32)
        n, L = 6, 3
        r = ref.hmc(oracle_lib, q0, a, b, eps, L, n, seed=9, chain_offset=1000, lanes=lanes)
        so = oracle_lib.new_state(q0, np.float64)
        xo = np.zeros((n, 6, sp.D)); ao = np.zeros((n, 6), np.uint8)
        orc.hmc_run(so, a, b, eps, L, n, seed=9, chain_offset=1000, lanes=lanes, trace=xo, trace_accept=ao,
                    trace_centered=False)
        np.testing.assert_array_equal(r["acc"], ao)
        np.testing.assert_allclose(r["x"], xo, rtol=1e-5, atol=1e-6)
        decisions.append(ao.ravel())
    decisions = np.concatenate(decisions)
    assert 0 < decisions.sum() < decisions.size     # both branches of the Metropolis test were taken


def test_model_spec(spec):
    cfg = models.get_model_by_name("german_credit_gammascale")
    sp = cfg.model
    assert sp.name == "german_credit_gammascale" and sp.D == 125
    assert sp.part_names == ["overall_log_scale", "beta_log_scales", "beta"]
    assert sp.part_shapes == [(), (62,), (62,)]
    assert sp.options == (("german_prior", "gamma"),) and sp.fixed_parts == {"beta_log_scales"}
    assert sp.scalar_loc == set()
    ln = models.get_model_by_name  # the log-normal spec is unchanged
    assert models._spec_german().options == () and models._spec_german().fixed_parts == set()
    np.testing.assert_array_equal(sp.raw["X"], models._spec_german().raw["X"])
    with pytest.raises(Exception, match="german_credit_gammascale"):
        ln("no_such_model")


def test_ab_from_reparam_without_the_fixed_part(spec):
    F = 62
    rp = {"overall_log_scale_a": 0.3, "overall_log_scale_b": 0.6, "beta_a": np.full(F, 0.2), "beta_b": np.linspace(0, 1, F)}
    a, b = spec.ab_from_reparam(rp)
    assert a[0] == np.float32(0.3) and b[0] == np.float32(0.6)
    np.testing.assert_array_equal(a[1 + F:], np.float32(0.2)); np.testing.assert_array_equal(b[1 + F:], np.float32(np.linspace(0, 1, F)))
    np.testing.assert_array_equal(a[1:1 + F], 1.0); np.testing.assert_array_equal(b[1:1 + F], 1.0)
    # CP / NCP vectors stay whole (the engine classifies them as CP / NCP)
    for kind, v in (("CP", 1.0), ("NCP", 0.0)):
        a, b = spec.ab_from_reparam(kind)
        assert (a == v).all() and (b == v).all()
    ones = {"overall_log_scale_a": 1.0, "beta_a": np.ones(F)}
    a, b = spec.ab_from_reparam(ones)
    assert (a == 1).all() and (b == 1).all()
    with pytest.raises(KeyError):
        spec.ab_from_reparam({"beta_a": np.ones(F)})


@pytest.mark.parametrize("tied", [True, False])
def test_learned_reparam_leaves_out_the_fixed_part(spec, monkeypatch, tied):
    """inference.find_best_learning_rate's learned_reparam (the engine replaced by a stand-in that returns a fit)"""
    from autoreparam_amd import engine, flags as flags_mod, graphs, inference
    cfg = collections.namedtuple("Cfg", "model")(spec)
    f = flags_mod.FlagValues()
    f.learning_rates, f.num_optimization_steps, f.num_mc_samples = [0.05], 40, 4
    _, _, elbo, vp, init = graphs.make_cvip_graph(cfg, tied_pparams=tied, flags=f)
    want = {"overall_log_scale_a", "beta_a"} if tied else {"overall_log_scale_a", "overall_log_scale_b", "beta_a", "beta_b"}
    assert set(init) == want

    class FakeEngine(object):
        def set_param(self, which, ab):
            a, b = ab
            assert a.shape == (spec.D,) and (a[1:63] == 1).all() and (b[1:63] == 1).all()

        def vi_run(self, lr, loc, rho, n_steps, n_mc, which=0, w=None, wb=None, **kw):
            assert (w is not None) and ((wb is None) == tied)
            return torch.zeros(len(lr), n_steps)
    monkeypatch.setattr(engine, "engine_for", lambda sp, dev=None: FakeEngine())
    f.device = "cpu"
    res = inference.find_best_learning_rate(elbo, vp, None, init, flags=f)
    rp = res[5]
    assert set(rp) == want
    assert rp["beta_a"].shape == (62,) and np.shape(rp["overall_log_scale_a"]) == ()
    if not tied:
        assert rp["beta_b"].shape == (62,)
