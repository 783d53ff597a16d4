"""Float64 pointwise log-likelihoods of the models with data, written from the reference's model programs (its models.py,
lines cited per model) and the frozen datasets under autoreparam_amd/data -- NOT through ModelSpec.observation_table,
which is itself under test against this file.  tf.one_hot is restated literally: a dense 0/1 matrix whose row is all
zero for an index outside [0, depth).

`predictor(spec, x)` -> (kind, eta [R, N], s [R, N], y [N]) for centred states x [R, D] in trace order;
`loglik(spec, x)` -> ll [R, N];  kind 0: Normal(eta, exp(s)), kind 1: Bernoulli(logits = eta)."""
import numpy as np

NORMAL, BERNOULLI = 0, 1
HALF_LOG_2PI = 0.9189385332046727


def one_hot(index, depth):
    index = np.asarray(index).astype(np.int64).reshape(-1)
    out = np.zeros((index.size, int(depth)), np.float64)
    ok = (index >= 0) & (index < depth)
    out[np.flatnonzero(ok), index[ok]] = 1.0
    return out


def _parts(spec, x):
    x = np.asarray(x, np.float64)
    return {name: part for name, part in zip(spec.part_names, spec.unpack(x))}


def _schools(spec, x):
    # models.py:139-147: y ~ Normal(theta, stddevs)
    p, r = _parts(spec, x), spec.raw
    eta = p["theta"]
    s = np.broadcast_to(np.log(np.asarray(r["sigma"], np.float64)), eta.shape)
    return NORMAL, eta, s, np.asarray(r["y"], np.float64)


def _radon(spec, x):
    # models.py:826-837: y_mu = C m + x b2, C = one_hot(county, J); scale sigma_y = 1
    p, r = _parts(spec, x), spec.raw
    C = one_hot(r["county"], len(r["u"]))
    eta = p["m"] @ C.T + p["b2"][:, None] * np.asarray(r["x"], np.float64)[None, :]
    return NORMAL, eta, np.zeros_like(eta), np.asarray(r["y"], np.float64)


def _radon_stddvs(spec, x):
    # models.py:772-788: y_mu as radon; y_stddv = C exp(log_m_stddv)
    p, r = _parts(spec, x), spec.raw
    C = one_hot(r["county"], len(r["u"]))
    eta = p["m"] @ C.T + p["b2"][:, None] * np.asarray(r["x"], np.float64)[None, :]
    with np.errstate(divide="ignore"):
        s = np.log(np.exp(p["log_m_stddv"]) @ C.T)
    return NORMAL, eta, s, np.asarray(r["y"], np.float64)


def _german(spec, x):
    # models.py:903-904 (and 944-945): logits = all_x . beta, y ~ Bernoulli(logits)
    p, r = _parts(spec, x), spec.raw
    eta = p["beta"] @ np.asarray(r["X"], np.float64).T
    return BERNOULLI, eta, np.zeros_like(eta), np.asarray(r["y"], np.float64).reshape(-1)


def _election(spec, x):
    # models.py:978-982: y_hat = C a + female b2 + black b1, C = one_hot(state, n_state)
    p, r = _parts(spec, x), spec.raw
    C = one_hot(r["state"], int(r["n_state"]))
    eta = (p["a"] @ C.T + p["b2"][:, None] * np.asarray(r["female"], np.float64)[None, :]
           + p["b1"][:, None] * np.asarray(r["black"], np.float64)[None, :])
    return BERNOULLI, eta, np.zeros_like(eta), np.asarray(r["y"], np.float64).reshape(-1)


def _electric(spec, x):
    # models.py:1016-1035: y_hat = C_pair a + (C_grade b) treatment, scale exp(C_grade sigma_y)
    p, r = _parts(spec, x), spec.raw
    Cp = one_hot(r["pair"], int(r["n_pair"]))
    Cg = one_hot(r["grade"], int(r["n_grade"]))
    a = p["a"].reshape(p["a"].shape[0], -1)
    eta = a @ Cp.T + (p["b"] @ Cg.T) * np.asarray(r["treatment"], np.float64)[None, :]
    s = p["sigma_y"] @ Cg.T
    return NORMAL, eta, s, np.asarray(r["y"], np.float64)


def _time_series(spec, x):
    # models.py:1096: y ~ Normal(stack(alpha) + beta x, 0.12)
    p, r = _parts(spec, x), spec.raw
    T = len(r["y"])
    alpha = np.stack([p["alpha%d" % t] for t in range(T)], axis=1)
    eta = alpha + p["beta"][:, None] * np.asarray(r["x"], np.float64)[None, :]
    return NORMAL, eta, np.full_like(eta, np.log(0.12)), np.asarray(r["y"], np.float64)


_BY_NAME = {"8schools": _schools, "radon": _radon, "radon_stddvs": _radon_stddvs,
            "german_credit_lognormalcentered": _german, "german_credit_gammascale": _german,
            "election": _election, "electric": _electric, "time_series": _time_series}
MODELS_WITH_DATA = tuple(_BY_NAME)


def predictor(spec, x):
    return _BY_NAME[spec.name](spec, x)


def loglik_from(kind, eta, s, y):
    """The two likelihoods in float64, the Bernoulli one in its stable form."""
    y = np.asarray(y, np.float64)
    if kind == NORMAL:
        z = (y - eta) * np.exp(-s)
        return -0.5 * z * z - s - HALF_LOG_2PI
    return y * eta - (np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta))))


def loglik(spec, x):
    kind, eta, s, y = predictor(spec, x)
    return loglik_from(kind, eta, s, y)
