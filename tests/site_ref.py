"""Float64 evaluation of a latent site table (autoreparam_amd/models.py: SiteTable), written from the formulas of
ModelSpec.site_table's docstring and include/autoreparam.h: arp_site_logprior -- NOT from csrc/prior.hip, which is under
test against this file.  All functions take the table's columns as they are given (float64 from site_table(), or the
float32-rounded host copies of an uploaded table) and centred states x [R, D].

`parts(table, x)`     -> dict of the [R, D] pieces: loc, s, A_loc, A_s (the sums of absolute terms)
`elements(table, x)`  -> lp [R, D], the log density of every element
`groups(lp, group_of, G)` -> [R, G], the sums over the elements of every group, ascending d
`total(table, x)`     -> [R], the sum over all elements, ascending d
`bound(table, x)`     -> [R, D], the header's first-order error bound of a float32 elem_lp
`group_bound(lp32, bounds, group_of, G)` -> [R, G], the header's bound of group_lp from the device's own float32 values"""
import numpy as np

NORMAL, NORMAL_SOFTPLUS, LOG_GAMMA = 0, 1, 2
U32 = 2.0 ** -24


def _chain(x, idx, w, c):
    """(c + sum_t w[d][t] x[idx[d][t]], |c| + sum_t |w x|), [R, D] each"""
    idx, w = np.asarray(idx, np.int64), np.asarray(w, np.float64)
    value = np.broadcast_to(np.asarray(c, np.float64), x.shape).copy()
    size = np.abs(value)
    for t in range(idx.shape[1]):
        term = w[None, :, t] * x[:, idx[:, t]]
        value = value + term
        size = size + np.abs(term)
    return value, size


def parts(table, x):
    x = np.asarray(x, np.float64)
    loc, a_loc = _chain(x, table.loc_idx, table.loc_w, table.loc0)
    s, a_s = _chain(x, table.scale_idx, table.scale_w, table.log_scale0)
    return dict(x=x, loc=loc, s=s, A_loc=a_loc, A_s=a_s)


def _softplus(s):
    return np.maximum(s, 0.0) + np.log1p(np.exp(-np.abs(s)))


def elements(table, x):
    p = parts(table, x)
    x, loc, s = p["x"], p["loc"], p["s"]
    form = np.asarray(table.form)[None, :]
    norm = np.asarray(table.norm, np.float64)[None, :]
    with np.errstate(all="ignore"):
        z0 = (x - loc) * np.exp(-s)
        lp0 = -0.5 * z0 * z0 - s
        sigma = _softplus(s)
        z1 = (x - loc) / sigma
        lp1 = -0.5 * z1 * z1 - np.log(sigma)
        lp2 = np.asarray(table.loc0, np.float64)[None, :] * x - np.exp(s + x)
    return np.where(form == LOG_GAMMA, lp2, np.where(form == NORMAL_SOFTPLUS, lp1, lp0)) + norm


def groups(lp, group_of, G):
    lp, group_of = np.asarray(lp, np.float64), np.asarray(group_of)
    out = np.zeros((lp.shape[0], int(G)))
    for d in range(lp.shape[1]):
        out[:, group_of[d]] += lp[:, d]
    return out


def total(table, x):
    return groups(elements(table, x), np.zeros(len(np.asarray(table.form)), np.int64), 1)[:, 0]


def bound(table, x):
    """include/autoreparam.h: arp_site_logprior, the three forms' bounds of elem_lp, in float64"""
    p = parts(table, x)
    x, loc, s, a_loc, a_s = p["x"], p["loc"], p["s"], p["A_loc"], p["A_s"]
    lp = np.abs(elements(table, x))
    form = np.asarray(table.form)[None, :]
    with np.errstate(all="ignore"):
        ems = np.exp(-s)
        z0 = (x - loc) * ems
        b0 = 3.0 * a_loc * ems * np.abs(z0) + z0 * z0 * (5.0 + 3.0 * a_s) + 4.0 * a_s + lp
        sigma = _softplus(s)
        z1 = (x - loc) / sigma
        B = (3.0 * a_s + 3.0) / sigma + 1.0
        b1 = 3.0 * a_loc * np.abs(z1) / sigma + z1 * z1 * (4.0 + B) + B + 3.0 * np.abs(np.log(sigma)) + lp
        E = np.exp(s + x)
        b2 = 2.0 * np.abs(np.asarray(table.loc0, np.float64)[None, :] * x) + E * (3.0 + 3.0 * a_s + np.abs(s + x)) + lp
    return U32 * np.where(form == LOG_GAMMA, b2, np.where(form == NORMAL_SOFTPLUS, b1, b0))


def group_bound(lp32, bounds, group_of, G):
    """sum of the elements' bounds + (n_g + 4) 2^-53 sum |elem_lp| per group"""
    group_of = np.asarray(group_of)
    n_g = np.bincount(group_of, minlength=int(G))[None, :]
    return groups(bounds, group_of, G) + (n_g + 4.0) * 2.0 ** -53 * groups(np.abs(np.asarray(lp32, np.float64)), group_of, G)
