"""Model definitions for the hot path: the four hierarchical models named by
BASELINE.json plus radon_stddvs, neals_funnel, electric, time_series and
german_credit_gammascale, as frozen data + a model id the HIP engine understands.

Mirrors the reference's ``models.get_model_by_name(name, dataset) -> ModelConfig``
(models.py:51-54, 1144-1175).  In the reference ``ModelConfig.model`` is an
Edward2 program; here it is a :class:`ModelSpec` (same role: it defines the joint
density, evaluated natively by the engine instead of by TensorFlow).
"""
import collections
import copy
import math
import os

import numpy as np

from . import _lib

DATA_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")

ModelConfig = collections.namedtuple(
    "ModelConfig", ("model", "model_args", "observed_data", "to_centered",
                    "to_noncentered", "make_to_centered",
                    "make_to_partially_noncentered", "bijectors_fn"))


# ModelSpec.observation_table: the likelihood of every observation as arp_pointwise_loglik reads it
ObservationTable = collections.namedtuple("ObservationTable", ("kind", "idx", "w", "y", "scale_idx", "log_scale"))
OBS_NORMAL, OBS_BERNOULLI = 0, 1     # include/autoreparam.h: ARP_OBS_NORMAL, ARP_OBS_BERNOULLI
# ModelSpec.site_table: the prior of every latent element as arp_site_logprior reads it
SiteTable = collections.namedtuple("SiteTable", ("form", "loc_idx", "loc_w", "loc0", "scale_idx", "scale_w", "log_scale0",
                                                 "norm", "part"))
SITE_NORMAL, SITE_NORMAL_SOFTPLUS, SITE_LOG_GAMMA = 0, 1, 2     # include/autoreparam.h: ARP_SITE_*
SITE_TERMS = 2                                                  # ARP_SITE_TERMS


class ModelSpec(object):
    """Joint density of one model: id, latent parts in trace order, raw inputs."""

    def __init__(self, name, model_id, part_names, part_shapes, raw, observed, scalar_loc=(), scalar_scale=(),
                 fixed_parts=(), options=()):
        # vector parts whose reference random variable has a SCALAR loc / scale: with --notied_pparams the
        # reference gives `<rv>_a` the loc's shape and `<rv>_b` the scale's (program_transformations.py:486-533),
        # i.e. one shared value for the part
        self.scalar_loc = set(scalar_loc)
        self.scalar_scale = set(scalar_scale)
        # parts the reference's interceptors never reparameterise (not Normal random variables): they have no
        # `<rv>_a` / `<rv>_b`, and the kernels ignore whatever (a, b) they are given
        self.fixed_parts = set(fixed_parts)
        # (key, value) pairs for arp_model_set_option, applied when an Engine is created
        self.options = tuple(options)
        self.name = name
        self.model_id = model_id
        self.part_names = list(part_names)
        self.part_shapes = [tuple(s) for s in part_shapes]
        self.part_sizes = [int(np.prod(s)) if len(s) else 1 for s in self.part_shapes]
        self.offsets = np.concatenate([[0], np.cumsum(self.part_sizes)]).astype(int)
        self.D = int(self.offsets[-1])
        self.raw = raw            # dict of numpy arrays, as the reference's model_args hold them
        self.observed = observed  # dict name -> array, as the reference's observed_data

    # ---- flat [C, D] <-> list of [C, *event] parts (reference layout) ----
    def pack(self, parts, xp=np):
        cols = []
        for p, shp in zip(parts, self.part_shapes):
            p = xp.asarray(p) if xp is np else p
            cols.append(p.reshape(p.shape[0], -1))
        return xp.concatenate(cols, axis=1) if xp is np else xp.cat(cols, dim=1)

    def unpack(self, flat):
        out = []
        for k, shp in enumerate(self.part_shapes):
            sl = flat[..., self.offsets[k]:self.offsets[k + 1]]
            out.append(sl.reshape(tuple(flat.shape[:-1]) + shp))
        return out

    def ab_from_reparam(self, reparam):
        """Per-element VIP parameters (a, b), float32 [D].

        'CP' -> a=b=1, 'NCP' -> a=b=0, otherwise a dict with keys ``<rv>_a`` and
        optionally ``<rv>_b`` (missing ``_b`` means 1, exactly as the reference's
        get_or_init falls back at program_transformations.py:495-500; other keys
        such as ``*_prior_mean`` are ignored).
        Parts in ``fixed_parts`` need no entry; they take the value of the rest ('NCP': 0, else 1), which keeps the
        engine's CP / NCP classification of the whole vector.
        """
        a = np.ones(self.D, np.float32)
        b = np.ones(self.D, np.float32)
        if isinstance(reparam, str):
            if reparam == "CP":
                return a, b
            if reparam == "NCP":
                return np.zeros(self.D, np.float32), np.zeros(self.D, np.float32)
            raise ValueError("unknown parameterisation %r" % (reparam,))
        for k, name in enumerate(self.part_names):
            lo, hi = self.offsets[k], self.offsets[k + 1]
            if name in self.fixed_parts:
                continue
            if name + "_a" not in reparam:
                raise KeyError("parameterisation has no entry for %s_a" % name)
            a[lo:hi] = np.broadcast_to(np.asarray(reparam[name + "_a"], np.float32).reshape(-1), (hi - lo,))
            if name + "_b" in reparam:
                b[lo:hi] = np.broadcast_to(np.asarray(reparam[name + "_b"], np.float32).reshape(-1), (hi - lo,))
        return a, b

    def untied_groups(self):
        """(a_group, b_group) int32 [D] for arp_vi_io: leader element of every element's untied a / b variable."""
        ag, bg = np.arange(self.D, dtype=np.int32), np.arange(self.D, dtype=np.int32)
        for k, name in enumerate(self.part_names):
            lo, hi = self.offsets[k], self.offsets[k + 1]
            if name in self.scalar_loc:
                ag[lo:hi] = lo
            if name in self.scalar_scale:
                bg[lo:hi] = lo
        return ag, bg

    def untied_shape(self, name, which):
        """shape of the reference's untied `<name>_a` (which='a') / `<name>_b` variable"""
        k = self.part_names.index(name)
        shared = name in (self.scalar_loc if which == "a" else self.scalar_scale)
        return () if shared else self.part_shapes[k]

    def with_observations(self, y):
        """A spec of the same model on other observations: `raw["y"]` and every entry of `observed` hold `y` (anything numpy
        reads, one value per observation, in observation_table's order) in the original's dtypes and shapes; everything
        else -- covariates, parts, options -- is shared with this spec, which is not touched.  What a refit on replicated
        data runs on (sbc.run_sbc).  A model without observations (neals_funnel) is refused."""
        if "y" not in self.raw:
            raise ValueError("%s has no observations to replace" % self.name)
        old = np.asarray(self.raw["y"])
        y = np.asarray(y)
        if y.size != old.size:
            raise ValueError("%s: %d observations are required, not %d" % (self.name, old.size, y.size))
        new = copy.copy(self)
        new.raw = dict(self.raw)
        new.raw["y"] = np.ascontiguousarray(y.reshape(old.shape).astype(old.dtype))
        new.observed = {name: new.raw["y"].reshape(np.shape(v)).astype(np.asarray(v).dtype) for name, v in self.observed.items()}
        return new

    def observation_table(self):
        """One row per observation for `arp_pointwise_loglik` -> ObservationTable, or None for a model without data
        (neals_funnel).  Every likelihood here is Normal or Bernoulli-logit over a linear predictor of the CENTRED latents,
        eta_n = sum_t w[n][t] x[idx[n][t]], with the log-scale s_n = log_scale[n] + (x[scale_idx[n]] if scale_idx[n] >= 0):
        kind (OBS_NORMAL / OBS_BERNOULLI), idx [N, T] int32, w [N, T] float32 (T the model's largest term count; padding
        terms have w = 0, idx = 0), y [N] float32, scale_idx [N] int32, log_scale [N] float32.  A function of the data
        alone: one table serves every parameterisation, since the trace is centred.  The reference's one-hot quirks are
        restated as csrc/arp_build.hip restates them for the sufficient statistics: an index outside [0, depth) is an
        all-zero one-hot row -- a term of weight 0 and, for electric's grade, scale_idx = -1 with log_scale = 0; radon_stddvs
        refuses such a county as its builder does (the observation's scale would be 0)."""
        r, off = self.raw, dict(zip(self.part_names, (int(o) for o in self.offsets[:-1])))
        mid = self.model_id
        if mid == _lib.MODEL_NEALS_FUNNEL:
            return None

        def term(base, index, depth, weight):
            """(idx, w) columns of a one-hot term: x[base + index] * weight where 0 <= index < depth, weight 0 elsewhere."""
            index = np.asarray(index).astype(np.int64).reshape(-1)
            ok = (index >= 0) & (index < depth)
            weight = np.broadcast_to(np.asarray(weight, np.float32), index.shape)
            return np.where(ok, base + index, 0), np.where(ok, weight, np.float32(0.0))

        y = np.asarray(r["y"], np.float32).reshape(-1)
        N = y.size
        kind, scale_idx, log_scale = OBS_NORMAL, np.full(N, -1), np.zeros(N, np.float32)
        if mid == _lib.MODEL_EIGHT_SCHOOLS:
            terms = [(off["theta"] + np.arange(N), np.ones(N, np.float32))]
            log_scale = np.log(np.asarray(r["sigma"], np.float64))
        elif mid in (_lib.MODEL_RADON, _lib.MODEL_RADON_STDDVS):
            J = len(r["u"])
            county = np.asarray(r["county"]).astype(np.int64).reshape(-1)
            terms = [term(off["m"], county, J, 1.0), (np.full(N, off["b2"]), np.asarray(r["x"], np.float32))]
            if mid == _lib.MODEL_RADON_STDDVS:
                if np.any((county < 0) | (county >= J)):
                    raise ValueError("radon_stddvs: county index out of range")
                scale_idx = off["log_m_stddv"] + county
        elif mid == _lib.MODEL_GERMAN_CREDIT:
            kind = OBS_BERNOULLI
            X = np.asarray(r["X"], np.float32)
            F = X.shape[1]
            terms = [(np.full(N, off["beta"] + f), X[:, f]) for f in range(F)]
        elif mid == _lib.MODEL_ELECTION:
            kind = OBS_BERNOULLI
            terms = [term(off["a"], r["state"], int(r["n_state"]), 1.0),
                     (np.full(N, off["b2"]), np.asarray(r["female"], np.float32)),
                     (np.full(N, off["b1"]), np.asarray(r["black"], np.float32))]
        elif mid == _lib.MODEL_ELECTRIC:
            G = int(r["n_grade"])
            grade = np.asarray(r["grade"]).astype(np.int64).reshape(-1)
            terms = [term(off["a"], r["pair"], int(r["n_pair"]), 1.0),
                     term(off["b"], grade, G, np.asarray(r["treatment"], np.float32))]
            scale_idx = np.where((grade >= 0) & (grade < G), off["sigma_y"] + grade, -1)
        elif mid == _lib.MODEL_TIME_SERIES:
            terms = [(np.asarray([off["alpha%d" % t] for t in range(N)]), np.ones(N, np.float32)),
                     (np.full(N, off["beta"]), np.asarray(r["x"], np.float32))]
            log_scale = np.full(N, np.log(0.12))
        else:
            raise ValueError("unknown model id")
        idx = np.ascontiguousarray(np.stack([np.asarray(i) for i, _ in terms], axis=1).astype(np.int32))
        w = np.ascontiguousarray(np.stack([np.asarray(v, np.float32) for _, v in terms], axis=1).astype(np.float32))
        idx[w == 0] = 0          # (a term of weight 0 reads element 0: padding and zero one-hot rows alike)
        return ObservationTable(kind, idx, w, y, np.ascontiguousarray(scale_idx, dtype=np.int32),
                                np.ascontiguousarray(log_scale, dtype=np.float32))

    def site_table(self):
        """One row per latent element d, in trace order, for `arp_site_logprior` -> SiteTable: the prior-side twin of
        observation_table.  Every latent site here is a Normal whose loc and log-scale are affine in at most SITE_TERMS
        EARLIER elements of the centred state, or the log of a Gamma variable:
          loc_d = loc0[d] + sum_t loc_w[d][t] x[loc_idx[d][t]],  s_d = log_scale0[d] + sum_t scale_w[d][t] x[scale_idx[d][t]]
          form SITE_NORMAL:           x_d ~ Normal(loc_d, exp(s_d))
          form SITE_NORMAL_SOFTPLUS:  x_d ~ Normal(loc_d, softplus(s_d))
          form SITE_LOG_GAMMA:        x_d = log g, g ~ Gamma(shape loc0[d], rate exp(s_d)): lp = loc0 x - exp(s + x) + norm
        form, part [D] int32; loc_idx, scale_idx [D, 2] int32; loc_w, scale_w [D, 2], loc0, log_scale0, norm [D] float64
        (the uploader rounds them to float32); padding terms have w = 0, idx = 0.  norm is the additive normaliser:
        -0.5 log(2 pi) for a Normal, shape log(rate) - lgamma(shape) for the log-Gamma form.  part[d] indexes part_names.
        The rows restate the reference's model programs (the lines: oracle/ed2_ref.py's header and
        _spec_german_gammascale's docstring); electric's one-hot quirk is restated as observation_table restates it -- a
        grade_pair outside [0, depth) is a term of weight 0.  Every term of non-zero weight points at an element before
        d (the ancestral order: the table can be walked front to back to draw from the prior); asserted here.  A function
        of the data alone, as observation_table is."""
        r, off = self.raw, dict(zip(self.part_names, (int(o) for o in self.offsets[:-1])))
        mid, D = self.model_id, self.D
        form = np.full(D, SITE_NORMAL, np.int32)
        loc_idx, scale_idx = np.zeros((D, SITE_TERMS), np.int32), np.zeros((D, SITE_TERMS), np.int32)
        loc_w, scale_w = np.zeros((D, SITE_TERMS)), np.zeros((D, SITE_TERMS))
        loc0, log_scale0, norm = np.zeros(D), np.zeros(D), np.full(D, -0.5 * np.log(2.0 * np.pi))

        def rows(name):
            k = self.part_names.index(name)
            return np.arange(self.offsets[k], self.offsets[k + 1])

        def term(idx_col, w_col, name, t, index, weight):
            """term t of the part's rows: weight * x[index] (arrays over the part's elements, or scalars)"""
            d = rows(name)
            index, weight = np.broadcast_to(np.asarray(index), d.shape), np.broadcast_to(np.asarray(weight, np.float64), d.shape)
            idx_col[d, t] = np.where(weight != 0, index, 0)
            w_col[d, t] = weight

        if mid == _lib.MODEL_EIGHT_SCHOOLS:
            log_scale0[rows("mu")] = log_scale0[rows("log_tau")] = np.log(5.0)
            term(loc_idx, loc_w, "theta", 0, off["mu"], 1.0)
            term(scale_idx, scale_w, "theta", 0, off["log_tau"], 1.0)
        elif mid in (_lib.MODEL_RADON, _lib.MODEL_RADON_STDDVS):
            term(loc_idx, loc_w, "m", 0, off["mua"], 1.0)
            term(loc_idx, loc_w, "m", 1, off["b1"], np.asarray(r["u"], np.float64).reshape(-1))
        elif mid == _lib.MODEL_NEALS_FUNNEL:
            log_scale0[rows("x1")] = np.log(3.0)
            term(scale_idx, scale_w, "x2", 0, off["x1"], 0.5)
        elif mid == _lib.MODEL_GERMAN_CREDIT:
            log_scale0[rows("overall_log_scale")] = np.log(10.0)
            bls = rows("beta_log_scales")
            if dict(self.options).get("german_prior") == "gamma":
                shape, rate = 0.5, 0.5
                form[bls] = SITE_LOG_GAMMA
                loc0[bls], log_scale0[bls] = shape, np.log(rate)
                norm[bls] = shape * np.log(rate) - math.lgamma(shape)
                term(scale_idx, scale_w, "beta", 0, off["overall_log_scale"], 1.0)
                term(scale_idx, scale_w, "beta", 1, bls, 1.0)
            else:
                term(loc_idx, loc_w, "beta_log_scales", 0, off["overall_log_scale"], 1.0)
                term(scale_idx, scale_w, "beta", 0, bls, 1.0)
        elif mid == _lib.MODEL_ELECTION:
            for name in ("mua", "b1", "b2"):
                log_scale0[rows(name)] = np.log(100.0)
            log_scale0[rows("log_sigma_a")] = np.log(10.0)
            term(loc_idx, loc_w, "a", 0, off["mua"], 1.0)
            term(scale_idx, scale_w, "a", 0, off["log_sigma_a"], 1.0)
        elif mid == _lib.MODEL_ELECTRIC:
            log_scale0[rows("b")] = np.log(100.0)
            gp = np.asarray(r["grade_pair"]).astype(np.int64).reshape(-1)
            ok = (gp >= 0) & (gp < int(r["n_grade_pair"]))
            term(loc_idx, loc_w, "a", 0, off["mua"] + np.where(ok, gp, 0), np.where(ok, 100.0, 0.0))
        elif mid == _lib.MODEL_TIME_SERIES:
            for t in range(len(r["y"])):
                for name, sigma in (("alpha%d" % t, "sigma_alpha"), ("mu%d" % t, "sigma_mu")):
                    form[rows(name)] = SITE_NORMAL_SOFTPLUS
                    term(scale_idx, scale_w, name, 0, off[sigma], 1.0)
                if t > 0:
                    term(loc_idx, loc_w, "alpha%d" % t, 0, off["alpha%d" % (t - 1)], 1.0)
                    term(loc_idx, loc_w, "alpha%d" % t, 1, off["mu%d" % (t - 1)], 1.0)
                    term(loc_idx, loc_w, "mu%d" % t, 0, off["mu%d" % (t - 1)], 1.0)
        else:
            raise ValueError("unknown model id")
        part = np.repeat(np.arange(len(self.part_names)), self.part_sizes).astype(np.int32)
        d = np.arange(D)[:, None]
        assert all(np.all((w == 0) | (i < d)) for i, w in ((loc_idx, loc_w), (scale_idx, scale_w))), "site table: not ancestral"
        return SiteTable(form, loc_idx, loc_w, loc0, scale_idx, scale_w, log_scale0, norm, part)

    def dataset(self):
        """(ctypes Dataset, keep-alive list) for arp_model_create."""
        keep = []

        def f32(x):
            arr = np.ascontiguousarray(x, dtype=np.float32)
            keep.append(arr)
            return arr.ctypes.data_as(_lib._f32p)

        def i32(x):
            arr = np.ascontiguousarray(x, dtype=np.int32)
            keep.append(arr)
            return arr.ctypes.data_as(_lib._i32p)

        d = _lib.Dataset()
        d.model = self.model_id
        r = self.raw
        if self.model_id in (_lib.MODEL_RADON, _lib.MODEL_RADON_STDDVS):
            d.n_obs = len(r["y"]); d.n_groups = len(r["u"])
            d.group_host = i32(r["county"]); d.u_host = f32(r["u"])
            d.x_host = f32(r["x"]); d.y_host = f32(r["y"])
        elif self.model_id == _lib.MODEL_EIGHT_SCHOOLS:
            d.n_obs = 8; d.n_groups = 8
            d.u_host = f32(r["sigma"]); d.y_host = f32(r["y"])
        elif self.model_id == _lib.MODEL_ELECTION:
            d.n_obs = len(r["y"]); d.n_groups = int(r["n_state"])
            d.group_host = i32(r["state"]); d.x_host = f32(r["female"]); d.x2_host = f32(r["black"])
            d.y_host = f32(r["y"])
        elif self.model_id == _lib.MODEL_NEALS_FUNNEL:
            pass
        elif self.model_id == _lib.MODEL_TIME_SERIES:
            d.n_obs = len(r["y"]); d.x_host = f32(r["x"]); d.y_host = f32(r["y"])
        elif self.model_id == _lib.MODEL_ELECTRIC:
            if int(r["n_grade"]) != int(r["n_grade_pair"]):
                raise ValueError("electric: n_grade and n_grade_pair must agree")
            d.n_obs = len(r["y"]); d.n_groups = int(r["n_pair"]); d.n_features = int(r["n_grade"])
            d.group_host = i32(r["pair"]); d.group2_host = i32(r["grade"]); d.group3_host = i32(r["grade_pair"])
            d.x_host = f32(r["treatment"]); d.y_host = f32(r["y"])
        elif self.model_id == _lib.MODEL_GERMAN_CREDIT:
            d.n_obs = r["X"].shape[0]; d.n_features = r["X"].shape[1]
            d.X_host = f32(r["X"]); d.y_host = f32(r["y"])
        else:
            raise ValueError("unknown model id")
        return d, keep


def _load(fname):
    path = os.path.join(DATA_DIR, fname)
    if not os.path.exists(path):
        raise IOError("frozen dataset %s not found (tools/freeze_data.py writes it)" % path)
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _spec_eight_schools():
    r = _load("eight_schools.npz")
    return ModelSpec("8schools", _lib.MODEL_EIGHT_SCHOOLS, ["mu", "log_tau", "theta"],
                     [(), (), (8,)], r, {"y": r["y"]})


def _spec_radon(state_code):
    r = _load("radon_%s.npz" % state_code)
    J = len(r["u"])
    return ModelSpec("radon", _lib.MODEL_RADON, ["mua", "b1", "b2", "m"], [(), (), (), (J,)],
                     r, {"y": r["y"].reshape(-1, 1)})


def _spec_radon_stddvs(state_code):
    """radon with inferred per-county observation scales (reference models.py:763-806)."""
    r = _load("radon_%s.npz" % state_code)
    J = len(r["u"])
    return ModelSpec("radon_stddvs", _lib.MODEL_RADON_STDDVS, ["mua", "b1", "b2", "m", "log_m_stddv"],
                     [(), (), (), (J,), (J,)], r, {"y": r["y"].reshape(-1, 1)})


def _spec_funnel():
    return ModelSpec("neals_funnel", _lib.MODEL_NEALS_FUNNEL, ["x1", "x2"], [(), ()], {}, {})


def _spec_electric():
    """electric company (reference models.py:1011-1066); `a` keeps the reference's [n_pair, 1] shape."""
    r = _load("electric.npz")
    P, G = int(r["n_pair"]), int(r["n_grade"])
    return ModelSpec("electric", _lib.MODEL_ELECTRIC, ["mua", "sigma_y", "a", "b"],
                     [(int(r["n_grade_pair"]),), (G,), (P, 1), (G,)], r, {"y": r["y"]},
                     scalar_loc=("mua", "sigma_y", "b"), scalar_scale=("a",))


def _spec_time_series():
    """local linear trend (reference models.py:1069-1141): every latent is its own scalar random variable, in
    trace order sigma_alpha, sigma_mu, alpha0, mu0, alpha1, mu1, ..., beta."""
    r = _load("time_series.npz")
    T = len(r["y"])
    names = ["sigma_alpha", "sigma_mu"] + [n for t in range(T) for n in ("alpha%d" % t, "mu%d" % t)] + ["beta"]
    return ModelSpec("time_series", _lib.MODEL_TIME_SERIES, names, [()] * len(names), r, {"y": r["y"]})


def _spec_german():
    r = _load("german_credit.npz")
    F = r["X"].shape[1]
    return ModelSpec("german_credit_lognormalcentered", _lib.MODEL_GERMAN_CREDIT,
                     ["overall_log_scale", "beta_log_scales", "beta"], [(), (F,), (F,)],
                     r, {"y": r["y"][np.newaxis, ...]}, scalar_loc=("beta_log_scales",))


def _spec_german_gammascale():
    """German credit with Gamma(1/2, 1/2) priors on the feature scales (reference models.py:926-964): the same data,
    parts and likelihood as the log-normal model; beta_log_scales is the log of a Gamma variable, which the reference's
    interceptors do not reparameterise."""
    r = _load("german_credit.npz")
    F = r["X"].shape[1]
    return ModelSpec("german_credit_gammascale", _lib.MODEL_GERMAN_CREDIT,
                     ["overall_log_scale", "beta_log_scales", "beta"], [(), (F,), (F,)],
                     r, {"y": r["y"][np.newaxis, ...]}, fixed_parts=("beta_log_scales",),
                     options=(("german_prior", "gamma"),))


def _spec_election():
    r = _load("election88.npz")
    S = int(r["n_state"])
    return ModelSpec("election", _lib.MODEL_ELECTION, ["mua", "log_sigma_a", "a", "b1", "b2"],
                     [(), (), (S,), (), ()], r, {"y": r["y"].reshape(-1, 1)}, scalar_loc=("a",))


def spec_by_name(model_name, dataset=None):
    """The ModelSpec get_model_by_name builds its ModelConfig around: the frozen data and the latent parts, nothing on the
    device."""
    if model_name == "8schools":
        spec = _spec_eight_schools()
    elif model_name == "radon":
        spec = _spec_radon(dataset if dataset else "MN")
    elif model_name == "neals_funnel":
        spec = _spec_funnel()
    elif model_name == "radon_stddvs":
        spec = _spec_radon_stddvs(dataset if dataset else "MN")
    elif model_name == "electric":
        spec = _spec_electric()
    elif model_name == "time_series":
        spec = _spec_time_series()
    elif model_name == "german_credit_lognormalcentered":
        spec = _spec_german()
    elif model_name == "german_credit_gammascale":
        spec = _spec_german_gammascale()
    elif model_name in ("election", "election88"):
        spec = _spec_election()
    else:
        raise Exception("unknown model {} (this build covers 8schools, radon, radon_stddvs, "
                        "neals_funnel, electric, time_series, german_credit_lognormalcentered, "
                        "german_credit_gammascale, election)".format(model_name))
    return spec


def get_model_by_name(model_name, dataset=None):
    """Reference: models.py:1144-1175 (the four BASELINE models and the scalar-Normal hierarchical models of
    SURVEY 8f-3; the GP / MVN / Wishart models are out of scope)."""
    return model_config_for(spec_by_name(model_name, dataset))


def model_config_for(spec):
    """The ModelConfig around a ModelSpec: what get_model_by_name returns for the frozen data, and what a refit on
    replicated data (ModelSpec.with_observations; sbc.run_sbc) is handed."""
    from . import engine  # deferred: converters run on the device

    varnames = spec.part_names
    noncentered = {p: 0. for v in varnames for p in (v + "_a", v + "_b", v + "_c")}
    make_to_centered = engine.build_make_to_centered(spec)
    make_to_partially_noncentered = engine.build_make_to_partially_noncentered(spec)
    to_centered = make_to_centered(**noncentered)
    to_noncentered = make_to_partially_noncentered(**noncentered)
    return ModelConfig(spec, [], spec.observed, to_centered, to_noncentered, make_to_centered,
                       make_to_partially_noncentered, None)
