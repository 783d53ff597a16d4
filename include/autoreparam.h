/*
 * autoreparam.h -- C ABI of the MI355X-native HMC / mean-field-VI engine.
 *
 * This is the drop-in boundary for the hot path of mgorinova/autoreparam.  The
 * reference has NO native interface for this path (it is pure Python on
 * TensorFlow-Probability); each entry point below names the
 * reference call it replaces so a maintainer can bind it with ctypes
 * (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain C types only; every array pointer is a DEVICE pointer (HBM, gfx950)
 *     unless the parameter name ends in `_host`;
 *   - the caller owns every buffer; the library never frees caller memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     calls only enqueue work, they never synchronise (one exception: arp_vi_run, see there);
 *   - every function returns 0 on success, non-zero on failure, and
 *     arp_last_error() then returns a human readable message (thread local);
 *   - chain states use the reference layout: the model's latent parts,
 *     flattened and concatenated in trace order, one row per chain,
 *     row-major float32 `[C][D]`  (reference: list of `[C,*event]` tensors,
 *     inference.py:207-216).
 *   - threads: a handle is used by one thread at a time; different handles (same device or not) may be
 *     driven from different threads concurrently, each on a stream of its own -- results do not depend on
 *     it.  arp_vi_run's multi-workgroup launches need their groups resident together: the library runs
 *     them one at a time per process; across processes sharing a device, or beside another kernel that
 *     holds the device for seconds, a hand-off that waits 2 s makes the call fail instead of hanging.
 */
#ifndef AUTOREPARAM_H_
#define AUTOREPARAM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARP_ABI_VERSION 2

/* Models on the hot path (reference models.py:131-166, 809-857, 884-923, 967-1008). */
enum {
  ARP_MODEL_EIGHT_SCHOOLS = 0,
  ARP_MODEL_RADON = 1,
  ARP_MODEL_GERMAN_CREDIT = 2, /* german_credit_lognormalcentered; german_credit_gammascale with option "german_prior" */
  ARP_MODEL_ELECTION = 3,
  ARP_MODEL_NEALS_FUNNEL = 5, /* models.py:671-696; no dataset fields are read */
  ARP_MODEL_RADON_STDDVS = 4, /* radon with per-county observation scales, models.py:763-806 */
  ARP_MODEL_ELECTRIC = 6,     /* electric company, models.py:1011-1066 */
  ARP_MODEL_TIME_SERIES = 7   /* local linear trend, models.py:1069-1141: n_obs = T, x = years, y = series */
};

/* Step-size adaptation wrapped around the HMC transition. */
enum {
  ARP_ADAPT_NONE = 0,   /* fixed step (parity runs) */
  ARP_ADAPT_DUAL = 1,   /* tfp.mcmc.DualAveragingStepSizeAdaptation defaults, inference.py:224-226 */
  ARP_ADAPT_SIMPLE = 2  /* tfp.mcmc.SimpleStepSizeAdaptation(rate, target), inference.py:288-306 */
};

/* Raw model inputs exactly as the reference's `model_args` / `observed_data`
 * hold them (HOST pointers; copied at create time).  Unused fields are NULL/0. */
typedef struct arp_dataset {
  int32_t model;        /* ARP_MODEL_* */
  int32_t n_obs;        /* N */
  int32_t n_groups;     /* radon: J counties; election: n_state; schools: 8; electric: n_pair */
  int32_t n_features;   /* german: 62; electric: n_grade (= n_grade_pair, at most 4) */
  const int32_t* group_host;   /* [N] radon county (0-based) / election state / electric pair (both 1-based, as the reference feeds tf.one_hot) */
  const float* u_host;         /* radon: [J] log uranium; schools: [8] treatment stddevs */
  const float* x_host;         /* radon: [N] floor; election: [N] female; electric: [N] treatment (0/1) */
  const float* x2_host;        /* election: [N] black */
  const float* y_host;         /* [N] observations (Bernoulli outcomes as 0/1 floats); schools: [8] effects */
  const float* X_host;         /* german: [N][n_features] row-major design matrix */
  const int32_t* group2_host;  /* electric: [N] grade (1-based, as fed to tf.one_hot) */
  const int32_t* group3_host;  /* electric: [n_groups] grade_pair (1-based) */
} arp_dataset;

typedef struct arp_model arp_model; /* opaque: frozen data + sufficient statistics, on one device */

/* One segment of `n_steps` HMC transitions over `n_chains` chains (replaces one
 * stretch of tfp.mcmc.sample_chain's while-loop, inference.py:228-236). */
typedef struct arp_hmc_config {
  int32_t n_chains;          /* C on this device */
  int32_t n_leapfrog;        /* L */
  int32_t n_steps;           /* transitions in this call */
  int64_t step_base;         /* transitions already done for these chains (0 on the first call) */
  int64_t chain_offset;      /* global id of chain 0 on this device (RNG keying; multi-GPU sharding) */
  uint64_t seed;
  int32_t adapt_kind;        /* ARP_ADAPT_* */
  int32_t n_adapt;           /* num_adaptation_steps */
  float adapt_target;        /* target accept prob (0.75) */
  float adapt_rate;          /* SIMPLE: adaptation_rate (0.05) */
  /* trace schedule, sample_chain semantics: result s is taken after transition
   * 1 + n_burnin + s*thin (thin = 1 + num_steps_between_results). */
  int32_t n_burnin;
  int32_t thin;
  int32_t n_samples;         /* S: capacity of the trace buffers (rows) */
  int32_t trace_centered;    /* 1: trace rows are mapped to centred coordinates (inference.py:238-239) */
  int32_t lanes_per_chain;   /* 0 = library default; otherwise 1,2,4,8,16 (also partitions the RNG streams) */
  int32_t stats_batch;       /* io.stats: samples per batch of the batch-means accumulators (>= 1) */
  int32_t trace_chains;      /* 0 or >= n_chains: trace rows hold every chain; otherwise only chains [0, trace_chains)
                              * are recorded and a trace row is [trace_chains][D] (a few chains kept next to io.stats) */
  int32_t reserved;
} arp_hmc_config;

/* Per-chain persistent state ("kernel results") + outputs.  All DEVICE pointers. */
typedef struct arp_hmc_io {
  float* q;                  /* [C][D] in/out current state (reparameterised coordinates) */
  float* grad;               /* [C][D] in/out cached gradient at q (ignored when step_base == 0) */
  float* logp;               /* [C]    in/out cached log-density at q (additive constants dropped) */
  float* adapt;              /* [C][4] in/out {step multiplier kappa, error sum, log-averaged multiplier, unused} */
  uint32_t* rng;             /* [C][16][4] in/out stream states, one 16-byte record per RNG slot (MWC64X: x, carry, 0, 0) */
  uint32_t* accept_count;    /* [C] in/out accepted transitions */
  const float* eps0;         /* [D] base step size per element (VI posterior std / (L/4)^2, inference.py:212-216) */
  float* trace;              /* [S][C][D] or NULL */
  uint8_t* trace_accept;     /* [S][C] is_accepted of recorded transitions, or NULL */
  float* stats;              /* [6][C][D] in/out or NULL: streaming statistics of the recorded samples (same schedule and
                              * coordinates as the trace rows), accumulated in the kernel so that a run needs no trace:
                              * {ref = a reference level near the samples, s1 = sum (x - ref), s2 = sum (x - ref)^2, cur = s1 at
                              * the start of the current batch, sb1 = sum of batch means (of x - ref), sb2 = sum of their
                              * squares}; zero it before the first call.  mean = ref + s1/n, var = (s2 - s1^2/n)/(n-1),
                              * batch-means ESS = n var / (stats_batch var(batch means)).  ref is chosen by
                              * the kernel and is only meaningful through these formulas (until the first batch ends the
                              * first recorded sample, or -- kernels that keep the running moments of a batch in LDS and touch
                              * the planes once per batch or launch -- the mean of the first stretch they fold; from then on
                              * the mean of the first batch, every sum re-referenced to it in place, which keeps the float32
                              * sums conditioned); the planes are sums, so they are exact to rounding however a run is cut
                              * into launches */
  uint32_t* rec_accept_count; /* [C] in/out or NULL: accepted transitions among the recorded ones (sum of is_accepted) */
} arp_hmc_io;

int arp_version(void);
const char* arp_last_error(void);

/* Build a model handle on the current HIP device: copies the data, derives the
 * per-group sufficient statistics and uploads them. */
int arp_model_create(const arp_dataset* data, arp_model** out);
int arp_model_destroy(arp_model* m);
int arp_model_dim(const arp_model* m);                 /* D */
/* Per-handle options (no reference counterpart).  "german_math": how german credit's likelihood contraction runs at 4 lanes
 * per chain -- "f32" = f32 matrix cores (v_mfma_f32_16x16x4_f32, exact f32 products), "bf16x3" = bf16 matrix cores with every
 * operand as three bf16 pieces (six leading cross products: f32-equivalent, error ~ 2^-23 per product; needs a design matrix
 * with at most 8 columns that are not exact in one bf16 piece -- the reference's data have 7), "auto" (default) = bf16x3 where
 * the data allow it.  "german_prior": the prior of german credit's feature scales -- "lognormal" (default) =
 * german_credit_lognormalcentered, beta_log_scales ~ N(overall_log_scale, 1), beta ~ N(0, exp(beta_log_scales)); "gamma" =
 * german_credit_gammascale, beta_log_scales = log g, g ~ Gamma(1/2, 1/2), beta ~ N(0, exp(overall_log_scale +
 * beta_log_scales)), where beta_log_scales is never reparameterised (its a, b are ignored) and no a has any effect.  Same
 * data, dimension, state layout, random streams and dropped constant; takes effect from the next launch.  "vi_launch": how arp_vi_run starts a launch whose workgroups wait for each other inside the launch --
 * "cooperative" = hipLaunchCooperativeKernel (the runtime checks the grid against the device's capacity and serialises such
 * launches of the process), "plain" = an ordinary launch sized by an occupancy query, one such launch at a time per process,
 * "auto" (default) = cooperative where the device supports it, plain if the runtime refuses the grid.  (Kernels of other
 * queues or processes can still keep a group from being resident together: arp_vi_run retakes a launch whose hand-offs timed
 * out -- arp_vi_attempts.)  Returns non-zero for an unknown key / value or a model the key does not apply to. */
int arp_model_set_option(arp_model* m, const char* key, const char* value);
/* Additive constant dropped from logp for parameterisation `which` (so callers can
 * report the reference-valued target_log_prob / ELBO): logp_ref = logp + const. */
double arp_model_logp_const(const arp_model* m, int which);

/* Set the parameterisation `which` (0 = primary, 1 = secondary, used by the
 * interleaved kernel): per-element VIP parameters a,b (HOST, [D]).  a=b=1 is CP,
 * a=b=0 is NCP (program_transformations.py:555-600). */
int arp_model_set_param(arp_model* m, int which, const float* a_host, const float* b_host);

/* target_log_prob_fn + its gradient for a batch of chains
 * (vectorize_log_joint_fn, inference.py:172-195 + tf.gradients inside TFP). */
int arp_logp_grad(arp_model* m, int which, const float* x, int n_chains,
                  float* logp, float* grad, int lanes_per_chain, void* stream);

/* State converters (models.py:56-128): dir 0: parameterisation `which` -> centred,
 * dir 1: centred -> parameterisation `which`. */
int arp_transform(arp_model* m, int which, int dir, const float* in, int n_chains,
                  float* out, void* stream);

/* Energy probe (build-specific): for every row of x [n_rows][D], a state in parameterisation `which`, draw a FRESH
 * momentum and integrate ONE leapfrog trajectory of `n_leapfrog` steps with per-element steps eps0[d] * kappa[row]
 * (kappa NULL: 1); out4 [n_rows][4] receives {logp at the start, kinetic energy at the start, logp at the end, kinetic
 * energy at the end} as computed -- NaN and +-inf are results, nothing is clamped.  x is not changed and no Metropolis
 * test is made.  What it is and is not: a fresh-momentum trajectory from the states handed in, NOT a replay of the
 * transition the sampler took from them; at stationarity state and fresh momentum are independent, so the energy errors
 * of probed trajectories have the distribution of the sampler's own next transitions.  The momentum of row r comes from a
 * stream keyed by (seed, row_offset + r): rows [0, n) at row_offset k equal rows [k, k + n) at offset 0.  p_out / q_out
 * (or NULL) [n_rows][D] receive the drawn momentum and the end state; p_out depends on the lanes per chain (every lane of
 * a chain draws from a stream of its own), so a replay on the host takes its momenta from p_out.  Asynchronous; all array
 * pointers are device pointers; the instantiation is chosen as arp_logp_grad chooses it.  Refused before any launch
 * (non-zero, arp_last_error): a NULL handle, x, eps0 or out4, `which` outside 0 / 1, n_rows < 1, n_leapfrog < 1. */
int arp_energy_probe(arp_model* m, int which, const float* x, int64_t n_rows, int n_leapfrog, const float* eps0,
                     const float* kappa, uint64_t seed, int64_t row_offset, float* out4, float* p_out, float* q_out,
                     int lanes_per_chain, void* stream);

/* Trajectory probe (build-specific): arp_energy_probe's trajectory with every intermediate step recorded.  For every row
 * of x [n_rows][D], a state in parameterisation `which`, draw a FRESH momentum and integrate ONE leapfrog trajectory of
 * `n_leapfrog_max` steps with per-element steps eps0[d] * kappa[row] (kappa NULL: 1).  energy_out
 * [n_leapfrog_max + 1][n_rows][2] receives {logp, kinetic energy} at the start (l = 0) and after every step l -- the
 * kinetic energy after the half kick that would close a trajectory of l steps, which goes into a temporary: the
 * trajectory itself runs on undisturbed -- as computed: NaN and +-inf are results.  path_out (or NULL)
 * [n_leapfrog_max][n_rows][D] receives the state after step l, centred (path_centred != 0) or in the coordinates of
 * parameterisation `which` (0); the flag does not change the integrator's arithmetic.  p_out (or NULL) [n_rows][D]
 * receives the drawn momentum: the stream of row r is keyed by (seed, row_offset + r) exactly as arp_energy_probe keys
 * it, so with equal seed, offset and lanes per chain p_out is that function's bit for bit, and rows [0, n) at row_offset
 * k equal rows [k, k + n) at offset 0.  x is not changed and no Metropolis test is made.
 * What the profile built from it (arp_jump_sums) is and is not: the trajectories start from fresh momenta, they are NOT
 * replays of the sampler's transitions; the step sizes are those the run adapted for its own leapfrog count, and a run at
 * another count would adapt others; the expected squared jump distance is a one-transition (lag-one) criterion, not an
 * effective sample size.
 * Asynchronous; all array pointers are device pointers; the instantiation is chosen as arp_logp_grad chooses it.
 * Refused before any launch (non-zero, arp_last_error): a NULL handle, x, eps0 or energy_out, `which` outside 0 / 1,
 * n_rows < 1 or too large for one launch (arp_energy_probe's limit), n_leapfrog_max < 1 or > 256. */
int arp_trajectory_probe(arp_model* m, int which, const float* x, int64_t n_rows, int n_leapfrog_max, const float* eps0,
                         const float* kappa, uint64_t seed, int64_t row_offset, float* energy_out, float* path_out,
                         int path_centred, float* p_out, int lanes_per_chain, void* stream);

/* Fold of a trajectory probe (needs no model handle): from the centred start states x0 [n_rows][D], the centred path
 * [n_leapfrog_max][n_rows][D] and the energies [n_leapfrog_max + 1][n_rows][2] of arp_trajectory_probe, sums
 * [n_leapfrog_max][5 + D] float64, per leapfrog count l: rows; divergent rows (energy error dH = (lp_0 - lp_l) +
 * (ke_l - ke_0), formed in float64, not finite or above 1000); rows whose dH is not finite; the sum of alpha = min(1,
 * exp(-dH)), a divergent row counting 0; left_out; then for every element d the sum over rows of alpha (x_l,d - x_0,d)^2.
 * A row with alpha = 0 is skipped; a term with alpha > 0 that is not finite is left out and counted in left_out.  All
 * sums are additive over rows, hence over calls and ranks.  One pass over `path`; differences, squares and alpha in
 * float64; fixed reduction order without atomics: two calls on the same input give bitwise equal sums.  The workspace
 * (arp_jump_workspace_bytes; 0: none needed, NULL is fine) is the caller's, 256-byte aligned.  Asynchronous; device
 * pointers.  Refused before any launch: a NULL x0, path, energy or sums, n_rows < 1 or above arp_energy_probe's limit,
 * D < 1, n_leapfrog_max < 1 or > 256, a workspace that is too small or misaligned. */
int64_t arp_jump_workspace_bytes(int64_t n_rows, int32_t D, int32_t n_leapfrog_max);
int arp_jump_sums(const float* x0, const float* path, const float* energy, int64_t n_rows, int32_t D,
                  int32_t n_leapfrog_max, double* sums, void* workspace, int64_t workspace_bytes, void* stream);

/* HMC segment (mcmc.HamiltonianMonteCarlo + step-size adaptation + sample_chain): `cfg->n_steps` transitions in ONE
 * launch.  (Internally a launch of 256 steps or more may hand its chains from workgroup to workgroup a few times -- DESIGN.md
 * section 3, relay segments --; chain state, counters and trace rows are bit for bit those of one workgroup per chain block.
 * The streaming statistics in io->stats are the exception: their partial-batch accumulators fold at every segment end, so
 * the sums are grouped differently and agree to float rounding only (~1e-6 relative), and the segment count follows the
 * device's CU count.  The call stays asynchronous; the hand-over waits are bounded, and a launch whose hand-over timed out
 * leaves the chains where they were and is reported by the next call on the handle or by arp_model_check.) */
int arp_hmc_run(arp_model* m, int which, const arp_hmc_config* cfg,
                const arp_hmc_io* io, void* stream);

/* Interleaved CP/NCP segment (interleaved.Interleaved.one_step, interleaved.py:113-155):
 * parameterisation 0 then 1 per step, each with its own leapfrog count, base
 * step sizes and adaptation state; `q` is kept in parameterisation-0 coordinates. */
typedef struct arp_interleaved_io {
  arp_hmc_io k0;             /* q/rng/trace live here; grad/logp are optional: kernels that carry the gradient across the
                                change of coordinates keep it there between calls (NULL: re-bootstrap at every call) */
  float* adapt1;             /* [C][4] adaptation state of kernel 1 */
  uint32_t* accept_count1;   /* [C] */
  const float* eps0_1;       /* [D] */
  uint8_t* trace_accept1;    /* [S][C] or NULL */
  uint32_t* rec_accept_count1; /* [C] in/out or NULL, as k0.rec_accept_count for kernel 1 */
} arp_interleaved_io;
int arp_interleaved_run(arp_model* m, const arp_hmc_config* cfg, int n_leapfrog_1,
                        const arp_interleaved_io* io, void* stream);

/* Mean-field VI (find_best_learning_rate, inference.py:26-154 on top of
 * util.get_mean_field_elbo, util.py:232-268): runs `n_lr` independent Adam
 * optimisations of `n_steps` steps in ONE launch (several when the learning rates do not all fit on the device at
 * once).  Every learning rate's `n_mc` draws are spread over a GROUP of workgroups that exchange their partial
 * gradient sums twice per step inside the launch and add them in a fixed order: a fit is bitwise reproducible, and
 * its draws do not depend on how the group is shaped.  The call is SYNCHRONOUS on `stream` when a group has more than
 * one workgroup (it waits for the launch to check that no in-launch hand-off timed out) and returns non-zero if one
 * did.  It keeps a hand-off workspace on the handle (freed by arp_model_destroy). */
typedef struct arp_vi_config {
  int32_t n_lr;              /* number of learning rates */
  int32_t n_steps;           /* num_optimization_steps */
  int32_t n_mc;              /* num_mc_samples (<= 4096) */
  int32_t learn_a;           /* 1: also optimise the VIP parameter a = sigmoid(w) (cVIP) */
  int32_t tied_b;            /* 1: b := a in the density (tied_pparams as intended); 0: b from set_param, or learned via io.wb */
  int32_t a_prior;           /* 0: none; 1: the reference's --discrete_prior on the learnable parameters (main.py:244-253):
                              * Mixture(logits (0,5,0); Laplace(0,0.1), Uniform(0,1), Laplace(1,0.1)), its log density
                              * added to the objective (inference.py:50-54) */
  uint64_t seed;
} arp_vi_config;
typedef struct arp_vi_io {
  const float* lr;           /* [n_lr] base learning rates */
  float* loc;                /* [n_lr][D] in: initial loc, out: final */
  float* rho;                /* [n_lr][D] in: initial pre-softplus scale, out: final */
  float* w;                  /* [n_lr][D] in/out unconstrained a (only if learn_a) */
  float* wb;                 /* [n_lr][D] in/out unconstrained b, learned separately (untied), or NULL */
  float* elbo;               /* [n_lr][n_steps] ELBO estimate per step (reference-valued, constants included) */
  float* prior;              /* [n_lr][n_steps] or NULL: log density of the a_prior on the learnable parameters at each step's
                              * values (the reference ranks learning rates on elbo + prior and reports elbo, inference.py:50-54,
                              * 120-150) */
  const int32_t* a_group;    /* [D] or NULL.  With untied parameters the reference gives `a` the shape of the variable's loc
                              * (program_transformations.py:486-493, 507-510): a vector variable whose loc is a scalar (german
                              * beta_log_scales, election a) learns ONE shared a.  a_group[d] = index of the first element of
                              * d's group (d itself when its a is its own); groups are contiguous.  DEVICE pointer, like every
                              * array here; arp_vi_run copies it back once and rejects a map that is not of that form */
  const int32_t* b_group;    /* the same for the separately learned b (shape of the variable's scale; only read with wb) */
} arp_vi_io;
int arp_vi_run(arp_model* m, int which, const arp_vi_config* cfg, const arp_vi_io* io, void* stream);
/* Measurement hook: the shape the calling thread's last arp_vi_run gave its launch -- out6 = {threads per workgroup,
 * sample groups G, row parts R (workgroups per learning rate = G x R), learning rates per launch, workgroups resident
 * together (= CUs in use when one fits per CU), workgroups of the kernel one CU holds}.  (bench.py: vi_kernel.) */
int arp_vi_geometry(int32_t* out6);
/* Measurement hook: how many launches the calling thread's last arp_vi_run needed for its slowest chunk of learning rates
 * (1 = every hand-off went through at once; a launch whose in-launch hand-offs ran into their bound -- the device was shared
 * for seconds -- is taken again from the parameters it started with, with 4 x the bound: 2 s, 8 s, 32 s, then an error). */
int arp_vi_attempts(int32_t* out1);

/* Deferred status of the handle's asynchronous launches: 0 if none failed; non-zero (and arp_last_error set) if a relay
 * hand-over inside an arp_hmc_run / arp_interleaved_run launch timed out since the last check -- the chains of that launch
 * were left partly advanced and must be discarded.  Reads a pinned host word: call it after synchronising the stream(s) the
 * launches went to.  Reports once (the word is cleared).  The same word is checked on entry to the next chain launch. */
int arp_model_check(arp_model* m);

/* Measurement hook: what the calling thread's last arp_hmc_run / arp_interleaved_run launch did -- out3 = {relay segments
 * the launch's steps were cut into (1 = one workgroup per chain block), chain blocks, workgroups of
 * the kernel one CU holds (0 where the question did not arise)}. */
int arp_relay_geometry(int32_t* out3);

/* The cut of a launch's n_steps into `segs` relay segments: lengths proportional to
 * (ratio_pct / 100)^s -- ratio_pct <= 0: the ratio the library itself cuts with -- that sum to n_steps, never increase and
 * are all >= 1; 100 is the equal cut.  Writes out[0 .. segs) (cap: the buffer's length) and returns segs, or 0 with
 * arp_last_error set (segs < 1, segs > n_steps, segs > cap, ratio_pct > 100).  A pure function: needs no device. */
int arp_relay_schedule(int n_steps, int segs, int ratio_pct, int32_t* out, int cap);

/* Effective sample size of every series of a recorded trace (replaces tfp.mcmc.effective_sample_size with its
 * defaults, inference.py:240, 327): `trace` holds n_samples rows of `row_stride` floats, series i is column i
 * (i < n_series, e.g. n_series = C*D of a [S][C][D] trace); ess[i] = S / (-1 + 2 sum_k (S-k)/S rho_k) with the
 * auto-correlations cut at the first negative one.  A constant series gives NaN (0/0), as the reference's does. */
int arp_ess(const float* trace, int64_t n_samples, int64_t n_series, int64_t row_stride, float* ess, void* stream);

/* The same statistic with a caller-owned device workspace for LONG traces (the [S = 50 000][k D] trace of a streaming
 * run's kept chains, inference.py:238-240 at main.py:101-110's default schedule): series that are still positively
 * correlated after the coalesced sweeps (48 lags) are copied series-major into the workspace and finished on the matrix
 * cores (csrc/ess_tail.h), instead of per-lane sweeps that re-read the trace 16 lags at a time (arp_ess: 5.5 s on the
 * german-credit trace, this: see profiles/).  arp_ess_workspace_bytes is the size at which every series fits at once
 * (0 when n_samples is short enough for the one-kernel path); a smaller workspace works (the listed series are taken in
 * chunks) as long as the work lists (28 bytes per series) and 64 series rows fit.  256-byte aligned. */
int64_t arp_ess_workspace_bytes(int64_t n_samples, int64_t n_series);
int arp_ess_ws(const float* trace, int64_t n_samples, int64_t n_series, int64_t row_stride, float* ess,
               void* workspace, int64_t workspace_bytes, void* stream);

/* Convergence diagnostics across chains (build-specific: the reference reports the within-chain ESS only).
 *
 * First and second moments of every series of a recorded trace, whole or per half.  Same trace addressing as arp_ess:
 * n_samples rows of row_stride floats, series i is column i (i < n_series).  split = 0: one part, all rows.
 * split = 1: two parts of h = n_samples / 2 rows each, rows [0, h) and [n_samples - h, n_samples) (an odd run drops its
 * middle row, as Stan / ArviZ do).  mean, var: [P][n_series] (P = 1 + split), var with the n - 1 divisor.  A part of one
 * row has var = NaN (an empty part, n_samples = 1 with split = 1, mean = NaN as well), a constant part var = 0 exactly.
 * Never fails on a short trace.  Shifted sums per chunk of 256 rows, chunks merged pairwise in a fixed order: a result
 * is bitwise reproducible and the same for a column however it is reached (alignment, grid, route).
 * arp_moments_workspace_bytes is 0 where one launch over the series axis fills the device; otherwise (few series, many
 * rows) it is the size of the per-chunk partials with which the row axis is cut over workgroups too and a second launch
 * merges them.  Without such a workspace (NULL, or fewer bytes) the one-launch form is taken.  256-byte aligned. */
int64_t arp_moments_workspace_bytes(int64_t n_samples, int64_t n_series, int split);
int arp_split_moments(const float* trace, int64_t n_samples, int64_t n_series, int64_t row_stride, int split,
                      float* mean, float* var, void* workspace, int64_t workspace_bytes, void* stream);

/* Column sums over `n_rows` rows of [n_rows][D] float32 moments (rows = chains, or half-chains: the [P][C][D] planes of
 * arp_split_moments are [(P C)][D] rows).  Over the rows whose var is finite: sums[0][d] = their number, sums[1][d] =
 * sum of mean, sums[2][d] = sum of mean^2, sums[3][d] = sum of var; sums[4][d] = number of rows with var == 0 (series that
 * never moved).  float64 accumulation in a fixed order (bitwise reproducible); sums is a DEVICE [5][D] double buffer.
 * The five vectors are additive over chains, hence over ranks.  n_rows = 0 gives zeros. */
int arp_moments_fold(const float* mean, const float* var, int64_t n_rows, int32_t D, double* sums, void* stream);

/* Rank normalisation (build-specific; what the rank-normalised, folded split R-hat of Vehtari et al. 2021 needs: the
 * result is a z-score trace that arp_split_moments / arp_moments_fold take unchanged) and order statistics of the pooled
 * draws.  Trace addressing as arp_split_moments with n_series = n_chains * D: draw s of chain c, element d is
 * trace[s * row_stride + c * D + d], row_stride >= n_chains * D.  The pool of element d is its N = n_samples * n_chains
 * values x_(1) <= ... <= x_(N); N < 2^31.
 *   median[d]       0.5f * (x_(floor((N+1)/2)) + x_(ceil((N+1)/2))), formed in float32                     [D], may be NULL
 *   quantiles[q][d] x_(k), k = clamp(ceil(probs[q] * N), 1, N) in float64 (the inverted-CDF definition: an order
 *                   statistic, no interpolation); probs is a HOST array of n_probs values       [n_probs][D], may be NULL
 *   values ranked   v = x (fold = 0) or v = fabsf(x - median[d]) in float32 (fold = 1)
 *   rank2           #{v' < v} + #{v' <= v} over the pool = 2 * (average 1-based rank) - 1; ties share it, -0 ties with
 *                   +0, subnormals are distinct, +-inf order as numbers                     uint32 [S][C][D], may be NULL
 *   z               Phi^-1((4 rank2 + 1) / (8 N + 2)) = Phi^-1((r - 3/8) / (N + 1/4)), formed from the integers in
 *                   float64 and from the nearer tail, rounded to float32                         [S][C][D], required
 * Every output is a function of the sorted pool alone: bitwise reproducible whatever the grid.  A NaN neither faults nor
 * hangs; the results of an element that holds one are unspecified.  The workspace (arp_rank_workspace_bytes: two key
 * buffers of the trace's size and the radix sort's counts; the same for both values of fold) is required and 256-byte
 * aligned; returns 1 (arp_last_error) on a missing argument, a workspace too small or misaligned, or N >= 2^31. */
int64_t arp_rank_workspace_bytes(int64_t n_samples, int64_t n_chains, int32_t D, int fold);
int arp_rank_normalize(const float* trace, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                       int fold, float* z, uint32_t* rank2, float* median,
                       const double* probs, int32_t n_probs, float* quantiles,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* Multi-chain effective sample size of every element (build-specific; the estimator of Vehtari et al. 2021 behind
 * bulk-ESS, tail-ESS and the Monte-Carlo standard error of the mean, as Stan / posterior / ArviZ report them next to the
 * rank-normalised R-hat).  Trace addressing as arp_rank_normalize.  Rows: split = 1 gives m = 2 n_chains rows of
 * n = n_samples / 2 draws, [0, n) and [n_samples - n, n_samples) of every chain (an odd run drops its middle draw, as
 * arp_split_moments does); split = 0 gives m = n_chains rows of n = n_samples.  With threshold, the value of a draw is
 * 1.0f where x <= threshold[d] and 0.0f otherwise (a NaN is 0); no indicator trace is written.  Per element, in float64:
 *   gamma_j(k) = (1/n) sum_{t < n-k} (x_t - mu_j)(x_{t+k} - mu_j) about row j's own mean,  Gamma(k) = mean_j gamma_j(k)
 *   mean_var = Gamma(0) n / (n - 1),  var_plus = Gamma(0) + [m > 1] (sample variance of the mu_j, divisor m - 1)
 *   rho(k) = 1 - (mean_var - Gamma(k)) / var_plus
 *   Geyer's initial positive sequence: t = 0, E = 1, O = rho(1), r[0] = E, r[1] = O; while t < n - 5 and E + O > 0:
 *     t += 2, E = rho(t), O = rho(t + 1), and r[t] = E, r[t+1] = O where E + O >= 0; then max_t = t and r[max_t] = E where
 *     E > 0; every other r is 0.  Initial monotone sequence: for t = 2, 4, ... <= max_t - 2, a pair r[t] + r[t+1] above
 *     the pair before it is replaced by that pair's mean, twice.
 *   tau = max(-1 + 2 sum_{k < max_t} r[k] + r[max_t], 1 / log10(n m)),  ess[d] = n m / tau                 [D], required
 *   max_t[d]     as above; 0 where ess is NaN                                                       [D], may be NULL
 *   rho[k][d]    rho(k) before the monotone step for k <= min(max_t + 1, n_rho - 1), NaN beyond  [n_rho][D], may be NULL
 * ess[d] is NaN where var_plus is not > 0 (an element that never moved) or n < 4; neither is an error.  The lagged
 * products are float32 in windows of 128, every window added into float64, about means summed in float64: rho is good to
 * 128 x 2^-24 of 1 at worst.  Every sum has a fixed order that depends on the shape alone: a result is bitwise
 * reproducible, and the same for a block of chains taken in place (row_stride > n_chains * D) as for its contiguous
 * copy.  A NaN or inf neither faults nor hangs; the results of an element that holds one are unspecified, the others'
 * are not touched.  Lags are taken 16 at a time, for the elements the pooled sequence has not cut yet; every launch the
 * longest cut could need is enqueued and the call never synchronises.  The workspace (arp_ess_multichain_workspace_bytes:
 * the rows' means and one partial sum per workgroup, element and lag) is required and 256-byte aligned; returns 1
 * (arp_last_error) on a missing argument, a workspace too small or misaligned, n_samples * n_chains >= 2^31, or more
 * than 2^20 draws per row (the launches enqueued grow with n / 16: at most 2^17). */
int64_t arp_ess_multichain_workspace_bytes(int64_t n_samples, int64_t n_chains, int32_t D, int split);
int arp_ess_multichain(const float* trace, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                       int split, const float* threshold, float* ess, int32_t* max_t,
                       float* rho, int32_t n_rho, void* workspace, int64_t workspace_bytes, void* stream);

/* Nested R-hat over superchains (build-specific; Margossian et al. 2024: the convergence diagnostic for many short chains).
 * The n_rows = K M chains form K superchains of M = `group` chains that are adjacent on the chain axis (superchain k owns
 * rows k M ... k M + M - 1) and started from one point.  mean, var: [n_rows][D] float32 per-chain moments as for
 * arp_moments_fold; var may be NULL (one draw per chain: every within-chain variance is 0 and only the means are tested).
 * A superchain counts where all M of its rows have a finite mean and a finite var in column d; any other is left out
 * whole.  With g_k = mean over its rows of mean, b_k = sum (mean - g_k)^2 / (M - 1) -- from deviations about a row of the
 * group, never a difference of raw squares -- and w_k = mean over its rows of var, over the superchains that count:
 *   sums[0][d] = their number, sums[1][d] = sum g_k, sums[2][d] = sum g_k^2, sums[3][d] = sum b_k, sums[4][d] = sum w_k,
 *   sums[5][d] = the number of superchains left out.
 * float64 accumulation in a fixed order (bitwise reproducible, no atomics); sums is a DEVICE [6][D] double buffer.  The six
 * vectors are additive over superchains, hence over ranks that hold whole superchains; the host takes
 * B = (sums[2] - sums[1]^2 / K) / (K - 1) in float64, good to ~ 2^-52 K gbar^2 / ((K - 1) B) of itself.  Any M from 2 to
 * n_rows, any D >= 1; n_rows = 0 gives zeros.  One workgroup, no workspace.  Returns 1 (arp_last_error) on a missing
 * argument, group < 2 or n_rows not a multiple of group. */
int arp_moments_fold_nested(const float* mean, const float* var, int64_t n_rows, int32_t D, int64_t group,
                            double* sums, void* stream);

/* The same sums with ONE draw per chain, for every row of a recorded trace: the profile of nested R-hat over the sampling
 * phase.  Trace addressing as arp_rank_normalize (draw s of chain c, element d is trace[s * row_stride + c * D + d],
 * row_stride >= n_chains * D: a block of chains of a wider trace is read in place); n_chains = K group.  With g and b
 * taken over the M draws of a superchain in row s, over the superchains whose M draws of (s, d) are all finite:
 *   sums[0][s][d] = their number, sums[1][s][d] = sum g, sums[2][s][d] = sum g^2, sums[3][s][d] = sum b.
 * sums is a DEVICE [4][n_samples][D] double buffer.  One pass over the trace, lanes along a superchain's contiguous
 * M * D floats; float64 deviations from a draw of the group, partial (count, mean, M2) merged in a fixed order, no
 * atomics: bitwise reproducible, and the same for a block of chains taken in place as for its contiguous copy.
 * arp_nested_step_workspace_bytes is 0 where one workgroup per row fills the device; otherwise it is the size of the
 * per-workgroup partial sums a second launch adds up, and the workspace is required and 256-byte aligned.  Returns 1
 * (arp_last_error) on a missing argument, group < 2, n_chains not a multiple of group, a workspace too small or
 * misaligned, or a shape arp_rank_normalize would refuse. */
int64_t arp_nested_step_workspace_bytes(int64_t n_samples, int64_t n_chains, int32_t D, int64_t group);
int arp_nested_step_sums(const float* trace, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                         int64_t group, double* sums, void* workspace, int64_t workspace_bytes, void* stream);

/* Cross moments of a trace on the matrix cores (build-specific; csrc/gram.hip): what the posterior geometry report takes a
 * covariance from.  Addressing as arp_rank_normalize: element d of draw s of chain c is x[s * row_stride + c * D + d],
 * row_stride >= n_chains * D (a block of chains of a wider trace is read in place; a plain [n][D] matrix is n_samples = n,
 * n_chains = 1); nothing past x[(n_samples - 1) * row_stride + n_chains * D - 1] is read.  shift: a device [D] array, NULL
 * for zeros (bitwise the result of explicit zeros).  For every row r, u_r = x_r - shift in float32 with one rounding; a row
 * with a non-finite element (of x, hence of u) is left out whole and counted.  sums is a DEVICE double [D + 2][D]:
 *   rows 0 ... D - 1: G[i][j] = sum_r u_ri u_rj over the rows that count -- the full matrix, the lower triangle a bitwise
 *                     mirror of the upper;
 *   row D:            sum_r u_rd;
 *   row D + 1:        [0] = rows that counted, [1] = rows left out (D = 1 has no room for it: n_samples * n_chains - [0]),
 *                     the rest 0.
 * All of it is additive over rows, hence over calls and ranks that use one shift.  The products and their accumulation
 * run on v_mfma_f32_32x32x2_f32 (exact f32, bit for bit a k-ordered fmaf chain; k is the row axis), upper-triangle blocks
 * only, an accumulator over a window of at most 256 rows (kGramWindow) that is then added into float64:
 *   |G_dev - G_f64|[i][j] <= (kGramWindow + 1) * 2^-24 * sum_r |u_ri u_rj|
 * where G_f64 is the float64 sum of the float32 u; row D is exact to float64 rounding and the counts are exact.
 * Select rule: padding columns, missing rows and rows left out enter the MFMA as 0 by select, never by a multiplication
 * (0 * inf is NaN), and a row's mask is complete before any of its blocks is multiplied.
 * Reproducibility rule: the workgroups' float64 partials are merged by a second launch in an order that depends on
 * (n_samples * n_chains, D) alone -- no atomics; two calls give bitwise equal sums, and a block of chains taken in place
 * gives bitwise the sums of its contiguous copy, at any alignment and stride.
 * 1 <= D <= 512.  The workspace (arp_gram_workspace_bytes: the partials; 0 for a shape that is refused) is always needed
 * and 256-byte aligned.  Returns 1 (arp_last_error) before any launch on a NULL x or sums, D < 1 or D > 512,
 * n_samples < 1 or n_chains < 1, n_samples * n_chains >= 2^31, row_stride < n_chains * D, or a workspace that is missing,
 * too small or misaligned. */
int64_t arp_gram_workspace_bytes(int64_t n_samples, int64_t n_chains, int32_t D);
int arp_gram_sums(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                  const float* shift, double* sums, void* workspace, int64_t workspace_bytes, void* stream);

/* Pointwise log-likelihood of recorded draws (csrc/loglik.hip; needs no model handle): for a block of recorded steps of
 * the CENTRED trace x [n_samples][n_chains][D] (rows `row_stride` floats apart, read in place, as arp_gram_sums reads it)
 * and the observations [n0, n1) of an observation table in device memory,
 *   eta_n = sum_t w[n * T + t] * x[idx[n * T + t]],   s_n = log_scale[n] + (scale_idx[n] >= 0 ? x[scale_idx[n]] : 0)
 *   kind ARP_OBS_NORMAL:     ll = -0.5 * ((y[n] - eta_n) * exp(-s_n))^2 - s_n - 0.5 * log(2 pi)
 *   kind ARP_OBS_BERNOULLI:  ll = y[n] * eta_n - (max(eta_n, 0) + log1p(exp(-|eta_n|)))
 * it writes ll[(n - n0) * ll_stride + r] for draw r = step * n_chains + chain, mask[r] = 1 for a draw with a non-finite
 * element among its D (0 otherwise; [n_samples * n_chains] bytes) and their count into *n_masked (device memory).  The ll
 * entries of a masked draw are written as 0 by select and are not to be read.  float32, contraction off, the T terms in
 * their order: with u = 2^-24, A = sum_t |w_t x_t|, z = (y - eta) exp(-s), to first order
 *   |eta_dev - eta| <= T u A
 *   Normal:     |ll_dev - ll| <= u (T A exp(-s) |z| + z^2 (5 + |s|) + 3 |s| + |ll|)
 *   Bernoulli:  |ll_dev - ll| <= u (T A (|y| + 1) + |y eta| + 3 + softplus(eta) + |ll|)
 * Nothing is read past the last element of the trace block; idx and scale_idx are clamped into [0, D).  Asynchronous.
 * Refused before any launch: a NULL pointer, D < 1 or D > 255, a trace shape the other diagnostics refuse,
 * row_stride < n_chains * D, an unknown kind, T < 1 or T > 4096, n0 < 0 or n1 <= n0, ll_stride < n_samples * n_chains. */
enum { ARP_OBS_NORMAL = 0, ARP_OBS_BERNOULLI = 1 };
int arp_pointwise_loglik(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                         int32_t kind, const int32_t* idx, const float* w, int32_t T, const float* y,
                         const int32_t* scale_idx, const float* log_scale, int64_t n0, int64_t n1, float* ll,
                         int64_t ll_stride, uint8_t* mask, int64_t* n_masked, void* stream);

/* PSIS-LOO and WAIC per observation (csrc/psis.hip; Vehtari, Gelman, Gabry 2017; Vehtari et al. 2024): from
 * ll [n_obs][n_draws] (rows ll_stride floats apart) over the draws with mask[r] == 0 (mask NULL: all of them),
 *   out[n][8] = {elpd_loo, pareto_k, lppd, p_waic, tail_len, cutoff, gpd_sigma, draws_used}      (float64)
 * One workgroup per observation; everything after the float32 load is float64.  The tail is the
 * M = min(floor(R' / 5), m), m^2 >= 9 R', largest log ratios -ll of the R' kept draws, found exactly by a radix select
 * (ties across the cut-off are handled by count); M < 5, or a fit that is not finite, gives pareto_k = +inf and raw
 * weights; a non-finite ll among the kept draws gives pareto_k = +inf and elpd_loo = -inf (NaN for a NaN).  No float
 * atomics, fixed reduction orders: two calls give bitwise equal results.  tail_len, cutoff and draws_used are exact;
 * |lppd - ref| <= (R' + 32) 2^-53 + 4 2^-53 max|ll|,  |p_waic - ref| <= (R' + 8) 2^-52 p_waic + R' (2^-52 max|ll|)^2.
 * The workspace (arp_psis_workspace_bytes; 0 for a shape that is refused) is the caller's, 256-byte aligned.
 * Asynchronous; device pointers.  Refused before any launch: a NULL ll or out, n_obs < 1, n_draws < 1 or above 2^24,
 * ll_stride < n_draws, a workspace that is missing, too small or misaligned. */
int64_t arp_psis_workspace_bytes(int64_t n_obs, int64_t n_draws);
int arp_psis_loo(const float* ll, int64_t n_obs, int64_t n_draws, int64_t ll_stride, const uint8_t* mask, double* out,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* arp_psis_loo, and the Pareto-smoothed log weight of every draw with it (csrc/psis.hip; the second launch is
 * csrc/psis_weights.hip): ll, mask and out are arp_psis_loo's and out[n][8] is that function's on the same input BIT FOR
 * BIT (the same kernel, launched the same way).
 * lw [n_obs][lw_stride] double receives the max-shifted, smoothed log weights as tests/psis_ref.py: psis_row forms `lws`:
 * a draw outside the tail takes its raw weight llmin - ll (llmin: the smallest kept ll of the row); the draw at position
 * i < M of the ascending-ll order -- ties in ascending draw index, a stable sort -- takes the (M - 1 - i)-th smallest
 * smoothed tail weight, truncated at 0; a row that is not fitted (M < 5, or a fit that is not finite) keeps raw weights
 * throughout; a masked draw takes -inf; every kept draw of a row with a non-finite kept ll takes NaN.  Raw positions are
 * exact (one float64 subtraction of two float32 values); smoothed ones carry the error of the fit (csrc/psis.hip).  The
 * tail's members find their rank by counting among themselves (at most 12 288), integers only; no float atomics: two
 * calls give bitwise equal out and lw.  The workspace (arp_psis_weights_workspace_bytes: arp_psis_loo's and one 64-bit
 * word per tail member; 0 for a shape that is refused) is the caller's, 256-byte aligned.  Asynchronous; device pointers.
 * Refused before any launch: what arp_psis_loo refuses, a NULL lw, lw_stride < n_draws. */
int64_t arp_psis_weights_workspace_bytes(int64_t n_obs, int64_t n_draws);
int arp_psis_weights(const float* ll, int64_t n_obs, int64_t n_draws, int64_t ll_stride, const uint8_t* mask, double* out,
                     double* lw, int64_t lw_stride, void* workspace, int64_t workspace_bytes, void* stream);

/* Posterior predictive check (csrc/ppc.hip; Gelman, Meng, Stern 1996; BDA3 ch. 6): replicated observations of recorded
 * draws, folded on the device.  The trace x, the table and the observation range [n0, n1) are those of
 * arp_pointwise_loglik (same addressing, same row_stride rule, 1 <= D <= 255, 1 <= T <= 4096), and eta_n, s_n are its
 * float32 chain, operation for operation.  For observation n (its GLOBAL index in the table) and draw
 * r = step * n_chains + chain, with mu and var the mean and the variance of y_rep given the draw:
 *   kind ARP_OBS_NORMAL:     mu = eta, var = exp(s)^2;  y_rep = eta + exp(s) * z;  z_obs = (y - eta) * exp(-s);
 *                            pit = Phi(z_obs) = 0.5 * erfc(-z_obs / sqrt 2);  dev(v) = ((v - eta) * exp(-s))^2 + 2 s + log(2 pi)
 *   kind ARP_OBS_BERNOULLI:  p = sigmoid(eta) = (eta >= 0 ? 1 : e) / (1 + e), e = exp(-|eta|);  mu = p, var = p * (1 - p);
 *                            y_rep = (u < p) ? 1 : 0;  pit = P(y_rep < y) + P(y_rep = y) / 2 (y > 0.5: 1 - p / 2; else (1 - p) / 2);
 *                            dev(v) = -2 * (v * eta - (max(eta, 0) + log1p(e)))
 * dev is -2 log-likelihood.  Random numbers: ONE call philox4x32_10(counter = (n, lo32(g), hi32(g), 0), key = (lo32(seed),
 * hi32(seed))) per (n, r), g = draw_offset + r; words 0 and 1 are used.  Bernoulli: u = (w0 >> 8) * 2^-24 in [0, 1).
 * Normal: z = sqrt(-2 log(u')) * cospi(2 a), u' = fma((float)w0, 2^-32, 2^-33) in (0, 1], a = the float in [1, 2) whose
 * mantissa is the low 23 bits of w1 (the sampler's normal_pair, through logf, sqrtf, cospif).  A result therefore never
 * depends on the tiling, on [n0, n1) or on which rank holds a draw.  Outputs (device memory):
 *   draw_stats [n_samples * n_chains][8] double, per draw over the observations of this call:
 *     {sum y_rep, sum y_rep^2, min y_rep, max y_rep, sum dev(y_rep), sum dev(y), sum mu, observations counted};
 *     two observation ranges combine by +, +, min, max, +, +, +, +.
 *   obs_sums [n1 - n0][4] double, per observation over the draws not left out:
 *     {sum mu, sum (mu^2 + var), sum pit, #{y_rep <= y}}.
 *   y_rep: NULL, or float [n1 - n0][y_rep_stride], y_rep[(n - n0) * y_rep_stride + r]; NULL leaves every other output
 *     bitwise as it is.
 *   mask [n_samples * n_chains] bytes and *n_masked as arp_pointwise_loglik's: a draw with a non-finite element is left
 *     out; its draw_stats row and its y_rep entries are written as 0 by select and it enters no obs_sums.
 * The per-(n, r) values are float32; every sum is accumulated in float64 in a fixed order, no float atomics: two calls give
 * bitwise equal outputs.  Error bounds of the per-(n, r) values: the header of csrc/ppc.hip.
 * The workspace (arp_predictive_workspace_bytes(n1 - n0, n_samples * n_chains): the per-tile partial sums of obs_sums,
 * (n_draws / 64) * n_obs * 32 bytes, and the per-group partials of draw_stats; <= 0 for a shape that is refused) is the
 * caller's, 256-byte aligned.  Asynchronous.  Refused before any launch: what arp_pointwise_loglik refuses (a NULL
 * pointer other than y_rep, D, the trace shape, row_stride, kind, T, n0 and n1; y_rep_stride < n_samples * n_chains with
 * a y_rep), a workspace that is missing, too small or misaligned. */
int64_t arp_predictive_workspace_bytes(int64_t n_obs, int64_t n_draws);
int arp_predictive_check(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride, int32_t kind,
                         const int32_t* idx, const float* w, int32_t T, const float* y, const int32_t* scale_idx,
                         const float* log_scale, int64_t n0, int64_t n1, uint64_t seed, int64_t draw_offset,
                         double* draw_stats, double* obs_sums, float* y_rep, int64_t y_rep_stride, uint8_t* mask,
                         int64_t* n_masked, void* workspace, int64_t workspace_bytes, void* stream);

/* Grouped predictive check (csrc/ppc_group.hip; Marshall, Spiegelhalter 2007): the replicated observations of
 * arp_predictive_check folded per GROUP of observations and draw.  The trace x and the table are arp_predictive_check's,
 * the table whole: n_obs is its length.  order [n_grouped] holds the indices (in the whole table) of the grouped
 * observations sorted by group, ascending within a group; group g of n_groups is order[group_start[g]] ...
 * order[group_start[g + 1] - 1], group_start [n_groups + 1] ascending from 0 to n_grouped; an observation may belong to no
 * group.  The call covers the groups [g0, g1).  y_rep of (n, r) is bit for bit arp_predictive_check's under the same seed
 * and draw_offset: the same Philox counter (n of the whole table, draw_offset + r) and the same float32 operations in the
 * same order (csrc/ppc_terms.h).  Output (device memory):
 *   group_stats [g1 - g0][n_samples * n_chains][8] double: draw_stats' eight columns over the observations of one group,
 *     {sum y_rep, sum y_rep^2, min y_rep, max y_rep, sum dev(y_rep), sum dev(y), sum mu, observations counted}, the sums
 *     in float64 in order's sequence, min and max of the float32 values.  An empty group: (0, 0, +inf, -inf, 0, 0, 0, 0).
 *     A draw that is left out: a zero row in every group, by select.
 *   mask and *n_masked as arp_predictive_check's.
 * No float atomics and one fixed chain of additions per (group, draw): a row does not depend on the tiling, on [g0, g1)
 * or on how many draws a call holds; two calls give bitwise equal outputs.  An order entry is clamped into [0, n_obs) and
 * a group_start entry into [0, n_grouped] before use.  No workspace.  Asynchronous.  Refused before any launch: what
 * arp_predictive_check refuses of the trace and the table (a NULL pointer, D, the trace shape, row_stride, kind, T), n_obs
 * outside [1, 2^31), n_grouped outside [0, 2^31), a NULL order with n_grouped > 0, n_groups < 1, 0 <= g0 < g1 <= n_groups
 * violated, draw_offset < 0. */
int arp_group_predictive_check(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                               int32_t kind, const int32_t* idx, const float* w, int32_t T, const float* y,
                               const int32_t* scale_idx, const float* log_scale, int64_t n_obs, const int32_t* order,
                               int64_t n_grouped, const int32_t* group_start, int64_t n_groups, int64_t g0, int64_t g1,
                               uint64_t seed, int64_t draw_offset, double* group_stats, uint8_t* mask, int64_t* n_masked,
                               void* stream);

/* Group log-likelihood (csrc/logo.hip; PSIS leave-one-group-out: Vehtari, Gelman, Gabry 2017; Merkle, Furr, Rabe-Hesketh
 * 2019): per group of observations and draw, the joint log-likelihood of the group at the recorded state (CONDITIONAL) and,
 * Normal data, with the group's own latent element integrated against its conditional prior (MARGINAL).  The trace x, the
 * table (whole: n_obs its length), order, n_grouped, group_start, n_groups and [g0, g1) are arp_group_predictive_check's.
 * slope [n_grouped] float runs parallel to order: the sum of the weights with which observation order[j] reads its
 * group's element; elem [n_groups]: that element's index in the state, clamped into [0, D) before use.  The site table --
 * site_loc_idx, site_scale_idx [D][ARP_SITE_TERMS] int32, site_loc_w, site_scale_w [D][ARP_SITE_TERMS] and site_loc0,
 * site_log_scale0 [D] float -- is arp_site_logprior's; only the rows elem names are read, as the float32 chains
 * loc = loc0 + sum_t loc_w x[loc_idx], sj = log_scale0 + sum_t scale_w x[scale_idx] of that kernel.
 * Per (n, r) the float32 value ll is arp_pointwise_loglik's, operation for operation; Normal data also b = slope *
 * exp(-s_n) and the float32 products b * z, b * b (z = (y_n - eta_n) * exp(-s_n)).  Per (group, draw), float64, in order's
 * sequence: S_ll = sum ll, S_bz = sum b z, S_bb = sum b b.  Outputs (device memory, either may be NULL, not both):
 *   lc [g1 - g0][out_stride] float, lc[(g - g0) * out_stride + r] = (float)S_ll: the float64 sum, in order's sequence, of
 *     the values arp_pointwise_loglik writes for the group's observations, rounded once.
 *   lm, same layout, kind ARP_OBS_NORMAL only.  With t0 = x[elem[g]], tau = exp(-2 sj), m = t0 - loc, P = S_bb + tau,
 *     q = S_bz - m * tau, all float64:  lm = (float)(S_ll - 0.5 * (m * m * tau - q * q / P) - 0.5 * log1p(S_bb / tau))
 *     = log of the integral over t of prod_n p(y_n | eta_n + slope_n (t - t0), s_n) * N(t | loc, exp(sj)) -- exact when
 *     nothing but the group's linear predictors reads the element.  A tau of 0, inf or NaN gives a non-finite lm, written
 *     as it comes.  lm == NULL: nothing is computed for it and lc is bitwise unchanged.
 *   An empty group writes 0 in both; a draw that is left out writes 0 in both, by select.
 *   mask and *n_masked as arp_pointwise_loglik's.
 * No float atomics and one fixed chain of additions per (group, draw): a row does not depend on the tiling, on [g0, g1) or
 * on how many draws a call holds; two calls give bitwise equal outputs.  Error bound of lm: the header of csrc/logo.hip.
 * No workspace.  Asynchronous.  Refused before any launch: what arp_group_predictive_check refuses of the trace, the
 * table and the groups; a NULL slope or elem; both outputs NULL; a NULL site pointer with lm; lm with kind
 * ARP_OBS_BERNOULLI; out_stride < n_samples * n_chains. */
int arp_group_loglik(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride, int32_t kind,
                     const int32_t* idx, const float* w, int32_t T, const float* y, const int32_t* scale_idx,
                     const float* log_scale, int64_t n_obs, const int32_t* order, const float* slope, int64_t n_grouped,
                     const int32_t* group_start, const int32_t* elem, int64_t n_groups, int64_t g0, int64_t g1,
                     const int32_t* site_loc_idx, const float* site_loc_w, const float* site_loc0,
                     const int32_t* site_scale_idx, const float* site_scale_w, const float* site_log_scale0, float* lc,
                     float* lm, int64_t out_stride, uint8_t* mask, int64_t* n_masked, void* stream);

/* Leave-one-out predictive sums (csrc/loopred.hip; Vehtari, Gelman, Gabry 2017 section 2; loo::E_loo, loo::loo_pit): the
 * per-(observation, draw) predictive quantities of arp_predictive_check folded over the draws with importance weights.
 * The trace x, the table and the observation range [n0, n1) are those of arp_pointwise_loglik (same addressing, same
 * row_stride rule, 1 <= D <= 255, 1 <= T <= 4096); eta_n, s_n are its float32 chain and mu, var, pit are
 * arp_predictive_check's definitions, operation for operation, through the same device-library functions:
 *   kind ARP_OBS_NORMAL:     mu = eta, var = exp(s)^2, pit = 0.5 * erfc(-(y - eta) * exp(-s) / sqrt 2)
 *   kind ARP_OBS_BERNOULLI:  mu = p = sigmoid(eta), var = p * (1 - p), pit = the mid-p value (y > 0.5: 1 - p / 2; else (1 - p) / 2)
 * lw[(n - n0) * lw_stride + r] (double, device memory) is the log weight of draw r = step * n_chains + chain for
 * observation n, as arp_psis_weights writes it; where it came from does not matter.  With W = exp(lw), one float64 exp:
 *   obs_sums [n1 - n0][6] double = {sum W, sum W^2, sum W * mu, sum W * (mu^2 + var), sum W * pit, draws counted}
 * over the draws with lw != -inf.  A draw with lw = -inf enters nothing, by select (its state may be non-finite); a NaN
 * lw enters, is counted and carries through to the observation's five float columns; the count is exact.  The per-(n, r)
 * values are float32 with the first-order bounds of csrc/ppc.hip's header (restated in csrc/loopred.hip); the products
 * with W and every sum are float64 in a fixed order (an xor butterfly over a tile of 64 draws, then the tiles in ascending
 * order), no float atomics: two calls give bitwise equal output, and the row of observation n does not depend on
 * [n0, n1).  Nothing is read past the last element of the trace block or of lw's rows; idx and scale_idx are clamped
 * into [0, D).  The workspace (arp_loo_predictive_workspace_bytes(n1 - n0, n_samples * n_chains): the per-tile partial
 * sums, ceil(n_draws / 64) * n_obs * 48 bytes; <= 0 for a shape that is refused) is the caller's, 256-byte aligned.
 * Asynchronous.  Refused before any launch: what arp_pointwise_loglik refuses (a NULL x or table pointer, D, the trace
 * shape, row_stride, kind, T, n0 and n1), a NULL lw or obs_sums, lw_stride < n_samples * n_chains, a workspace that is
 * missing, too small or misaligned. */
int64_t arp_loo_predictive_workspace_bytes(int64_t n_obs, int64_t n_draws);
int arp_loo_predictive(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride, int32_t kind,
                       const int32_t* idx, const float* w, int32_t T, const float* y, const int32_t* scale_idx,
                       const float* log_scale, int64_t n0, int64_t n1, const double* lw, int64_t lw_stride,
                       double* obs_sums, void* workspace, int64_t workspace_bytes, void* stream);

/* Power-scaling sensitivity (csrc/psens.hip; Kallioinen, Paananen, Buerkner, Vehtari 2023; priorsense, ArviZ psens): the
 * three device pieces below the smoothed weights of arp_psis_weights.  Device pointers; asynchronous; everything is
 * refused before any launch with 1 (arp_last_error).
 *
 * arp_loglik_total: the log-likelihood of every draw from a tile of pointwise values.  For every draw r:
 *   acc = total[r];  for n = 0 ... n_obs - 1: acc += (double)ll[n * ll_stride + r];  total[r] = acc
 * strictly sequential in n, so walking the observations in several tiles (ascending, into the same total) gives bitwise
 * the result of one call; exact against float64 sequential addition.  A masked draw is the caller's business
 * (arp_pointwise_loglik writes 0 there).  Refused: a NULL pointer, n_obs < 1, n_draws < 1 or >= 2^31,
 * ll_stride < n_draws. */
int arp_loglik_total(const float* ll, int64_t n_obs, int64_t n_draws, int64_t ll_stride, double* total, void* stream);

/* arp_element_order: the order of every element's pooled draws with the draw index carried along.  Trace addressing and
 * shape refusals are arp_rank_normalize's: element d of draw s of chain c is x[s * row_stride + c * D + d], read in place,
 * row_stride >= n_chains * D, N = n_samples * n_chains < 2^31.
 *   order[d * N + i]   the draw index r = s * n_chains + c of the i-th smallest value of element d      uint32 [D][N]
 *   sorted[d * N + i]  that value (from its key: -0 reads +0)                                   float [D][N], may be NULL
 * The order is that of arp_rank_normalize's keys (sign-flipped bits, -0 as +0, subnormals distinct, +-inf as numbers);
 * ties go in ascending r (a stable sort: the LSD radix sort of csrc/segment_sort.h, which arp_rank_normalize runs without
 * the payload).  A NaN lands at the end its sign bit sends it to and neither faults nor hangs.  Integers only: exact, and
 * no output depends on the grid or on the order atomics resolve in.  The workspace (arp_element_order_workspace_bytes: two
 * key buffers and one index buffer of the trace's size and the sort's counts; 0 for a shape that is refused) is the
 * caller's, 256-byte aligned.  Refused: what arp_rank_normalize refuses of the trace, a NULL x or order, a workspace that is
 * missing, too small or misaligned. */
int64_t arp_element_order_workspace_bytes(int64_t n_samples, int64_t n_chains, int32_t D);
int arp_element_order(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride, uint32_t* order,
                      float* sorted, void* workspace, int64_t workspace_bytes, void* stream);

/* arp_cjs_sums: what the cumulative Jensen-Shannon distance between the unweighted and the weighted ECDF of every element
 * is made of, for K weight rows at once.  sorted and order [D][N] are arp_element_order's; lw[k * lw_stride + r] (double)
 * is the log weight of draw r in row k, as arp_psis_weights writes it, 1 <= K <= 8; shift [D] float, may be NULL (0).  A
 * draw with lw = -inf is left out of row k altogether, by select (it counts in neither ECDF); a NaN lw enters and carries
 * through.  Everything is float64 after the loads.  Per (k, d), with the kept draws in sorted order i = 1 ... n',
 * W_i = exp(lw), P_i = i / n', Q_i = (sum_{j <= i} W_j) / sum W, M_i = (P_i + Q_i) / 2, b_i = x_(i+1) - x_(i) (of the kept
 * draws), log2 of 0 taken as 0, u = x - shift[d]:
 *   out[k][d][8] = { n', sum W, sum W u, sum W u^2,
 *                    A_pq = sum_{i < n'} b_i P_i (log2 P_i - log2 M_i),  A_qp = sum_{i < n'} b_i Q_i (log2 Q_i - log2 M_i),
 *                    I_p = sum_{i < n'} b_i P_i,  I_q = sum_{i < n'} b_i Q_i }
 * n' < 2 gives zeros in the last four.  n' is exact.  Scan and reduction orders depend on N alone and there are no float
 * atomics: two calls give bitwise equal output.  First-order bounds, c = ceil(N / 256) (derivation: csrc/psens.hip):
 *   sum W, sum W u, sum W u^2, I_p:  (c + 64) 2^-52 times the sum of the absolute terms;  I_q: twice that;
 *   A_pq, A_qp:  (c + 64) 2^-52 (sum b (|P log2 P| + |Q log2 Q| + (P + Q) |log2 M|) + 2 (I_p + I_q) / ln 2).
 * Refused: a NULL sorted, order, lw or out, N < 1 or >= 2^31, D < 1, more than 2^35 values, K outside 1 ... 8,
 * lw_stride < N. */
int arp_cjs_sums(const float* sorted, const uint32_t* order, int64_t N, int32_t D, const double* lw, int64_t lw_stride,
                 int32_t K, const float* shift, double* out, void* stream);

/* Per-site log prior of recorded draws (csrc/prior.hip; needs no model handle): the prior-side twin of
 * arp_pointwise_loglik.  For a block of recorded steps of the CENTRED trace x (arp_pointwise_loglik's addressing and
 * row_stride rule) and a latent site table in device memory -- one row per element d, ARP_SITE_TERMS terms each,
 *   loc_d = loc0[d] + sum_t loc_w[d * 2 + t] * x[loc_idx[d * 2 + t]]
 *   s_d   = log_scale0[d] + sum_t scale_w[d * 2 + t] * x[scale_idx[d * 2 + t]]
 *   form ARP_SITE_NORMAL:           z = (x_d - loc_d) * exp(-s_d);  lp = -0.5 * z^2 - s_d + norm[d]
 *   form ARP_SITE_NORMAL_SOFTPLUS:  sigma = max(s_d, 0) + log1p(exp(-|s_d|));  z = (x_d - loc_d) / sigma;
 *                                   lp = -0.5 * z^2 - log(sigma) + norm[d]
 *   form ARP_SITE_LOG_GAMMA:        lp = loc0[d] * x_d - exp(s_d + x_d) + norm[d]
 *                                   (x = log g, g ~ Gamma(shape loc0, rate exp(log_scale0)), Jacobian included; the loc
 *                                   terms are not read)
 * -- it writes, for draw r = step * n_chains + chain,
 *   elem_lp[r * D + d]   float, the density of element d; elem_lp may be NULL, which leaves every other output bitwise as it is
 *   group_lp[r * G + g]  double, the sum of the float32 values of the elements with group_of[d] == g, added in float64 in
 *                        an order that is a function of (D, group_of) alone (no float atomics: two calls give bitwise equal
 *                        output); group_of need not be contiguous; a group without elements is 0
 *   mask, *n_masked      as arp_pointwise_loglik's; the elem_lp and group_lp entries of a masked draw are written as 0 by select.
 * NaN and +-inf of a finite draw are results; nothing is clamped but the indices (into [0, D); group_of into [0, G)); a form
 * other than 1 or 2 is read as 0.  float32, contraction off, the loc and s chains in term order from loc0 / log_scale0,
 * rounded once per operation: with u = 2^-24, A_loc = |loc0| + sum_t |w_t x_t|, A_s = |log_scale0| + sum_t |w_t x_t|, to
 * first order against the exact value of the same float32 inputs (derivation: csrc/prior.hip)
 *   |loc_dev - loc| <= 3 u A_loc,   |s_dev - s| <= 3 u A_s
 *   form 0:  |lp_dev - lp| <= u (3 A_loc exp(-s) |z| + z^2 (5 + 3 A_s) + 4 A_s + |lp|)
 *   form 1:  |lp_dev - lp| <= u (3 A_loc |z| / sigma + z^2 (4 + B) + B + 3 |log sigma| + |lp|),  B = (3 A_s + 3) / sigma + 1
 *   form 2:  |lp_dev - lp| <= u (2 |loc0 x| + E (3 + 3 A_s + |s + x|) + |lp|),  E = exp(s + x)
 *   |group_lp - sum| <= the sum of its elements' bounds + (n_g + 4) 2^-53 sum |elem_lp|     (n_g elements in the group)
 * Nothing is read past the last element of the trace block.  Asynchronous.  Refused before any launch: a NULL pointer
 * other than elem_lp, D < 1 or D > 255, a trace shape the other diagnostics refuse, row_stride < n_chains * D, G < 1 or
 * G > D. */
enum { ARP_SITE_NORMAL = 0, ARP_SITE_NORMAL_SOFTPLUS = 1, ARP_SITE_LOG_GAMMA = 2, ARP_SITE_TERMS = 2 };
int arp_site_logprior(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                      const int32_t* form, const int32_t* loc_idx, const float* loc_w, const float* loc0,
                      const int32_t* scale_idx, const float* scale_w, const float* log_scale0, const float* norm,
                      const int32_t* group_of, int32_t G, double* group_lp, float* elem_lp /* may be NULL */,
                      uint8_t* mask, int64_t* n_masked, void* stream);

/* Ancestral draws from the prior (csrc/prior_draw.hip; needs no model handle): arp_site_logprior's table columns walked
 * front to back, n_draws times -- what a prior predictive check (Gabry et al. 2019) starts from.  x is [n_draws][row_stride]
 * float, columns d >= D are not touched; a contiguous result reads as a centred trace of one step and n_draws chains, so
 * arp_predictive_check, arp_site_logprior and arp_element_order take it in place.  Elements are drawn in ascending d;
 * loc_d and s_d are arp_site_logprior's float32 chains (term order, contraction off, indices clamped into [0, D)) over the
 * elements of the same draw drawn before d -- an element not drawn yet reads as 0, and the table is in ancestral order
 * (ModelSpec.site_table), so a term of non-zero weight never points at one.  g = draw_offset + r is the global draw number.
 *   forms ARP_SITE_NORMAL, ARP_SITE_NORMAL_SOFTPLUS:  ONE call philox4x32_10(counter = (d, lo32(g), hi32(g), 0), key =
 *     (lo32(seed), hi32(seed)));  z = sqrt(-2 log(u')) * cospi(2 a) from words 0 and 1, u' and a formed exactly as
 *     arp_predictive_check forms them, through logf, sqrtf, cospif;  x_d = loc_d + sigma_d * z, rounded twice, sigma_d =
 *     expf(s_d), or max(s_d, 0) + log1p(exp(-|s_d|)) for the softplus form
 *   form ARP_SITE_LOG_GAMMA:  x_d = log g, g ~ Gamma(shape k = loc0[d], rate exp(s_d)); the loc terms are not read.
 *     Marsaglia and Tsang (2000) in log space:  boost = k < 1;  a = boost ? k + 1 : k;  dd = a - 1/3;  c = 1 / sqrt(9 dd);
 *     attempt j = 0 ... 31 uses philox4x32_10(counter = (d, lo32(g), hi32(g), 1 + j), same key):  z from words (0, 1) as
 *     above;  t = 1 + c z, rejected if t <= 0;  U = fma((float)w2, 2^-32, 2^-33);  accepted iff
 *       log U < ((0.5 z^2 + dd) - dd ((t t) t)) + (3 dd) log t
 *     and then  x_d = ((log dd + 3 log t) + (boost ? log(U_b) / k : 0)) - s_d,  U_b formed as U from w3 of that attempt.
 *     After 32 rejections (every attempt accepts with probability above 0.95) x_d = NaN and undrawn[r] = 1.  k <= 0 or a
 *     non-finite k gives NaN without an attempt.
 *   undrawn: NULL, or [n_draws] bytes, written 0 or 1 for every draw; NULL leaves x bitwise as it is.
 * The value of (d, g) is a function of (seed, d, g) and the draw's earlier elements alone: rows [0, n) at draw_offset k
 * equal rows [k, k + n) at offset 0, bit for bit; two calls give bitwise equal output; no result depends on the launch
 * shape; no atomics.  A form other than 1 or 2 is read as 0.  float32, contraction off; with u = 2^-24, A_loc and A_s as
 * arp_site_logprior's, |z_dev - z| <= 18 u |z|, to first order against the exact value of the same float32 parents, the
 * same table and the same Philox words (derivation: csrc/prior_draw.hip; library functions at the OpenCL full-profile
 * limits):
 *   form 0:  |x_dev - x| <= u (3 A_loc + exp(s) |z| (25 + 3 A_s) + |x|)
 *   form 1:  |x_dev - x| <= u (3 A_loc + |z| (3 A_s + 6 + 20 sigma) + |x|)
 *   form 2:  |x_dev - x| <= u (5 + 6 |log dd| + 3 T + 21 |log t| + |L| + [boost: (1 + 7 |log U_b|) / k] + |L + B| + 3 A_s + |x|),
 *            T = 29 |t - 1| / t + 1,  L = log dd + 3 log t,  B = boost ? log(U_b) / k : 0
 *   the accept margin m = ((0.5 z^2 + dd) - dd t^3 + 3 dd log t) - log U is within
 *            E_m = u (19 z^2 + 6 dd + 8 dd t^3 + 39 dd |log t| + |0.5 z^2 + dd - dd t^3| + |m + log U| + 1 + 6 |log U|
 *                     + 3 dd |1 - t^3| T)
 *   of its exact value; an attempt with |m| <= E_m is undecided -- float32 and float64 may disagree about accepting it, and
 *   the form-2 bound holds for an element none of whose attempts up to the accepting one is undecided.
 * Asynchronous.  Refused before any launch: a NULL pointer other than undrawn, D < 1 or D > 255, n_draws < 1 or above 2^24,
 * row_stride < D, draw_offset < 0. */
int arp_site_prior_draws(int32_t D, const int32_t* form, const int32_t* loc_idx, const float* loc_w, const float* loc0,
                         const int32_t* scale_idx, const float* scale_w, const float* log_scale0, int64_t n_draws,
                         uint64_t seed, int64_t draw_offset, float* x, int64_t row_stride, uint8_t* undrawn /* may be NULL */,
                         void* stream);

/* Conditional redraw of recorded draws (csrc/site_redraw.hip; needs no model handle): what a mixed predictive check
 * (Gelman, Meng, Stern 1996; Marshall, Spiegelhalter 2007) replicates its data from -- the hyperparameters of every
 * posterior draw kept, the group-level elements drawn anew from their conditional prior given them.  x is a block of
 * recorded steps of the CENTRED trace [n_samples][n_chains][D], read in place with arp_pointwise_loglik's addressing and
 * row_stride rule; the table columns are arp_site_prior_draws'; redraw is [D] bytes in device memory.  out is
 * [R][out_stride] float, R = n_samples * n_chains, row r = step * n_chains + chain; columns d >= D are not touched.  For
 * draw r, g = draw_offset + r its global number, the table is walked front to back:
 *   redraw[d] == 0:  out[r][d] = x[r][d], bit for bit (NaN and +-inf included)
 *   redraw[d] != 0:  out[r][d] is drawn exactly as arp_site_prior_draws draws element d of draw g: the same three forms, the
 *     same float32 operation order with contraction off, the same philox4x32_10 counter (d, lo32(g), hi32(g), j) and key
 *     (lo32(seed), hi32(seed)), the same 32 attempts of the log-Gamma form and the same undrawn rule (one copy of the code:
 *     csrc/site_draw.h).  Its parents are read from the row being built: the redrawn value where the parent is flagged, the
 *     recorded one where it is not.
 * The row starts as the recorded value in every unflagged column and 0 in every flagged one: a flagged element reads as 0
 * until it is redrawn, as "not drawn yet" does in arp_site_prior_draws, and the flagged columns of x never enter a result
 * (they are not read).  With every element flagged, out is arp_site_prior_draws' x at the same seed and draw_offset, bit
 * for bit; with none, it is x.
 *   undrawn: NULL, or [R] bytes, written 0 or 1 for every draw (1: a flagged log-Gamma element ran out of attempts and is
 *     NaN); NULL leaves out bitwise as it is.
 * The value of (d, g) is a function of (seed, d, g), the flags and the draw's own row alone: a block of steps [s0, s1) at
 * draw_offset s0 * n_chains equals those rows of the whole, bit for bit; two calls give bitwise equal output; no result
 * depends on the launch shape or on other draws; no atomics.  The error bounds of a redrawn element are
 * arp_site_prior_draws' above, as they stand, against the exact value of the same float32 parents, the same table and the
 * same Philox words, and so is the rule for an undecided attempt.
 * WHICH elements are flagged is not policed here: a selection that is not closed under descent (an unflagged element with
 * a term of non-zero weight at a flagged one) is walked like any other and gives rows that are draws from no distribution
 * the model defines.  That rule is the host's: diagnostics.redraw_selection.
 * Nothing is read past the last element of the trace block, and no padding is read or written.  Asynchronous.  Refused
 * before any launch: a NULL pointer other than undrawn, D < 1 or D > 255, a trace shape or row_stride that
 * arp_pointwise_loglik refuses, more than 2^24 draws, out_stride < D, draw_offset < 0, out == x. */
int arp_site_redraw(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                    const int32_t* form, const int32_t* loc_idx, const float* loc_w, const float* loc0,
                    const int32_t* scale_idx, const float* scale_w, const float* log_scale0,
                    const uint8_t* redraw /* [D], device */, uint64_t seed, int64_t draw_offset, float* out, int64_t out_stride,
                    uint8_t* undrawn /* may be NULL */, void* stream);

/* The fold of simulation-based calibration (csrc/sbc.hip; needs no model handle; Talts, Betancourt, Simpson, Vehtari,
 * Gelman 2018): where the truth of every replicate sits among the posterior draws a refit on its simulated data returned.
 * draws is [n_rep][n_draws][Q] float in device memory, element (r, i, q) at draws[r * rep_stride + i * row_stride + q]
 * (rep_stride >= n_draws * row_stride, row_stride >= Q: an inner block of a wider buffer is read in place); truth is
 * [n_rep][Q] float, element (r, q) at truth[r * truth_stride + q] (truth_stride >= Q).  Outputs (device memory, contiguous),
 * per replicate r and quantity q over the replicate's n_draws rows, x = draws (r, i, q), t = truth (r, q):
 *   counts [n_rep][Q][2] int32:  #{x < t}, #{x == t}   (-0.0 == 0.0 counts as equal; denormals compare as themselves)
 *   sums   [n_rep][Q][2] double: sum (x - t), sum (x - t)^2 -- the subtraction in float64, rounded once, the square
 *     rounded once (contraction off), each sum the chain over rows i = 0 ... n_draws - 1 in that order: the order of
 *     addition does not depend on the launch shape or on the strides, and each sum is within (n_draws - 1) 2^-53 sum |term|
 *     of the exact sum of the same float64 terms, to first order
 *   left_out [n_rep] uint8: 1 for a replicate whose truth or any of whose draws has a non-finite element; its counts and
 *     sums are written as 0 (by select, not by a product); 0 otherwise
 *   n_left_out: int64 scalar, the number of such replicates (an integer count)
 * No float atomics; two calls give bitwise equal outputs; nothing is read past the last addressed element, and the
 * padding the strides leave is never read.  Asynchronous.  Refused before any launch: a NULL pointer, Q < 1 or Q > 256,
 * n_draws < 1 or above 2^24, n_rep < 1 or above 2^20, row_stride < Q, rep_stride < n_draws * row_stride, truth_stride < Q. */
int arp_sbc_fold(const float* draws, int64_t n_rep, int64_t n_draws, int32_t Q, int64_t rep_stride, int64_t row_stride,
                 const float* truth, int64_t truth_stride, int32_t* counts, double* sums, uint8_t* left_out,
                 int64_t* n_left_out, void* stream);

/* Check of a mean-field normal fit (csrc/vicheck.hip; Yao, Vehtari, Simpson, Gelman 2018, "Yes, but did it work?"): draws
 * from q = N(loc, diag(scale^2)) in the coordinates the fit was made in.  For draw r, g = draw_offset + r, and element
 * d = 4 e + i: ONE call philox4x32_10(counter = (e, lo32(g), hi32(g), 0), key = (lo32(seed), hi32(seed))) per (r, e); words
 * (0, 1) give z[4 e] = rho * cospi(2 a) and z[4 e + 1] = rho * sinpi(2 a), words (2, 3) give z[4 e + 2] and z[4 e + 3] the
 * same way, rho = sqrt(-2 log(u')), with u' and a formed from their two words exactly as arp_predictive_check forms them,
 * through logf, sqrtf, cospif and sinpif:  |z_dev - z| <= 18 * 2^-24 |z| to first order (csrc/ppc.hip's derivation; sinpi
 * has cospi's ulp figure).  Outputs (device memory): z and x [n_draws][row_stride] float, x = fmaf(scale[d], z, loc[d]),
 * columns d >= D are not touched;  logq [n_draws] double = -sum_d (z_d^2 / 2 + log(scale_d)) - (D / 2) log(2 pi), in
 * float64 from the float32 z, in ascending d.  No result depends on the launch shape: rows [0, n) at draw_offset k equal
 * rows [k, k + n) at offset 0, bit for bit.  Asynchronous.  Refused before any launch: a NULL pointer, D < 1, n_draws < 1
 * or above 2^24, row_stride < D, more than 2^35 values, draw_offset < 0.  The scale is not checked here (a scale that is
 * not finite and positive gives NaN): the Python wrapper refuses it before upload. */
int arp_vi_draws(const float* loc, const float* scale, int32_t D, int64_t n_draws, uint64_t seed, int64_t draw_offset,
                 float* x, float* z, int64_t row_stride, double* logq, void* stream);

/* Fold of a fit check (csrc/vicheck.hip): ONE pass over z (arp_vi_draws), grad (arp_logp_grad at x) and e (the centred
 * image of x, arp_transform), all [n_draws][row_stride] float, with ll [n_draws] float (the negated log ratio
 * log q - log p), lw [n_draws] double (arp_psis_weights), scale [D] and e0 [D] (the centred image of loc).  Every sum is
 * over the draws with lw > -inf (a draw the caller left out has lw = -inf; NaN does not count either), in float64.  With
 * u = scale_d * grad[r][d], c = e[r][d] - e0[d], w = exp(lw[r]):
 *   elem [D][9] = {sum u, sum u^2, sum u z, sum (u z)^2, sum (u + z)^2, sum w z, sum w z^2, sum w c, sum w c^2}
 *   tot [5]     = {kept draws, sum w, sum w^2, sum ll, min ll}
 * The rows are tiled and a second launch adds the tiles' partials in ascending order: fixed order, no float atomics, two
 * calls give bitwise equal output; tot[0] and tot[4] are exact.  The workspace (arp_vi_fold_workspace_bytes: the tiles'
 * partials; 0 for a shape that is refused) is the caller's, 256-byte aligned.  Asynchronous; device pointers.  Refused
 * before any launch: a NULL pointer, D < 1 or above 2^24, n_draws < 1 or above 2^24, row_stride < D, a workspace that is
 * missing, too small or misaligned. */
int64_t arp_vi_fold_workspace_bytes(int64_t n_draws, int32_t D);
int arp_vi_fold(const float* z, const float* grad, const float* e, int64_t row_stride, const float* ll, const double* lw,
                const float* scale, const float* e0, int64_t n_draws, int32_t D, double* elem, double* tot, void* workspace,
                int64_t workspace_bytes, void* stream);

/* Moment matching for importance sampling (csrc/mmatch.hip; needs no model handle; Paananen, Piironen, Buerkner, Vehtari
 * 2021; loo::loo_moment_match): the two device pieces of diagnostics.moment_match besides the densities and
 * arp_psis_weights.  Device pointers; asynchronous; everything is refused before any launch with 1 (arp_last_error).
 *
 * arp_weighted_moments: the first two weighted moments of every column of x for n_targets rows of log weights at once.
 * x is [n_rows][D] float, rows row_stride floats apart, read in place (1 <= D <= 255; nothing is read past a row's D-th
 * element); lw[b * lw_stride + r] (double) is the log weight of draw r for target b, as arp_psis_weights writes it: -inf
 * leaves the draw out; centre is [D] float.  Per target b, with lw_max = max_r lw (NaN entries skipped),
 * w_r = exp(lw_r - lw_max) and e = (double)x[r][d] - (double)centre[d]:
 *   out[b][4 + 2 D] double = { lw_max, sum w, sum w^2, draws kept, then for d = 0 ... D - 1 the pair sum w e, sum w e^2 }
 * The sums are about centre so that nothing cancels (arp_cjs_sums' shift); everything after the float32 load is float64.
 * A draw with lw = -inf enters nothing, by select (its row of x may be non-finite), and neither does a kept draw whose w
 * underflows to 0; a target without a kept draw gives lw_max = -inf, zeros and a count of 0; a NaN lw is kept, is counted
 * and gives NaN in the sums of ITS target and nowhere else; lw_max and the count are exact.  A row of all-zero lw gives the
 * unweighted sums.  The rows are walked in chunks of 256 and the chunks' partial sums added in ascending order by a
 * second launch; every order of addition is a function of (n_rows, D) alone and there are no float atomics: two calls give
 * bitwise equal output, and the row of target b depends neither on n_targets nor on where b stands among the targets.  A
 * chunk of x is read once for (up to) 8 targets.  First-order bound, u = 2^-53, R' kept draws, for every output sum
 * s = sum w t (t = 1, w, e, e^2), against the exact sum over the same weights w_r = exp(fl(lw_r - lw_max)):
 *   |s_dev - s| <= (R' + 32) 2 u sum w |t|
 * (R' roundings of the summation in any order, the roundings of e and of the products, one unit in the last place of exp;
 * derivation: csrc/mmatch.hip).  The workspace (arp_weighted_moments_workspace_bytes: the chunks' partial sums,
 * ceil(n_rows / 256) * n_targets * (2 + 2 D) * 8 bytes and the targets' heads; 0 for a shape that is refused) is the
 * caller's, 256-byte aligned.  Refused: a NULL x, lw, centre or out, n_rows < 1 or >= 2^31, D < 1 or D > 255, n_targets < 1
 * or > 4096, row_stride < D, lw_stride < n_rows, a workspace that is missing, too small or misaligned. */
int64_t arp_weighted_moments_workspace_bytes(int64_t n_rows, int32_t D, int64_t n_targets);
int arp_weighted_moments(const float* x, int64_t n_rows, int32_t D, int64_t row_stride, const double* lw, int64_t n_targets,
                         int64_t lw_stride, const float* centre, double* out, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* arp_affine_rows: one matrix of draws pushed through n_targets elementwise affine maps.  x as above; m, s, u are
 * [n_targets][D] float, out is [n_targets][n_rows][D] float, contiguous.  For the rows the parity picks -- every row when
 * parity < 0, the rows with (r & 1) == parity when parity is 0 or 1 --
 *   out[b][r][d] = (x[r][d] - m[b][d]) * s[b][d] + u[b][d]
 * in float32 with contraction off: three roundings, in that order.  Every other row is copied bit for bit (NaN payloads
 * and the sign of zero included).  Non-finite values are results; nothing is clamped.  An element of x is loaded once for
 * all targets; nothing is read past the D-th element of a row, so a view into a wider matrix is read in place.  No
 * workspace, no atomics; two calls give bitwise equal output, and out[b] does not depend on n_targets.  Refused: a NULL
 * pointer, n_rows < 1 or >= 2^31, D < 1 or D > 255, n_targets < 1 or > 4096, row_stride < D, parity > 1, out == x,
 * more than 2^35 values written. */
int arp_affine_rows(const float* x, int64_t n_rows, int32_t D, int64_t row_stride, const float* m, const float* s,
                    const float* u, int64_t n_targets, int32_t parity, float* out, void* stream);

/* Test hook: the step-size adaptation recurrence of the chain kernels on SCRIPTED log acceptance ratios
 * (tfp.mcmc.DualAveragingStepSizeAdaptation / SimpleStepSizeAdaptation as wired at inference.py:224-226, 288-306;
 * SURVEY.md 8c known answer (7)).  For each of `n` independent rows, applies the update after transitions
 * cfg->step_base + 1 ... cfg->step_base + n_steps with log_accept[s][row]; `adapt` is [n][4] in/out as in arp_hmc_io;
 * kappa_out ([n_steps][n] or NULL) receives the multiplier in force after each update.  Only the adapt_* fields,
 * step_base and n_steps of cfg are read. */
int arp_adapt_probe(const arp_hmc_config* cfg, const float* log_accept, int n, float* adapt, float* kappa_out,
                    void* stream);

/* Measurement hook (no reference counterpart): the shader clock the chip holds under a vector-bound load.  Runs packed FMAs
 * on every SIMD (two resident waves each) for `iters` loop iterations of 64 instructions (~ 0.27 us each) while one wave
 * reads s_memtime (shader cycles) and s_memrealtime (100 MHz) around its loop; cycles_ticks (device, 3 x uint64) receives
 * {shader cycles, 100 MHz ticks, 1}.  bench.py reports cycles / ticks x 0.1 GHz next to every roofline figure. */
int arp_clock_probe(int iters, unsigned long long* cycles_ticks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AUTOREPARAM_H_ */
