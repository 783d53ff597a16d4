// C ABI of the engine (include/autoreparam.h): model handles, sufficient
// statistics, launcher selection.  No torch types, no callbacks.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <mutex>
#include "host_common.h"

namespace arp {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

// The measurement records, per thread as the ABI defines them, each assigned by its entry point from what the call handed back:
// what the last chain launch did (arp_relay_geometry), the geometry of the last arp_vi_run (arp_vi_geometry) and the launches it
// needed per chunk, at most (arp_vi_attempts)
static thread_local RelayGeometry g_relay_geometry = {{1, 0, 0}};
struct ViGeometry { int v[6]; };
static thread_local ViGeometry g_vi_geometry = {{0, 0, 0, 0, 0, 0}};
static thread_local int g_vi_attempts = 0;
// arp_vi_run launches whose workgroups wait for each other hold this from the launch to the end of the launch: two such
// launches from two threads of a process would share the device's workgroup slots, and a group that is only partly
// resident waits for slots the other launch's waiting groups hold
static std::mutex g_vi_launch_mutex;

// Test hook (ARP_DEBUG=1 ARP_HOST_ONLY=1, announced on stderr): model handles WITHOUT a device.  Host memory stands in
// for the device tables, so that every entry point's argument validation and host-side sizing can be driven -- and run
// under a sanitizer -- on a GPU-less machine (tests/test_api_fuzz.py).  Nothing can be computed with such a handle:
// every call that gets past validation fails with HIP's own "no device" error at its first HIP call.
static bool host_only() {
  static bool said = false;             // asked at every arp_model_create, announced once
  const char* e = getenv("ARP_HOST_ONLY");
  return e && e[0] == '1' && debug_switch("ARP_HOST_ONLY", " (handles without a device: validation only)", &said);
}

// pick the instantiation: requested lanes-per-chain (or a default from the chain
// count) and the smallest slice size that covers `groups`.
// `exact`: the family needs NL == ceil(groups / K), rounded up to a multiple of `unit` (only a lane's last slice may be
// padding; time_series: a lane owns whole time steps, unit = 2) -- the random-stream partition depends on it.
static const LaneOps* pick(const std::vector<LaneOps>& ops, int groups, int K_req, int C, bool exact,
                           long long fill_lanes, int unit) {
  auto best_for = [&](int K) -> const LaneOps* {
    const LaneOps* best = nullptr;
    const int need = ((groups + K - 1) / K + unit - 1) / unit * unit;
    for (const auto& o : ops)
      if (o.K == K && (long long)o.NL * K >= groups && (!exact || o.NL == need) &&
          (!best || o.NL < best->NL)) best = &o;
    return best;
  };
  if (K_req > 0) return best_for(K_req);
  // default: the fewest lanes per chain that still put `fill_lanes` lanes on the device (arp_build.hip: kFamilies)
  std::vector<int> Ks;
  for (const auto& o : ops) if (std::find(Ks.begin(), Ks.end(), o.K) == Ks.end()) Ks.push_back(o.K);
  std::sort(Ks.begin(), Ks.end());
  const LaneOps* last = nullptr;
  for (int K : Ks) {
    const LaneOps* o = best_for(K);
    if (!o) continue;
    last = o;
    if ((long long)C * K >= fill_lanes) return o;
  }
  return last;
}

namespace {
// test hook (arp_adapt_probe): adapt_update on scripted log acceptance ratios, one row per thread
__global__ void adapt_probe_kernel(HmcParams P, const float* __restrict__ la, int n, float* __restrict__ adapt,
                                   float* __restrict__ kappa_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float kappa = adapt[i * 4 + 0], esum = adapt[i * 4 + 1], logavg = adapt[i * 4 + 2];
  for (int s = 0; s < P.n_steps; ++s) {
    adapt_update(P, P.step_base + s + 1, la[(size_t)s * n + i], kappa, esum, logavg);
    if (kappa_out) kappa_out[(size_t)s * n + i] = kappa;
  }
  adapt[i * 4 + 0] = kappa; adapt[i * 4 + 1] = esum; adapt[i * 4 + 2] = logavg;
}

}  // namespace

}  // namespace arp

using namespace arp;

extern "C" {

int arp_version(void) { return ARP_ABI_VERSION; }
const char* arp_last_error(void) { return g_err.c_str(); }

int arp_model_create(const arp_dataset* data, arp_model** out) {
  if (!data || !out) { set_error("arp_model_create: null argument"); return 1; }
  // (before anything is allocated: an unknown id has nothing to release)
  const Family* family = family_of(data->model);
  if (!family) { set_error("arp_model_create: unknown model id"); return 1; }
  std::unique_ptr<arp_model> m(new arp_model());
  m->model = data->model;
  m->family = family;
  m->host_only = host_only();
  if (m->host_only) m->device = -1;
  else {
    ARP_HIP_OK(hipGetDevice(&m->device));
    hipDeviceProp_t prop;
    ARP_HIP_OK(hipGetDeviceProperties(&prop, m->device));
    m->cus = prop.multiProcessorCount;
    int coop = 0;
    if (hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, m->device) == hipSuccess) m->coop_ok = coop != 0;
    ARP_HIP_OK(hipHostMalloc((void**)&m->relay_err, sizeof(unsigned), hipHostMallocMapped));
    *m->relay_err = 0u;
    const hipError_t mapped = hipHostGetDevicePointer((void**)&m->relay_err_dev, m->relay_err, 0);
    if (mapped != hipSuccess) {          // (the handle is not complete yet: nothing else to release)
      (void)hipHostFree(m->relay_err);
      m->relay_err = nullptr;
      ARP_HIP_OK(mapped);
    }
  }
  const int rc = family->build(m.get(), data);
  if (rc) { arp_model_destroy(m.release()); return rc; }
  for (int w = 0; w < 2; ++w) {
    if (m->host_only) {
      m->dev_ab[w] = (float*)malloc(2 * (size_t)m->D * sizeof(float));
      if (!m->dev_ab[w]) { set_error("arp_model_create: out of memory"); arp_model_destroy(m.release()); return 1; }
      continue;
    }
    if (hipMalloc(&m->dev_ab[w], 2 * (size_t)m->D * sizeof(float)) != hipSuccess) {
      set_error("arp_model_create: hipMalloc of the parameterisation arrays failed");
      arp_model_destroy(m.release());
      return 1;
    }
  }
  // default parameterisations: 0 = CP (a=b=1), 1 = NCP (a=b=0)
  std::vector<float> ones(m->D, 1.0f), zeros(m->D, 0.0f);
  // the handle is handed over only once it is complete: on any failure the caller gets *out == NULL and nothing to destroy
  *out = nullptr;
  if (arp_model_set_param(m.get(), 0, ones.data(), ones.data()) ||
      arp_model_set_param(m.get(), 1, zeros.data(), zeros.data())) {
    arp_model_destroy(m.release());
    return 1;
  }
  *out = m.release();
  return 0;
}

int arp_model_destroy(arp_model* m) {
  if (!m) return 0;
  if (m->host_only) {
    free(m->dev_tables);
    for (int w = 0; w < 2; ++w) free(m->dev_ab[w]);
    delete m;
    return 0;
  }
  if (m->dev_tables) (void)hipFree(m->dev_tables);
  for (int w = 0; w < 2; ++w) if (m->dev_ab[w]) (void)hipFree(m->dev_ab[w]);
  if (m->vi_ws) (void)hipFree(m->vi_ws);
  if (m->vi_snap) (void)hipFree(m->vi_snap);
  if (m->relay_err) (void)hipHostFree(m->relay_err);
  delete m;
  return 0;
}

int arp_model_dim(const arp_model* m) { return m ? m->D : -1; }

int arp_model_set_option(arp_model* m, const char* key, const char* value) {
  if (!m || !key || !value) { set_error("arp_model_set_option: null argument"); return 1; }
  if (!strcmp(key, "german_math")) {
    if (m->model != ARP_MODEL_GERMAN_CREDIT) { set_error("arp_model_set_option: german_math applies to german credit only"); return 1; }
    if (!strcmp(value, "auto")) m->german_math = 0;
    else if (!strcmp(value, "f32")) m->german_math = 1;
    else if (!strcmp(value, "bf16x3")) {
      if (!m->german.Xb) { set_error("arp_model_set_option: this design matrix has more than 8 columns that need three bf16 pieces"); return 1; }
      m->german_math = 2;
    } else { set_error("arp_model_set_option: german_math is one of auto, f32, bf16x3"); return 1; }
    return 0;
  }
  if (!strcmp(key, "german_prior")) {
    // prior of the feature scales: log-normal centred (german_credit_lognormalcentered) or Gamma (german_credit_gammascale)
    if (m->model != ARP_MODEL_GERMAN_CREDIT) { set_error("arp_model_set_option: german_prior applies to german credit only"); return 1; }
    if (!strcmp(value, "lognormal")) m->german_prior = 0;
    else if (!strcmp(value, "gamma")) m->german_prior = 1;
    else { set_error("arp_model_set_option: german_prior is one of lognormal, gamma"); return 1; }
    return 0;
  }
  if (!strcmp(key, "vi_launch")) {
    // how arp_vi_run starts a kernel whose workgroups wait for each other: "cooperative" (hipLaunchCooperativeKernel),
    // "plain" (ordinary launch, one at a time per process) or "auto" (cooperative where the device supports it)
    if (!strcmp(value, "auto")) m->vi_launch = 0;
    else if (!strcmp(value, "plain")) m->vi_launch = 1;
    else if (!strcmp(value, "cooperative")) m->vi_launch = 2;
    else { set_error("arp_model_set_option: vi_launch is one of auto, plain, cooperative"); return 1; }
    return 0;
  }
  set_error("arp_model_set_option: unknown key");
  return 1;
}

double arp_model_logp_const(const arp_model* m, int which) {
  return (m && which >= 0 && which < 2) ? m->logp_const[which] : NAN;
}

int arp_model_set_param(arp_model* m, int which, const float* a_host, const float* b_host) {
  if (!m || which < 0 || which > 1 || !a_host || !b_host) { set_error("arp_model_set_param: bad argument"); return 1; }
  if (m->host_only) {
    memcpy(m->dev_ab[which], a_host, m->D * sizeof(float));
    memcpy(m->dev_ab[which] + m->D, b_host, m->D * sizeof(float));
  } else {
    ARP_HIP_OK(hipMemcpy(m->dev_ab[which], a_host, m->D * sizeof(float), hipMemcpyHostToDevice));
    ARP_HIP_OK(hipMemcpy(m->dev_ab[which] + m->D, b_host, m->D * sizeof(float), hipMemcpyHostToDevice));
  }
  m->has_param[which] = true;
  bool all1 = true, all0 = true, b1 = true;
  for (int d = 0; d < m->D; ++d) {
    all1 = all1 && a_host[d] == 1.0f && b_host[d] == 1.0f;
    all0 = all0 && a_host[d] == 0.0f && b_host[d] == 0.0f;
    b1 = b1 && b_host[d] == 1.0f;
  }
  m->param_kind[which] = all1 ? kModeCP : (all0 ? kModeNCP : (b1 ? kModeB1 : kModeVIP));
  // dropped constant: -sum_i b_i log(prior scale_i) over the top-level latents, plus the base
  double c = m->const_base;
  for (const auto& ts : m->top_scale) c -= (double)b_host[ts.first] * ts.second;
  m->logp_const[which] = c;
  return 0;
}

// The instantiation that serves K lanes per chain (0: by chain count, pick).  German credit's variant choice is made here and
// nowhere else: the prior of the scales names the table (indexed by GermanPrior: a third prior is one more entry), and at
// 4 lanes per chain the likelihood runs on bf16 matrix cores with three-piece operands where the data allow it
// (model_german.h), unless the caller asked for the f32 matrix-core form (arp_model_set_option).
static const LaneOps* lane_ops(const arp_model* m, int K, int C) {
  const Family& f = *m->family;
  const std::vector<LaneOps>* table = &f.ops();
  if (m->model == ARP_MODEL_GERMAN_CREDIT) {
    static const struct { const std::vector<LaneOps>& (*table)(); const LaneOps& (*bf3)(); } by_prior[] = {
        {german_ops, german_bf3_ops}, {german_gamma_ops, german_gamma_bf3_ops}};
    if (K == 4 && m->german.Xb && m->german_math != 1) return &by_prior[m->german_prior].bf3();
    table = &by_prior[m->german_prior].table();
  }
  return pick(*table, m->n_groups, K, C, f.exact, f.fill_lanes, f.unit);
}

static const LaneOps* select_ops(arp_model* m, int K_req, int C) {
  if (K_req != 0 && K_req != 1 && K_req != 2 && K_req != 4 && K_req != 8 && K_req != 16) {
    set_error("lanes_per_chain must be 0,1,2,4,8 or 16");
    return nullptr;
  }
  const LaneOps* o = lane_ops(m, K_req ? K_req : m->family->default_lanes, C);
  if (!o) set_error("no kernel instantiation for this (lanes_per_chain, group count): add <Model>Lane<K, ceil(groups/K)> to the model's inst_*.hip");
  return o;
}

int arp_logp_grad(arp_model* m, int which, const float* x, int n_chains, float* logp, float* grad,
                  int lanes_per_chain, void* stream) {
  if (!m || which < 0 || which > 1 || !x || !logp || !grad || n_chains <= 0) { set_error("arp_logp_grad: bad argument"); return 1; }
  const LaneOps* o = select_ops(m, lanes_per_chain, n_chains);
  if (!o) return 1;
  o->logp_grad(m->args, m->dev_ab[which], m->dev_ab[which] + m->D, x, n_chains, m->D, logp, grad,
               (hipStream_t)stream);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}

int arp_transform(arp_model* m, int which, int dir, const float* in, int n_chains, float* out, void* stream) {
  if (!m || which < 0 || which > 1 || !in || !out || n_chains <= 0 || (dir != 0 && dir != 1)) { set_error("arp_transform: bad argument"); return 1; }
  const LaneOps* o = select_ops(m, 0, n_chains);
  if (!o) return 1;
  o->transform(m->args, m->dev_ab[which], m->dev_ab[which] + m->D, dir, in, n_chains, m->D, out,
               (hipStream_t)stream);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}

// What both probes ask before a launch: a handle, x, eps0 and the output, `which` in 0 / 1, n_rows >= 1 and few enough for
// one launch (the instantiation is chosen as arp_logp_grad chooses it; the chain count it decides by is an int), and
// 1 <= n_leapfrog <= max_leapfrog (0: no upper limit).  Returns the instantiation, or nullptr with the error set; `fn` is
// the entry point the refusal names.
static const LaneOps* probe_ops(const char* fn, arp_model* m, int which, const float* x, int64_t n_rows, int n_leapfrog,
                                int max_leapfrog, const float* eps0, const float* out, int lanes_per_chain) {
  if (!m || which < 0 || which > 1 || !x || !eps0 || !out || n_rows < 1 || n_leapfrog < 1 ||
      (max_leapfrog > 0 && n_leapfrog > max_leapfrog)) {
    set_error(std::string(fn) + ": bad argument (a handle, x, eps0, the output, which in 0 / 1, n_rows >= 1 and a leapfrog "
              "count of at least 1" + (max_leapfrog > 0 ? " and at most " + std::to_string(max_leapfrog) : "") + " are required)");
    return nullptr;
  }
  if (n_rows > 0x7fffffffLL / 16) { set_error(std::string(fn) + ": n_rows is too large for one launch"); return nullptr; }
  return select_ops(m, lanes_per_chain, (int)n_rows);
}

int arp_energy_probe(arp_model* m, int which, const float* x, int64_t n_rows, int n_leapfrog, const float* eps0,
                     const float* kappa, uint64_t seed, int64_t row_offset, float* out4, float* p_out, float* q_out,
                     int lanes_per_chain, void* stream) {
  const LaneOps* o = probe_ops("arp_energy_probe", m, which, x, n_rows, n_leapfrog, 0, eps0, out4, lanes_per_chain);
  if (!o) return 1;
  o->probe(m->args, m->dev_ab[which], m->dev_ab[which] + m->D, {x, n_rows, m->D, eps0, kappa, seed, row_offset}, n_leapfrog,
           out4, p_out, q_out, (hipStream_t)stream);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}

int arp_trajectory_probe(arp_model* m, int which, const float* x, int64_t n_rows, int n_leapfrog_max, const float* eps0,
                         const float* kappa, uint64_t seed, int64_t row_offset, float* energy_out, float* path_out,
                         int path_centred, float* p_out, int lanes_per_chain, void* stream) {
  const LaneOps* o = probe_ops("arp_trajectory_probe", m, which, x, n_rows, n_leapfrog_max, 256, eps0, energy_out, lanes_per_chain);
  if (!o) return 1;
  o->profile(m->args, m->dev_ab[which], m->dev_ab[which] + m->D, {x, n_rows, m->D, eps0, kappa, seed, row_offset},
             n_leapfrog_max, energy_out, path_out, path_centred, p_out, (hipStream_t)stream);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}

// The step-size recurrences compare log alpha itself with log(target) (kernels.h: adapt_update), which equals TFP's
// min(log alpha, 0) > log(target) only for a target below 1; a rate <= -1 would flip or zero the step.
static int check_adapt(const arp_hmc_config* cfg) {
  if (cfg->adapt_kind == ARP_ADAPT_NONE) return 0;
  if (!(cfg->adapt_target > 0.0f && cfg->adapt_target < 1.0f)) { set_error("adapt_target must lie in (0, 1)"); return 1; }
  if (cfg->adapt_kind == ARP_ADAPT_SIMPLE && !(cfg->adapt_rate > 0.0f)) { set_error("adapt_rate must be positive"); return 1; }
  return 0;
}
// the adaptation schedule as the kernels read it (kernels.h: adapt_update)
static void fill_adapt(HmcParams& P, const arp_hmc_config* cfg) {
  P.adapt_kind = cfg->adapt_kind; P.n_adapt = cfg->n_adapt;
  P.adapt_target = cfg->adapt_target; P.adapt_rate = cfg->adapt_rate;
  P.adapt_log_target = logf(cfg->adapt_target > 0.f ? cfg->adapt_target : 1e-30f);
  P.adapt_inv_opr = 1.0f / (1.0f + cfg->adapt_rate);
}

static int fill_params(arp_model* m, const arp_hmc_config* cfg, const arp_hmc_io* io, bool need_cache, HmcParams* Pp) {
  if (cfg->n_chains <= 0 || cfg->n_leapfrog <= 0 || cfg->n_steps < 0 || cfg->thin <= 0 || cfg->step_base < 0) {
    set_error("n_chains, n_leapfrog, thin must be positive and n_steps, step_base non-negative");
    return 1;
  }
  if (!io->q || !io->adapt || !io->rng || !io->accept_count || !io->eps0 ||
      (need_cache && (!io->grad || !io->logp))) {
    set_error("q, grad, logp, adapt, rng, accept_count and eps0 are required");
    return 1;
  }
  if (cfg->adapt_kind < ARP_ADAPT_NONE || cfg->adapt_kind > ARP_ADAPT_SIMPLE) { set_error("bad adapt_kind"); return 1; }
  if (check_adapt(cfg)) return 1;
  if (m->D > kMaxD) { set_error("state dimension exceeds the chain kernels' limit (256)"); return 1; }
  HmcParams& P = *Pp;
  P.C = cfg->n_chains; P.L = cfg->n_leapfrog; P.n_steps = cfg->n_steps;
  P.step_base = cfg->step_base; P.chain_offset = cfg->chain_offset; P.seed = cfg->seed;
  fill_adapt(P, cfg);
  P.n_burnin = cfg->n_burnin; P.thin = cfg->thin;
  P.n_samples = (io->trace || io->trace_accept || io->stats || io->rec_accept_count) ? cfg->n_samples : 0;
  if (io->stats && cfg->stats_batch < 1) { set_error("stats_batch must be >= 1 when stats is given"); return 1; }
  P.trace_centered = cfg->trace_centered;
  P.stats_batch = cfg->stats_batch > 0 ? cfg->stats_batch : 1;
  rec_schedule(P);             // rec_step, rec_row, stats_bpos (kernels.h)
  P.D = m->D;
  P.q = io->q; P.grad = io->grad; P.logp = io->logp; P.adapt = io->adapt;
  P.rng = io->rng; P.accept_count = io->accept_count; P.eps0 = io->eps0;
  P.trace = io->trace; P.trace_accept = io->trace_accept; P.stats = io->stats; P.rec_accept = io->rec_accept_count;
  P.trace_chains = (cfg->trace_chains > 0 && cfg->trace_chains < cfg->n_chains) ? cfg->trace_chains : cfg->n_chains;
  P.L1 = 0; P.adapt1 = nullptr; P.accept_count1 = nullptr; P.eps0_1 = nullptr; P.trace_accept1 = nullptr;
  P.rec_accept1 = nullptr;
  relay_off(P);      // (the launcher's relay_plan writes the segments in, where it decides on any: relay_host.h)
  return 0;
}

int arp_model_check(arp_model* m) {
  if (!m) { set_error("arp_model_check: null argument"); return 1; }
  return relay_failed(m->relay_err, "arp_model_check");
}

int arp_hmc_run(arp_model* m, int which, const arp_hmc_config* cfg, const arp_hmc_io* io, void* stream) {
  if (!m || !cfg || !io || which < 0 || which > 1) { set_error("arp_hmc_run: null argument"); return 1; }
  if (relay_failed(m->relay_err, "arp_hmc_run")) return 1;
  HmcParams P;
  if (fill_params(m, cfg, io, true, &P)) return 1;
  if (cfg->n_steps == 0) return 0;
  const LaneOps* o = select_ops(m, cfg->lanes_per_chain, cfg->n_chains);
  if (!o) return 1;
  RelayAsk ask;
  if (relay_prepare(m->cus, m->relay_err_dev, cfg, o->K, true, (hipStream_t)stream, &ask)) return 1;
  // (kModeVIP too: where a family has the general form on the packed layer, "hmc_vip_pk", it sits in that slot -- host_common.h)
  g_relay_geometry = o->hmc[m->param_kind[which]](m->args, m->dev_ab[which], m->dev_ab[which] + m->D, P, ask, (hipStream_t)stream);
  return relay_release(ask, g_relay_geometry, hipGetLastError(), (hipStream_t)stream);
}

int arp_interleaved_run(arp_model* m, const arp_hmc_config* cfg, int n_leapfrog_1,
                        const arp_interleaved_io* io, void* stream) {
  if (!m || !cfg || !io) { set_error("arp_interleaved_run: null argument"); return 1; }
  if (n_leapfrog_1 <= 0 || !io->adapt1 || !io->accept_count1 || !io->eps0_1) {
    set_error("arp_interleaved_run: n_leapfrog_1, adapt1, accept_count1 and eps0_1 are required");
    return 1;
  }
  if (io->k0.grad && !io->k0.logp) {
    // radon_interleaved_kernel (radon_fast.h) carries the gradient across the change of coordinates and keeps BOTH between calls
    set_error("arp_interleaved_run: k0.logp is required whenever k0.grad is given (pass both or neither)");
    return 1;
  }
  if (relay_failed(m->relay_err, "arp_interleaved_run")) return 1;
  HmcParams P;
  if (fill_params(m, cfg, &io->k0, false, &P)) return 1;
  if (io->trace_accept1 && !P.n_samples) P.n_samples = cfg->n_samples;
  P.L1 = n_leapfrog_1; P.adapt1 = io->adapt1; P.accept_count1 = io->accept_count1;
  P.eps0_1 = io->eps0_1; P.trace_accept1 = io->trace_accept1; P.rec_accept1 = io->rec_accept_count1;
  if (cfg->n_steps == 0) return 0;
  const LaneOps* o = select_ops(m, cfg->lanes_per_chain, cfg->n_chains);
  if (!o) return 1;
  const auto fn = o->interleaved[m->param_kind[0] == kModeCP && m->param_kind[1] == kModeNCP];
  // (radon_interleaved_kernel carries the gradient from step to step: it has to travel with the state, as it does between launches)
  RelayAsk ask;
  if (relay_prepare(m->cus, m->relay_err_dev, cfg, o->K, io->k0.grad != nullptr, (hipStream_t)stream, &ask)) return 1;
  g_relay_geometry = fn(m->args, m->dev_ab[0], m->dev_ab[0] + m->D, m->dev_ab[1], m->dev_ab[1] + m->D, P, ask, (hipStream_t)stream);
  return relay_release(ask, g_relay_geometry, hipGetLastError(), (hipStream_t)stream);
}

// arp_vi_run's arguments, the instantiation that serves them (*op), the kernel's view of them (P: all but the geometry and the
// workspace) and the group arrays
static int vi_check(arp_model* m, int which, const arp_vi_config* cfg, const arp_vi_io* io, hipStream_t stream,
                    const LaneOps** op, ViParams& P) {
  if (!m || !cfg || !io || which < 0 || which > 1) { set_error("arp_vi_run: null argument"); return 1; }
  if (cfg->n_lr <= 0 || cfg->n_steps <= 0 || cfg->n_mc <= 0 || cfg->n_mc > 4096) {
    set_error("arp_vi_run: n_lr, n_steps must be positive and 0 < n_mc <= 4096");
    return 1;
  }
  if (!io->lr || !io->loc || !io->rho || !io->elbo || (cfg->learn_a && !io->w)) {
    set_error("arp_vi_run: lr, loc, rho, elbo (and w when learn_a) are required");
    return 1;
  }
  if (m->D > kViDmax) { set_error("arp_vi_run: model dimension exceeds the VI kernel's limit"); return 1; }
  // the VI kernel wants the smallest per-lane slice: the widest lanes-per-chain instantiation that has one, unless the
  // family names its own (german credit: its matrix-core instantiation, in the variant the chain kernels take too)
  int K_vi = m->family->vi_lanes;
  if (!K_vi) for (const auto& t : m->family->ops()) if (t.vi) K_vi = std::max(K_vi, t.K);
  const LaneOps* o = *op = lane_ops(m, K_vi, 1 << 30);
  if (!o || !o->vi) { set_error("no VI kernel instantiation covers this group count"); return 1; }
  if (m->D > o->vi_dmax) { set_error("arp_vi_run: model dimension exceeds this model's VI kernel instantiation"); return 1; }
  P.n_steps = cfg->n_steps; P.n_mc = cfg->n_mc; P.learn_a = cfg->learn_a; P.tied_b = cfg->tied_b; P.a_prior = cfg->a_prior; P.D = m->D;
  P.seed = cfg->seed;
  P.const_base = (float)m->const_base;
  P.n_top = (int)m->top_scale.size();
  for (int k = 0; k < 4; ++k) { P.top_idx[k] = 0; P.top_logscale[k] = 0.f; }
  for (int k = 0; k < P.n_top; ++k) { P.top_idx[k] = m->top_scale[k].first; P.top_logscale[k] = (float)m->top_scale[k].second; }
  P.lr = io->lr; P.loc = io->loc; P.rho = io->rho; P.w = io->w; P.wb = cfg->learn_a ? io->wb : nullptr;
  P.elbo = io->elbo;
  P.prior = cfg->a_prior ? io->prior : nullptr;
  P.a_group = (cfg->learn_a && !cfg->tied_b) ? io->a_group : nullptr;
  P.b_group = (cfg->learn_a && io->wb) ? io->b_group : nullptr;
  // The kernel indexes LDS with these (device) arrays and assumes a group's members sit contiguously behind their
  // leader: check that here, once per fit ([D] ints each).
  for (const int* grp : {P.a_group, P.b_group}) {
    if (!grp) continue;
    std::vector<int> g(m->D);
    ARP_HIP_OK(hipMemcpyAsync(g.data(), grp, m->D * sizeof(int), hipMemcpyDeviceToHost, stream));
    ARP_HIP_OK(hipStreamSynchronize(stream));
    for (int d = 0; d < m->D; ++d) {
      const int l = g[d];
      bool ok = l >= 0 && l <= d && g[l] == l;
      for (int e = l; ok && e <= d; ++e) ok = g[e] == l;     // every element between the leader and d belongs to it
      if (!ok) {
        set_error("arp_vi_run: a_group / b_group must map every element to the first element of a contiguous group (0 <= g[d] <= d, g[g[d]] == g[d])");
        return 1;
      }
    }
  }
  return 0;
}

// Geometry of arp_vi_run's launches (kernels.h: vi_kernel): G sample groups x R row parts per learning rate.  It decides
// whether a learning rate's workgroups are resident together, that is, whether a fit finishes or runs into its bounds.
struct ViPlan {
  int B, K;                  // threads of a workgroup, lanes per chain
  int G, R, GR;              // sample groups, row parts, workgroups of a learning rate (G * R)
  int occ;                   // workgroups of the kernel one CU holds (occupancy query)
  long long capacity;        // workgroups the plan lets be resident together
  int groups_per_launch;     // learning rates one launch takes
  int nq, Tp;                // quantities per latent the workgroups exchange; floats of an exchanged row, padded
  size_t ws_bytes;           // hand-off workspace: the error flag's 256 bytes, then the granules
  size_t snap_floats;        // the rows a launch starts from, kept for a retry (0: nothing waits, nothing is retried)
  bool coop;                 // cooperative launch
};
// Arithmetic only: no HIP call, nothing of the handle.  `o`: the instantiation's shape (K, vi_block, vi_parts); occ: its
// occupancy query; tiles: tiles of German credit's observations (vi_parts); g_max, r_forced: ARP_VI_G / ARP_VI_R (0: not
// set); n_keep: parameter rows per learning rate a retry restores.
static int vi_plan(const arp_vi_config* cfg, int D, const LaneOps& o, int occ, int cus, int tiles, int g_max, int r_forced,
                   int n_keep, int vi_launch, bool coop_ok, ViPlan* plan) {
  ViPlan& p = *plan;
  const int B = p.B = o.vi_block, K = p.K = o.K;
  const int CPW = B / K;                                 // draws a workgroup takes per pass
  const int unit = kViBlock / B;                         // G must be a multiple of this when a lane takes several draws
  int G = (cfg->n_mc + CPW - 1) / CPW;                   // one pass
  int R = 1;
  // German credit: the observations' tiles (128 rows on f32 matrix cores, 64 on bf16 x 3) are split too, so that a learning
  // rate's group has about 32 workgroups (five learning rates: 160 CUs) and a gradient is two tiles of matrix-core work per wave
  if (o.vi_parts) R = std::min(tiles, std::max(1, 32 / G));
  if (g_max > 0 && !o.vi_parts) G = std::min(G, g_max);      // experiments (ARP_DEBUG=1 only)
  if (r_forced > 0 && o.vi_parts) R = r_forced;
  p.occ = occ;
  if (occ <= 0) { set_error("arp_vi_run: the VI kernel does not fit on this device (occupancy query)"); return 1; }
  // every workgroup of a group has to be resident together (they wait for each other twice per step).  One or two per
  // CU is an LDS or register-file limit, which the query gets right; at more than that it can be one workgroup per CU
  // high (MI355X_MICROARCH.md, residency: the scalar-register edge), so one is given away
  const long long capacity = p.capacity = (long long)(occ > 2 ? occ - 1 : occ) * cus;
  while ((long long)G * R > capacity && R > 1) R = (R + 1) / 2;
  if ((long long)G * R > capacity && o.vi_parts) {
    set_error("arp_vi_run: n_mc draws of this model do not fit on the device in one pass");   // 4 096 draws: 128 workgroups
    return 1;
  }
  if ((long long)G * R > capacity) G = (int)std::max<long long>(unit, capacity / R / unit * unit);
  if ((long long)G * CPW < cfg->n_mc && G % unit != 0) G = (G + unit - 1) / unit * unit;   // several draws per lane: whole turns
  if ((long long)G * R > capacity) { set_error("arp_vi_run: one learning rate's workgroups do not fit on this device"); return 1; }
  p.G = G; p.R = R;
  const int GR = p.GR = G * R;
  p.groups_per_launch = (int)std::max<long long>(1, std::min<long long>(cfg->n_lr, capacity / GR));
  p.nq = cfg->learn_a ? 4 : 2;
  p.Tp = (p.nq * D + 1 + 15) & ~15;
  p.ws_bytes = GR > 1 ? 256 + p.groups_per_launch * vi_xch_group_granules(GR, p.Tp) * 8 : 256;
  p.snap_floats = GR > 1 ? (size_t)n_keep * p.groups_per_launch * D : 0;
  // A group's workgroups wait for each other, so all of them must be resident.  Cooperative launch (the default where the
  // device has it): the runtime checks the grid against the device's capacity and serialises such launches of the process.
  // Plain launch: the occupancy arithmetic above plus one such launch at a time in this process (the mutex).  Neither holds
  // against kernels of other queues or processes: see the retry (vi_launch_chunks).
  p.coop = GR > 1 && (vi_launch == 2 || (vi_launch == 0 && coop_ok));
  if (vi_launch == 2 && !coop_ok) { set_error("arp_vi_run: vi_launch=cooperative but the device does not support cooperative launches"); return 1; }
  return 0;
}

// A handle-owned device buffer grown to `count` elements of `elem` bytes (never shrunk).  The old one is given back only
// once the work on `stream` that may still read it is done.
static int grow_device(void** buf, size_t* have, size_t count, size_t elem, hipStream_t stream) {
  if (*have >= count) return 0;
  if (*buf) { ARP_HIP_OK(hipStreamSynchronize(stream)); (void)hipFree(*buf); *buf = nullptr; *have = 0; }
  ARP_HIP_OK(hipMalloc(buf, count * elem));
  *have = count;
  return 0;
}

// the parameter rows of a chunk (`chunk` floats each, from float `first` of every row) to the snapshot, or back
static int vi_snapshot(float* snap, float* const (&rows)[4], size_t first, size_t chunk, bool restore, hipStream_t stream) {
  size_t k = 0;
  for (float* r : rows) {
    if (!r) continue;
    float* const live = r + first;
    float* const kept = snap + (k++) * chunk;
    ARP_HIP_OK(hipMemcpyAsync(restore ? live : kept, restore ? kept : live, chunk * sizeof(float), hipMemcpyDeviceToDevice, stream));
  }
  return 0;
}

// The learning rates, plan.groups_per_launch per launch.  A launch whose hand-offs ran into their bound (the device was
// shared with kernels of other queues or processes for that long: no launch mode guarantees residency against THOSE) is not
// an error yet: the parameters it started from are kept, and it is taken again with four times the bound -- 2 s, 8 s, 32 s
// -- before the call gives up.  A fit under contention is slower, not failed; an undisturbed one never takes the second launch
// (*attempts: the launches a chunk needed, at most).
static int vi_launch_chunks(arp_model* m, int which, const LaneOps* o, const arp_vi_config* cfg, const arp_vi_io* io,
                            const ViPlan& plan, ViParams P, std::unique_lock<std::mutex>& one_at_a_time, hipStream_t stream, int* attempts) {
  const int GR = plan.GR, groups_per_launch = plan.groups_per_launch;
  const size_t rowf = (size_t)m->D;
  int dbg = 0, fault_attempts = 0;      // test hook (ARP_DEBUG=1): treat the first n launches of every chunk as timed out
  if (debug_int("ARP_VI_FAULT_ATTEMPTS", &dbg) && dbg > 0) fault_attempts = dbg;
  for (int lr0 = 0; lr0 < cfg->n_lr; lr0 += groups_per_launch) {
    const int ng = std::min(groups_per_launch, cfg->n_lr - lr0);
    float* const rows[4] = {io->loc, io->rho, io->w, (io->wb && cfg->learn_a) ? io->wb : nullptr};
    const size_t chunk = (size_t)ng * rowf;
    if (GR > 1 && vi_snapshot(m->vi_snap, rows, (size_t)lr0 * rowf, chunk, false, stream)) return 1;
    P.lr0 = lr0;
    P.spin_ticks = kViSpinTicks;
    for (int attempt = 0;; ++attempt) {
      if (attempt > 0) {
        if (vi_snapshot(m->vi_snap, rows, (size_t)lr0 * rowf, chunk, true, stream)) return 1;
        P.spin_ticks *= 4;
      }
      // every polled word starts at zero (epochs start at 1): the flag and this launch's granules
      ARP_HIP_OK(hipMemsetAsync(m->vi_ws, 0, plan.ws_bytes, stream));
      hipError_t launched = o->vi(m->args, m->dev_ab[which], m->dev_ab[which] + m->D, P, ng, plan.coop, stream);
      if (plan.coop && m->vi_launch == 0 && (launched == hipErrorCooperativeLaunchTooLarge || launched == hipErrorNotSupported)) {
        // "auto" only: the runtime counts co-residency more strictly than the occupancy query (vi_plan) (or lacks the feature
        // after all) -- take the plain launch, one at a time per process, as round 5 did
        (void)hipGetLastError();
        if (!one_at_a_time.owns_lock()) one_at_a_time.lock();
        launched = o->vi(m->args, m->dev_ab[which], m->dev_ab[which] + m->D, P, ng, false, stream);
      }
      ARP_HIP_OK(launched);
      *attempts = std::max(*attempts, attempt + 1);
      if (GR <= 1) break;
      // the hand-offs' waits are bounded: a group that was not resident together reports it here instead of hanging
      int err = 0;
      ARP_HIP_OK(hipMemcpyAsync(&err, m->vi_ws, sizeof(int), hipMemcpyDeviceToHost, stream));
      ARP_HIP_OK(hipStreamSynchronize(stream));
      if (attempt < fault_attempts) err = 1;
      if (!err) break;
      if (attempt == 2) {
        set_error("arp_vi_run: a hand-off between the workgroups of a learning rate timed out three times (2 s, 8 s, 32 s: the "
                  "group was never resident together -- is another process holding the device?)");
        return 1;
      }
    }
  }
  return 0;
}

int arp_vi_run(arp_model* m, int which, const arp_vi_config* cfg, const arp_vi_io* io, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const LaneOps* o = nullptr;
  ViParams P;
  if (vi_check(m, which, cfg, io, st, &o, P)) return 1;
  int g_max = 0, r_forced = 0;
  debug_int("ARP_VI_G", &g_max);
  debug_int("ARP_VI_R", &r_forced);
  const int tiles = o->vi_parts ? (m->german.N + o->vi_tile_obs - 1) / o->vi_tile_obs : 0;
  const int n_keep = 2 + (io->w ? 1 : 0) + (io->wb && cfg->learn_a ? 1 : 0);
  ViPlan plan;
  if (vi_plan(cfg, m->D, *o, o->vi_occ ? o->vi_occ() : 0, m->cus, tiles, g_max, r_forced, n_keep, m->vi_launch, m->coop_ok, &plan)) return 1;
  if (grow_device(&m->vi_ws, &m->vi_ws_bytes, plan.ws_bytes, 1, st)) return 1;
  P.G = plan.G; P.R = plan.R; P.xch_tp = plan.Tp;
  P.err = (int*)m->vi_ws;
  P.xch = plan.GR > 1 ? (unsigned long long*)((char*)m->vi_ws + 256) : nullptr;
  // plain launches of waiting workgroups: one at a time in this process, from here to the end of the call
  std::unique_lock<std::mutex> one_at_a_time(g_vi_launch_mutex, std::defer_lock);
  if (plan.GR > 1 && !plan.coop) one_at_a_time.lock();
  int attempts = 0;
  const int rc = grow_device((void**)&m->vi_snap, &m->vi_snap_floats, plan.snap_floats, sizeof(float), st) ||
                 vi_launch_chunks(m, which, o, cfg, io, plan, P, one_at_a_time, st, &attempts);
  // this thread's records of the call, failed or not: the plan's geometry, and the launches its chunks took
  g_vi_geometry = {plan.B, plan.G, plan.R, plan.groups_per_launch,
                   (int)std::min<long long>((long long)cfg->n_lr * plan.GR, plan.capacity), plan.occ};
  g_vi_attempts = attempts;
  return rc;
}

int arp_vi_attempts(int32_t* out1) {
  if (!out1) { set_error("arp_vi_attempts: null argument"); return 1; }
  *out1 = g_vi_attempts;
  return 0;
}

int arp_relay_schedule(int n_steps, int segs, int ratio_pct, int32_t* out, int cap) {
  if (!out || n_steps < 1 || segs < 1 || segs > n_steps || segs > cap || ratio_pct > 100) {
    set_error("arp_relay_schedule: want 1 <= segs <= n_steps, segs <= cap, ratio_pct <= 100 and a buffer");
    return 0;
  }
  std::vector<int> len(segs);
  relay_schedule(n_steps, segs, (ratio_pct > 0 ? ratio_pct : kSegRatioPct) / 100.0, len.data());
  for (int s = 0; s < segs; ++s) out[s] = len[s];
  return segs;
}

int arp_relay_geometry(int32_t* out3) {
  if (!out3) { set_error("arp_relay_geometry: null argument"); return 1; }
  for (int i = 0; i < 3; ++i) out3[i] = g_relay_geometry.v[i];
  return 0;
}

int arp_vi_geometry(int32_t* out6) {
  if (!out6) { set_error("arp_vi_geometry: null argument"); return 1; }
  for (int i = 0; i < 6; ++i) out6[i] = g_vi_geometry.v[i];
  return 0;
}

int arp_adapt_probe(const arp_hmc_config* cfg, const float* log_accept, int n, float* adapt, float* kappa_out,
                    void* stream) {
  if (!cfg || !log_accept || !adapt || n <= 0 || cfg->n_steps < 0 || cfg->step_base < 0) {
    set_error("arp_adapt_probe: bad argument");
    return 1;
  }
  if (cfg->adapt_kind < ARP_ADAPT_NONE || cfg->adapt_kind > ARP_ADAPT_SIMPLE) { set_error("bad adapt_kind"); return 1; }
  if (check_adapt(cfg)) return 1;
  HmcParams P{};
  P.n_steps = cfg->n_steps; P.step_base = cfg->step_base;
  fill_adapt(P, cfg);
  hipLaunchKernelGGL(adapt_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, log_accept, n, adapt,
                     kappa_out);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}

}  // extern "C"
