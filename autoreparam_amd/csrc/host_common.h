// Host-side plumbing shared by the API translation units: the opaque model
// handle and the per-model launcher tables (error reporting and the debug-switch gate: host_error.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../include/autoreparam.h"
#include "host_error.h"
#include "kernels.h"
#include "relay_host.h"
#include "energy_probe.h"
#include "trajectory_probe.h"
#include "model_radon.h"
#include "radon_fast.h"
#include "election_fast.h"
#include "model_schools.h"
#include "model_election.h"
#include "model_german.h"
#include "model_radon_stddvs.h"
#include "model_funnel.h"
#include "model_electric.h"
#include "model_time_series.h"

namespace arp {

// chain launchers: the kernel's parameters without a relay, what the entry point asks of one, and back what the launch did
using HmcFn = RelayGeometry (*)(const void* args, const float* a, const float* b, const HmcParams& P, const RelayAsk& ask,
                                hipStream_t s);
using InterleavedFn = RelayGeometry (*)(const void* args, const float* a0, const float* b0, const float* a1, const float* b1,
                                        const HmcParams& P, const RelayAsk& ask, hipStream_t s);
// the rows both probes walk: x[N][D], row 0 being row `row_offset` of the caller's, their step sizes and the generator's seed
struct ProbeRows { const float* x; long long N; int D; const float* eps0; const float* kappa; uint64_t seed; long long row_offset; };

// Launchers a model family exports for one (lanes-per-chain, slice-size) pair.
struct LaneOps {
  int K = 0, NL = 0;   // lanes per chain; groups (counties, states, features ...) owned by one lane
  void (*logp_grad)(const void* args, const float* a, const float* b, const float* x, int C, int D,
                    float* logp, float* grad, hipStream_t s) = nullptr;
  void (*transform)(const void* args, const float* a, const float* b, int dir, const float* in,
                    int C, int D, float* out, hipStream_t s) = nullptr;
  // chain launcher by the handle's parameterisation, indexed by kModeVIP / kModeCP / kModeNCP / kModeB1.  Launch::ops():
  // every slot holds the generic hmc_kernel, in the general (a, b) form unless the lane model has that form at compile time
  // (HAS_MODES, HAS_MODE_B1).  A family with packed kernels (radon_lane_ops, election_lane_ops) fills all four with those
  // and names no generic hmc_kernel: naming one is what compiles it
  HmcFn hmc[4] = {};
  // [0] any pair of parameterisations: the generic interleaved_kernel in the general form, in every family;
  // [1] the compile-time (CP, NCP) pair: generic where the lane model has HAS_MODES, the family's packed kernel where
  // there is one, [0] again otherwise
  InterleavedFn interleaved[2] = {};
  // mean-field VI: `n_groups` learning rates x (P.G x P.R) workgroups of vi_block threads (kernels.h: vi_kernel)
  // coop: hipLaunchCooperativeKernel -- the runtime itself guarantees that every workgroup of the grid is resident (or
  // refuses the launch), which is what the in-launch hand-offs of a learning rate's group need
  hipError_t (*vi)(const void* args, const float* a, const float* b, const ViParams& P, int n_groups, bool coop, hipStream_t s) = nullptr;
  // shape of the VI kernel's workgroups: threads, whether the lane model splits a gradient's observations into row
  // parts (German credit) and then the observations per tile of its image, and how many workgroups of it one CU holds
  // (occupancy query)
  int vi_block = 0;
  int vi_dmax = 0;
  bool vi_parts = false;
  int vi_tile_obs = 0;
  int (*vi_occ)() = nullptr;
  // energy probe (energy_probe.h): one fresh-momentum trajectory per row of x[N][D], general (a, b) form, every family
  void (*probe)(const void* args, const float* a, const float* b, const ProbeRows& r, int L, float* out4, float* p_out,
                float* q_out, hipStream_t s) = nullptr;
  // trajectory probe (trajectory_probe.h): the probe's trajectory with every step l = 1 ... Lmax recorded, every family
  void (*profile)(const void* args, const float* a, const float* b, const ProbeRows& r, int Lmax, float* energy_out,
                  float* path_out, int path_centred, float* p_out, hipStream_t s) = nullptr;
};

// threads of a VI workgroup: 128 (two waves: with 16 - 32 workgroups per learning rate five learning rates cover
// 80 - 160 CUs) unless the lane model names its own
template <class L, class = void> struct lane_vi_block { static constexpr int value = 128; };
template <class L> struct lane_vi_block<L, std::void_t<decltype(L::VI_BLOCK)>> { static constexpr int value = L::VI_BLOCK; };

template <class Lane>
struct Launch {
  static int blocks(int C) { return (int)(((long long)C * Lane::K + kBlock - 1) / kBlock); }
  static void logp_grad(const void* args, const float* a, const float* b, const float* x, int C, int D,
                        float* logp, float* grad, hipStream_t s) {
    hipLaunchKernelGGL(logp_grad_kernel<Lane>, dim3(blocks(C)), dim3(kBlock), 0, s,
                       *(const typename Lane::Args*)args, a, b, x, C, D, logp, grad);
  }
  static void transform(const void* args, const float* a, const float* b, int dir, const float* in,
                        int C, int D, float* out, hipStream_t s) {
    hipLaunchKernelGGL(transform_kernel<Lane>, dim3(blocks(C)), dim3(kBlock), 0, s,
                       *(const typename Lane::Args*)args, a, b, dir, in, C, D, out);
  }
  // the probes' grid: K lanes per row of a ProbeRows, whose row count is a long long (arp_api.hip keeps it inside a launch)
  static dim3 probe_grid(const ProbeRows& r) { return dim3((unsigned)((r.N * Lane::K + kBlock - 1) / kBlock)); }
  static void probe(const void* args, const float* a, const float* b, const ProbeRows& r, int L, float* out4, float* p_out,
                    float* q_out, hipStream_t s) {
    hipLaunchKernelGGL(energy_probe_kernel<Lane>, probe_grid(r), dim3(kBlock), 0, s, *(const typename Lane::Args*)args,
                       a, b, r.x, r.N, r.D, L, r.eps0, r.kappa, r.seed, r.row_offset, out4, p_out, q_out);
  }
  static void profile(const void* args, const float* a, const float* b, const ProbeRows& r, int Lmax, float* energy_out,
                      float* path_out, int path_centred, float* p_out, hipStream_t s) {
    hipLaunchKernelGGL(trajectory_probe_kernel<Lane>, probe_grid(r), dim3(kBlock), 0, s, *(const typename Lane::Args*)args,
                       a, b, r.x, r.N, r.D, Lmax, r.eps0, r.kappa, r.seed, r.row_offset, energy_out, path_out, path_centred, p_out);
  }
  template <int MODE>
  static RelayGeometry hmc(const void* args, const float* a, const float* b, const HmcParams& P, const RelayAsk& ask, hipStream_t s) {
    return relay_launch(hmc_kernel<Lane, MODE>, blocks(P.C), P, ask, s, *(const typename Lane::Args*)args, a, b);
  }
  template <int M0, int M1>
  static RelayGeometry interleaved(const void* args, const float* a0, const float* b0, const float* a1, const float* b1,
                                   const HmcParams& P, const RelayAsk& ask, hipStream_t s) {
    return relay_launch(interleaved_kernel<Lane, M0, M1>, blocks(P.C), P, ask, s, *(const typename Lane::Args*)args, a0, b0, a1, b1);
  }
  static constexpr int kViB = lane_vi_block<Lane>::value;
  static hipError_t vi(const void* args, const float* a, const float* b, const ViParams& P, int n_groups, bool coop, hipStream_t s) {
    if constexpr (Lane::HAS_VI) {
      if (coop) {
        void* kargs[] = {const_cast<void*>(args), (void*)&a, (void*)&b, const_cast<ViParams*>(&P)};
        return hipLaunchCooperativeKernel((const void*)vi_kernel<Lane, kViB>, dim3(n_groups * P.G * P.R), dim3(kViB), kargs, 0, s);
      }
      hipLaunchKernelGGL((vi_kernel<Lane, kViB>), dim3(n_groups * P.G * P.R), dim3(kViB), 0, s,
                         *(const typename Lane::Args*)args, a, b, P);
    }
    return hipGetLastError();
  }
  static int vi_occ() {
    int n = 0;
    if constexpr (Lane::HAS_VI)
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, vi_kernel<Lane, kViB>, kViB, 0) != hipSuccess) n = 0;
    return n;
  }
  // the VI launcher of this lane into `o` (German credit: a lane sized for the VI kernel's workgroup, in its row-part form,
  // beside chain launchers from the lane sized for kBlock)
  static void set_vi(LaneOps& o) {
    if constexpr (Lane::HAS_VI) {
      o.vi = &vi; o.vi_block = kViB; o.vi_parts = lane_has_part<Lane>::value; o.vi_occ = &vi_occ;
      o.vi_dmax = lane_vi_dmax<Lane>::value;
      if constexpr (lane_has_part<Lane>::value) o.vi_tile_obs = Lane::kTileObs;
    }
  }
  template <class L, class = void> struct has_b1 : std::false_type {};
  template <class L> struct has_b1<L, std::enable_if_t<L::HAS_MODE_B1>> : std::true_type {};
  // The table on the generic kernels, with (ops) or without (base) the chain slots hmc and interleaved.  A family whose
  // chain kernels are packed ones starts from base() and so names, and compiles, only the generic chain kernels it keeps.
  // (One body for both, so that ops() goes on naming its kernels in the order the code objects have them in.)
  static LaneOps base() { return table<false>(); }
  static LaneOps ops() { return table<true>(); }
  template <bool CHAIN>
  static LaneOps table() {
    LaneOps o;
    o.K = Lane::K; o.NL = Lane::NGRP;
    o.logp_grad = &logp_grad; o.transform = &transform;
    if constexpr (CHAIN) {
      for (auto& f : o.hmc) f = &hmc<kModeVIP>;
      for (auto& f : o.interleaved) f = &interleaved<kModeVIP, kModeVIP>;
    }
    set_vi(o);
    if constexpr (CHAIN && has_b1<Lane>::value) o.hmc[kModeB1] = &hmc<kModeB1>;
    if constexpr (CHAIN && Lane::HAS_MODES) {
      o.hmc[kModeCP] = &hmc<kModeCP>;
      o.hmc[kModeNCP] = &hmc<kModeNCP>;
      o.interleaved[1] = &interleaved<kModeCP, kModeNCP>;
    }
    o.probe = &probe;   // named last: the kernels a translation unit already had keep their order
    o.profile = &profile;   // (and after probe, for the same reason)
    return o;
  }
};

// experiments only: ARP_STATS_LDS=0 sends statistics runs down the plane-per-sample route of kernels.h again (asked once
// per process; any other value is the default and says nothing)
inline bool stats_lds_enabled() {
  static const char* const e = getenv("ARP_STATS_LDS");
  static const bool on = !(e && e[0] == '0' && debug_switch("ARP_STATS_LDS", " (statistics take the plane-per-sample route)"));
  return on;
}

// Launch of a packed chain kernel (pk_chain.h) over the chain blocks of K lanes per chain (relay_launch: x the segments
// relay_plan decides for the kernel it is given), the kernel's own arguments first, the parameters last.
// A run that accumulates statistics takes StatsLds, the instantiation with the accumulators in LDS (the same kernel as Plain
// where they do not fit: PkBlock::kStatsFit).  (StatsLds is named first because a translation unit emits its kernels in the
// order they are first named: the code objects stay byte for byte what they were.)
template <int K, auto StatsLds, auto Plain, class... Args>
RelayGeometry pk_launch(const HmcParams& P, const RelayAsk& ask, hipStream_t s, const Args&... args) {
  const int nb = (int)(((long long)P.C * K + kBlock - 1) / kBlock);
  const auto kernel = (StatsLds != Plain && P.stats && stats_lds_enabled()) ? StatsLds : Plain;
  return relay_launch(kernel, nb, P, ask, s, args...);
}
// pk_hmc_kernel in one compile-time parameterisation; AB: the kernel reads the handle's (a, b) arrays
template <class T, int MODE, bool AB = true>
RelayGeometry pk_hmc(const void* args, const float* a, const float* b, const HmcParams& P, const RelayAsk& ask, hipStream_t s) {
  return pk_launch<T::K, pk_hmc_kernel<T, MODE, PkBlock<T>::kStatsFit>, pk_hmc_kernel<T, MODE>>(
      P, ask, s, *(const typename T::Args*)args, AB ? a : nullptr, AB ? b : nullptr);
}

// Radon.  Where the packed layer of radon_fast.h applies it takes every plain HMC run (the two compile-time
// parameterisations and the general form) and the (CP, NCP) interleaving; only interleaved[0], any pair of
// parameterisations in the general form, stays on the generic interleaved_kernel.  The packed layer wants at least two
// county pairs per lane: the 13- and 15-county states at 8 / 16 lanes per chain are all generic.
template <int K, int NL>
LaneOps radon_lane_ops() {
  using G = Launch<RadonLane<K, NL>>;
  if constexpr (K >= 4 && NL >= 4) {
    using T = RadonPk<K, NL>;
    LaneOps o = G::base();
    o.hmc[kModeCP] = &pk_hmc<T, kModeCP, false>;
    o.hmc[kModeNCP] = &pk_hmc<T, kModeNCP, false>;
    // cVIP / dVIP runs: a free per county (m has unit scale, so b is inert: "a free, b = 1" and the untied form are the
    // same kernel, "hmc_vip_pk")
    o.hmc[kModeVIP] = o.hmc[kModeB1] = &pk_hmc<T, kModeVIP>;
    o.interleaved[0] = &G::template interleaved<kModeVIP, kModeVIP>;
    o.interleaved[1] = [](const void* args, const float*, const float*, const float*, const float*,
                          const HmcParams& P, const RelayAsk& ask, hipStream_t s) {
      return pk_launch<K, radon_interleaved_kernel<T, PkBlock<T>::kStatsFit>, radon_interleaved_kernel<T>>(
          P, ask, s, *(const RadonArgs*)args);
    };
    return o;
  } else {
    return G::ops();
  }
}

// Election: the packed kernels (election_fast.h on pk_chain.h) serve every plain HMC run -- the three compile-time
// parameterisations and the general per-element (a, b), "hmc_vip_pk", with the statistics accumulators in LDS where they
// fit (two workgroups per CU instead of three) -- and the (CP, NCP) interleaving.  Only interleaved[0], any pair of
// parameterisations in the general form, stays on the generic interleaved_kernel.
template <int K, int NL>
LaneOps election_lane_ops() {
  static_assert(K >= 4, "the packed kernels deal the top-level momenta out over the first slots of a chain");
  using T = ElectionPk<K, NL>;
  LaneOps o = Launch<ElectionLane<K, NL>>::base();
  o.hmc[kModeVIP] = &pk_hmc<T, kModeVIP>;
  o.hmc[kModeCP] = &pk_hmc<T, kModeCP>;
  o.hmc[kModeNCP] = &pk_hmc<T, kModeNCP>;
  o.hmc[kModeB1] = &pk_hmc<T, kModeB1>;
  o.interleaved[0] = &Launch<ElectionLane<K, NL>>::template interleaved<kModeVIP, kModeVIP>;
  // --method=i: centred / non-centred interleaving on the packed layer (pk_chain.h: pk_interleaved_kernel)
  o.interleaved[1] = [](const void* args, const float* a0, const float* b0, const float*, const float*,
                        const HmcParams& P, const RelayAsk& ask, hipStream_t s) {
    return pk_launch<K, pk_interleaved_kernel<T, kModeCP, kModeNCP, PkBlock<T>::kStatsFit>, pk_interleaved_kernel<T, kModeCP, kModeNCP>>(
        P, ask, s, *(const ElectionArgs*)args, a0, b0);
  };
  return o;
}

// German credit under one prior of the scales (model_german.h: GermanPrior).  At 4 lanes per chain the likelihood runs on the
// matrix cores, f32 or (BF3) bf16 with three-piece operands: chain kernels from the lane sized for 4 waves per workgroup, the
// VI kernel from the same lane in its row-part form, sized for the VI workgroup.
template <int PRIOR, bool BF3>
LaneOps german_lane4_ops() {
  LaneOps o = Launch<GermanLane<4, 16, kBlock / 64, false, BF3, PRIOR>>::ops();
  Launch<GermanLane<4, 16, kGermanViBlock / 64, true, BF3, PRIOR>>::set_vi(o);
  return o;
}
template <int PRIOR>
std::vector<LaneOps> german_lane_ops() {
  return {german_lane4_ops<PRIOR, false>(), Launch<GermanLane<8, 8, kBlock / 64, false, false, PRIOR>>::ops(),
          Launch<GermanLane<16, 4, kBlock / 64, false, false, PRIOR>>::ops()};
}

// per-family tables (defined in inst_*.hip)
const std::vector<LaneOps>& radon_ops();
const std::vector<LaneOps>& schools_ops();
const std::vector<LaneOps>& election_ops();
const std::vector<LaneOps>& german_ops();
const LaneOps& german_bf3_ops();   // 4 lanes per chain, likelihood on bf16 matrix cores with three-piece operands
const std::vector<LaneOps>& german_gamma_ops();   // the same two with Gamma-prior scales (german_credit_gammascale)
const LaneOps& german_gamma_bf3_ops();
const std::vector<LaneOps>& radon_sd_ops();
const std::vector<LaneOps>& funnel_ops();
const std::vector<LaneOps>& electric_ops();
const std::vector<LaneOps>& time_series_ops();

// What a model id is on the host (arp_build.hip: kFamilies, one row per ARP_MODEL_*): how its handle is built, its launcher
// table, and how an instantiation is chosen from the table (arp_api.hip: pick).
struct Family {
  int model;                                         // ARP_MODEL_*: the row's own index
  int (*build)(arp_model* m, const arp_dataset* d);  // sufficient statistics -> tables, m->args, D, n_groups, constants
  const std::vector<LaneOps>& (*ops)();
  bool exact;             // the family needs NL == ceil(groups / K) rounded up to `unit` (the random-stream partition)
  int unit;
  long long fill_lanes;   // default lanes per chain: the fewest that still put this many lanes on the device ...
  int default_lanes;      // ... or this many whatever the chain count (0: by chain count)
  int vi_lanes;           // lanes per chain of the VI kernel (0: the widest instantiation that has a VI launcher)
};
const Family* family_of(int model);   // nullptr: unknown id

}  // namespace arp

struct arp_model {
  int model = -1;
  const arp::Family* family = nullptr;
  const void* args = nullptr;   // the family's kernel arguments: the one live *Args member below (set by Family::build)
  int D = 0;
  int device = 0;
  bool host_only = false;    // test hook (arp_api.hip: host_only): no device behind this handle
  int german_math = 0;       // 0 auto (bf16 x 3 where the data allow), 1 f32 matrix cores, 2 bf16 x 3 (arp_model_set_option)
  int german_prior = 0;      // prior of German credit's feature scales, a GermanPrior: 0 log-normal centred, 1 Gamma (arp_model_set_option)
  int n_groups = 0;          // slice axis length (radon J, election 52, schools 8)
  float* dev_tables = nullptr;   // one allocation holding all frozen tables
  float* dev_ab[2] = {nullptr, nullptr};  // [2][D]: a then b, per parameterisation
  bool has_param[2] = {false, false};
  int param_kind[2] = {0, 0};   // kModeVIP / kModeCP / kModeNCP / kModeB1, detected in arp_model_set_param
  double logp_const[2] = {0.0, 0.0};
  arp::RadonArgs radon{};
  arp::SchoolsArgs schools{};
  arp::ElectionArgs election{};
  arp::GermanArgs german{};
  arp::RadonSdArgs radon_sd{};
  arp::FunnelArgs funnel{};
  arp::ElectricArgs electric{};
  arp::TimeSeriesArgs time_series{};
  std::vector<float> host_tables;
  // hand-off workspace of the VI kernel (granules + the error flag in its first 256 bytes), grown on demand
  void* vi_ws = nullptr;
  size_t vi_ws_bytes = 0;
  // the parameters a VI launch starts from, kept until its hand-offs are known to have gone through (arp_vi_run retries)
  float* vi_snap = nullptr;
  size_t vi_snap_floats = 0;
  // pinned, device-visible word a relay launch sets when a hand-over timed out (kernels.h: relay_begin; arp_model_check)
  unsigned* relay_err = nullptr;
  unsigned* relay_err_dev = nullptr;
  bool coop_ok = false;      // the device supports cooperative launches (hipDeviceAttributeCooperativeLaunch)
  int vi_launch = 0;         // 0 auto (cooperative where supported), 1 plain launch + process-wide mutex, 2 cooperative (arp_model_set_option "vi_launch")
  int cus = 0;               // CUs of `device` (relay decisions are made for the handle's device, not the current one)
  double const_base = 0.0;                       // parameterisation independent part of the dropped constant
  std::vector<std::pair<int, double>> top_scale; // (flattened index, log prior scale) of top-level latents
};
