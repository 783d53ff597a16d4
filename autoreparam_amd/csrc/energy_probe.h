// Energy probe: for every state handed to it, one trajectory of the sampler's integrator from a FRESH momentum, and the
// energies at both ends.  Not a replay of the transition the sampler took from that state: at stationarity state and
// fresh momentum are independent, so the probed trajectory has the distribution of the sampler's next transition, and the
// divergence rate, the energy-error moments and the expected acceptance over many probed states estimate the sampler's
// own.  The state is not changed and there is no Metropolis test.  The chain kernels are not involved: the momentum draw
// below is the probe's own (one stream per (row_offset + row, slot, K), layout 0 for every lane model).
#pragma once
#include "kernels.h"

namespace arp {

// Thread-to-(row, slot) mapping, dead-lane shadowing and prologue of logp_grad_kernel; integrator of hmc_transition
// (half kick, drift, L - 1 x kick-drift, gradient, closing half kick) in the general (a, b) form, without the LDS parking.
// out[r] = {lp0, ke0, lp1, ke1} as computed (NaN and +-inf are results); p_out / q_out (or null): the drawn momentum and
// the end state, [N][D].  (trajectory_probe_kernel restates the lines from load_row to ke0: an edit here goes there too.)
template <class Lane>
__global__ __launch_bounds__(kBlock, Lane::MINW) void energy_probe_kernel(
    typename Lane::Args A, const float* __restrict__ av, const float* __restrict__ bv, const float* __restrict__ x,
    long long N, int D, int L, const float* __restrict__ eps0, const float* __restrict__ kappa, uint64_t seed,
    long long row_offset, float* __restrict__ out, float* __restrict__ p_out, float* __restrict__ q_out) {
  constexpr int K = Lane::K, ND = Lane::ND, NG = Lane::NG;
  long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  int slot = (int)(t % K);
  long long c = t / K;
  bool live = c < N;
  long long cc = live ? c : N - 1;  // dead lanes shadow the last row (keeps DPP groups uniform)
  ARP_LANE_SMEM(Lane);
  Lane M;
  lane_tables(M, A, s_lane_tab);
  M.init(A, av, bv, slot);

  float q[ND], g[ND], p[ND], eps[ND];
  load_row(M, x + cc * D, q);
  load_row(M, eps0, eps);
  if (kappa) {
    const float k = kappa[cc];
#pragma unroll
    for (int i = 0; i < ND; ++i) eps[i] *= k;
  }

  // every lane draws ND normals from its own stream; the replicated top-level elements take slot 0's draw, padding gets none
  Rng rng = rng_seed(seed, (unsigned long long)(row_offset + cc), (uint32_t)slot, (uint32_t)K);
#pragma unroll
  for (int i = 0; i < ND; i += 2) {
    float z0, z1;
    uint32_t w0 = rng_next(rng), w1 = rng_next(rng);
    normal_pair(w0, w1, z0, z1);
    p[i] = z0;
    if (i + 1 < ND) p[i + 1] = z1;
  }
#pragma unroll
  for (int i = 0; i < NG; ++i) p[i] = group_bcast0<K>(p[i], M.slot);
  float ke0 = 0.0f, keg0 = 0.0f;
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    if (i < NG) {
      keg0 = fmaf(p[i], p[i], keg0);
    } else {
      p[i] = M.lvalid(i - NG) ? p[i] : 0.0f;
      ke0 = fmaf(p[i], p[i], ke0);
    }
  }
  ke0 = 0.5f * (group_sum<K>(ke0) + keg0);
  if (p_out) store_row(M, p_out + cc * D, p, live);

  const float lp0 = lane_grad<kModeVIP, true>(M, q, g);
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    p[i] = fmaf(0.5f * eps[i], g[i], p[i]);
    q[i] = fmaf(eps[i], p[i], q[i]);
  }
  for (int l = 1; l < L; ++l) lane_kick_drift<kModeVIP>(M, q, p, eps);
  const float lp1 = lane_grad<kModeVIP, true>(M, q, g);
#pragma unroll
  for (int i = 0; i < ND; ++i) p[i] = fmaf(0.5f * eps[i], g[i], p[i]);
  float ke1 = 0.0f, keg1 = 0.0f;
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    if (i < NG) keg1 = fmaf(p[i], p[i], keg1); else ke1 = fmaf(p[i], p[i], ke1);
  }
  ke1 = 0.5f * (group_sum<K>(ke1) + keg1);

  if (q_out) store_row(M, q_out + cc * D, q, live);
  if (live && slot == 0) {
    float* o = out + c * 4;
    o[0] = lp0; o[1] = ke0; o[2] = lp1; o[3] = ke1;
  }
}

}  // namespace arp
