// Trajectory probe: the energy probe's trajectory (energy_probe.h) with every intermediate step recorded.  For every state
// handed to it, ONE trajectory of Lmax leapfrog steps from a FRESH momentum, and after each step l = 1 ... Lmax the log
// density, the kinetic energy the trajectory would end with if it stopped there, and the state: what the Metropolis-weighted
// expected squared jump distance of a sampler with l leapfrogs is made of, for every l at once (jump.hip folds it;
// diagnostics.profile_from_sums reads it).  What the profile is and is not:
//   - the trajectories start from fresh momenta: they are NOT replays of the sampler's transitions;
//   - the step sizes are those the run adapted for its own leapfrog count: a run at another count would adapt others;
//   - the expected squared jump distance is a one-transition (lag-one) criterion, not an effective sample size.
// The state is not changed and there is no Metropolis test.  The chain kernels are not involved.
#pragma once
#include "kernels.h"

namespace arp {

// Thread-to-(row, slot) mapping, dead-lane shadowing, step-size load and momentum draw of energy_probe_kernel, the same
// stream key (seed, row_offset + row, slot, K): with equal seed, offset and lanes p_out and ke0 are that kernel's bit for bit.
// (The lines from load_row to ke0 are that kernel's, restated: an edit to one goes into the other.  A shared function was
// tried and compiles to other schedules in a quarter of the instantiations, NOTES_r07.md; what holds the two together is
// tests/test_gpu_trajectory.py::test_same_stream_as_the_energy_probe, on every family and lane shape.)
// Integrator: half kick, drift, then per step gradient (with the log density: the fused kick_drift of the radon and
// election lanes returns none), full kick, drift.  The half kick that would close a trajectory of l steps goes into a
// temporary, for the kinetic energy only: the trajectory itself runs on undisturbed.
// energy_out [Lmax + 1][N][2] = {lp, ke} for l = 0 ... Lmax as computed (NaN and +-inf are results); path_out (or null)
// [Lmax][N][D]: the state after step l, centred (path_centred != 0: lane_to_centered into a temporary, the integrator's
// arithmetic is the same) or in the sampler's coordinates; p_out (or null) [N][D]: the drawn momentum.
template <class Lane>
__global__ __launch_bounds__(kBlock) void trajectory_probe_kernel(
    typename Lane::Args A, const float* __restrict__ av, const float* __restrict__ bv, const float* __restrict__ x,
    long long N, int D, int Lmax, const float* __restrict__ eps0, const float* __restrict__ kappa, uint64_t seed,
    long long row_offset, float* __restrict__ energy_out, float* __restrict__ path_out, int path_centred,
    float* __restrict__ p_out) {
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
  if (live && slot == 0) {
    energy_out[c * 2] = lp0;
    energy_out[c * 2 + 1] = ke0;
  }
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    p[i] = fmaf(0.5f * eps[i], g[i], p[i]);
    q[i] = fmaf(eps[i], p[i], q[i]);
  }
  for (int l = 1; l <= Lmax; ++l) {
    const float lp = lane_grad<kModeVIP, true>(M, q, g);
    float ke = 0.0f, keg = 0.0f;
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      const float pe = fmaf(0.5f * eps[i], g[i], p[i]);     // the closing half kick of a trajectory that ends here
      if (i < NG) keg = fmaf(pe, pe, keg); else ke = fmaf(pe, pe, ke);
    }
    ke = 0.5f * (group_sum<K>(ke) + keg);
    if (live && slot == 0) {
      float* o = energy_out + ((long long)l * N + c) * 2;
      o[0] = lp; o[1] = ke;
    }
    if (path_out) {
      float* row = path_out + ((long long)(l - 1) * N + cc) * D;
      if (path_centred) {
        float xc[ND];
        lane_to_centered<kModeVIP>(M, q, xc);
        store_row(M, row, xc, live);
      } else {
        store_row(M, row, q, live);
      }
    }
    if (l < Lmax) {
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        p[i] = fmaf(eps[i], g[i], p[i]);
        q[i] = fmaf(eps[i], p[i], q[i]);
      }
    }
  }
}

}  // namespace arp
