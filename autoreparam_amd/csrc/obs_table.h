// What the kernels over a model's observation table share (loglik.hip, ppc.hip, loopred.hip; the table:
// autoreparam_amd/models.py: ModelSpec.observation_table): the tile of draws, the linear predictor and the scale of an
// observation, the predictive terms of the two data kinds, and on the host the split of the observations, the size of the
// tile and the refusals every such entry point makes.  Every model with data here is Normal or Bernoulli-logit over a
// linear predictor of the centred latents,
//
//   eta_n = sum_t w[n][t] x[idx[n][t]],   s_n = log_scale[n] + (scale_idx[n] >= 0 ? x[scale_idx[n]] : 0)
//
// Shape of the work.  Draws lie across the lanes of a wave and the observation is uniform per wave, so idx, w, y and the
// scale entries are wave-uniform (scalar) loads.  A workgroup of four waves stages ONE tile of 64 draws -- all D elements
// of each, read coalesced from the trace in place -- in LDS with an odd row pitch (lane l reads x[l][idx]: ds_read_b32
// banks by (l Dp + idx) mod 32 within a half-wave, 32 different banks whatever idx is), and its waves then walk the
// observations of the workgroup's share (blockIdx.y), wave v taking every fourth.
//
// The table pointers are separate __restrict__ kernel arguments and reach the helpers below as separate pointers: that is
// what lets the compiler load idx and w through the scalar unit (handed over in a struct they became per-lane vector loads).
//
// Arithmetic.  float32 throughout, contraction off: eta is the chain eta <- eta + w_t x_t over t = 0 ... T - 1 in that
// order, every product and every sum rounded once; s is a table entry rounded to float32 and one addition.  With
// u = 2^-24 and A = sum_t |w_t x_t|, to first order against the exact value of the same float32 inputs
//
//   |eta_dev - eta| <= T u A
//
// The bounds of what a kernel makes of eta and s stand in its own file; those of the predictive terms in ppc.hip.
//
// Things that go wrong quietly here:
//  * Reads past the end.  A load is issued for (r < n_samples * n_chains, d < D) only; nothing is read past
//    x[(n_samples - 1) * row_stride + n_chains * D - 1].  Dead rows of the tile hold 0 and are never stored.
//  * The table.  idx and scale_idx are clamped into [0, D) before they address the tile; the caller's checks
//    (diagnostics.upload_table) keep them there in the first place.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "diag_host.h"

#pragma clang fp contract(off)

namespace arp {

constexpr int kObsThreads = 256;
constexpr int kObsWaves = kObsThreads / 64;
constexpr int kObsDraws = 64;                    // draws per tile: one per lane
constexpr int kObsMaxD = 255;                    // 64 rows of pitch 255 floats: 65 280 bytes of LDS
constexpr int kObsMaxT = 4096;
constexpr long long kObsTargetWorkgroups = 2048;
constexpr float kNegInvSqrt2F = -0.7071067811865476f;

// The workgroup's tile [64][D | 1] of the draws r0 ... r0 + nrows - 1, barriers included.  Flag: bad[lr] (LDS, 64 ints) is
// set for a row with a non-finite element; it is not touched otherwise.
template <bool Flag>
__device__ __forceinline__ void stage_tile(const float* x, long long r0, int nrows, unsigned n_chains, int D, long long stride,
                                           float* tile, int* bad) {
  const int t = threadIdx.x;
  const int Dp = D | 1;
  if (Flag) {
    if (t < kObsDraws) bad[t] = 0;
    __syncthreads();
  }
  // element e = t + 256 a of the tile is (row e / D, column e % D); a dead row takes 0 without a load
  const int nelem = kObsDraws * D;
  for (int e = t; e < nelem; e += kObsThreads) {
    const int lr = (int)((unsigned)e / (unsigned)D), d = e - lr * D;
    float v = 0.0f;
    if (lr < nrows) {
      const unsigned r = (unsigned)(r0 + lr);
      const unsigned step = r / n_chains, chain = r - step * n_chains;
      v = x[(long long)step * stride + (long long)chain * D + d];
      if (Flag && !(v - v == 0.0f)) bad[lr] = 1;
    }
    tile[lr * Dp + d] = v;
  }
  __syncthreads();
}

// mask[r] of the tile's live draws and their count; once per tile, so the caller asks blockIdx.y == 0, wave 0 only.
// (The two flags by reference: the caller's own variables, as when these lines stood in the kernel.  By value the compiler
// forms the ballot's operand another way, one instruction shorter, and every loop behind it sits at another address:
// arp_pointwise_loglik then measured 1 % slower at T = 2 and T = 3, NOTES_r07.md.)
__device__ __forceinline__ void write_mask(const bool& live, const bool& bad, int lane, long long r0, unsigned char* mask,
                                           unsigned long long* n_masked) {
  if (live) mask[r0 + lane] = bad ? 1 : 0;
  const unsigned long long b = __ballot(live && bad);
  if (lane == 0 && b != 0) atomicAdd(n_masked, (unsigned long long)__popcll(b));      // (an integer count: order-free)
}

// eta of observation n from this lane's row of the tile
__device__ __forceinline__ float obs_eta(const float* row, const int* idx, const float* w, long long n, int T, int D) {
  const int* ip = idx + n * T;
  const float* wp = w + n * T;
  float eta = 0.0f;
#pragma unroll 4
  for (int k = 0; k < T; ++k) {
    const int i = min(max(ip[k], 0), D - 1);
    eta = eta + wp[k] * row[i];
  }
  return eta;
}

// s of observation n (Normal data)
__device__ __forceinline__ float obs_log_scale(const float* row, const int* scale_idx, const float* log_scale, long long n, int D) {
  const int si = scale_idx[n];
  float s = log_scale[n];
  if (si >= 0) s = s + row[min(si, D - 1)];
  return s;
}

// The predictive terms of (observation, draw): the mean mu of y_rep, its second moment m2 = mu^2 + var, the PIT value of
// the observed y -- and aux, what ppc.hip's deviance goes on from: z_obs (Normal), e = exp(-|eta|) (Bernoulli; mu is p).
struct PredTerms { float mu, m2, pit, aux; };
//   Normal:     mu = eta, var = exp(s)^2;  z_obs = (y - eta) exp(-s);  pit = 0.5 erfc(-z_obs / sqrt 2)
__device__ __forceinline__ PredTerms normal_terms(float eta, float y, float es, float ems) {
  PredTerms p;
  p.aux = (y - eta) * ems;
  p.pit = 0.5f * erfcf(p.aux * kNegInvSqrt2F);
  p.mu = eta;
  p.m2 = eta * eta + es * es;
  return p;
}
//   Bernoulli:  e = exp(-|eta|), p = (eta >= 0 ? 1 : e) / (1 + e);  mu = p, var = p (1 - p);
//               pit = y > 0.5 ? 1 - p / 2 : (1 - p) / 2 (the mid-p value)
__device__ __forceinline__ PredTerms bernoulli_terms(float eta, float y) {
  PredTerms p;
  p.aux = expf(-fabsf(eta));
  p.mu = (eta >= 0.0f ? 1.0f : p.aux) / (1.0f + p.aux);
  p.pit = y > 0.5f ? 1.0f - 0.5f * p.mu : 0.5f * (1.0f - p.mu);
  p.m2 = p.mu * p.mu + p.mu * (1.0f - p.mu);
  return p;
}

// ---- host ----
// The one launch rule, gridDim.y of `ntiles` tiles over `units` (observations, or groups of them: group_table.h): enough
// workgroups to fill the device at few tiles; never more waves than units
inline long long shares_of(long long ntiles, long long units) {
  const long long shares = std::max<long long>(1, (kObsTargetWorkgroups + ntiles - 1) / ntiles);
  return std::min<long long>(std::min<long long>(shares, (units + kObsWaves - 1) / kObsWaves), 65535);
}

// how the observations [n0, n1) are shared among blockIdx.y, and the tiles of R draws
struct Split { long long ntiles, groups, per_group; };
inline Split split_of(long long nobs, long long R) {
  Split s;
  s.ntiles = (R + kObsDraws - 1) / kObsDraws;
  const long long groups = shares_of(s.ntiles, nobs);
  s.per_group = (nobs + groups - 1) / groups;
  s.groups = (nobs + s.per_group - 1) / s.per_group;
  return s;
}
inline size_t tile_lds_bytes(int D) { return (size_t)kObsDraws * (D | 1) * sizeof(float); }

// the shapes a workspace is sized for
inline bool obs_shape_ok(int64_t n_obs, int64_t n_draws) {
  return n_obs >= 1 && n_obs < (1ll << 31) && n_draws >= 1 && n_draws < (1ll << 31);
}

// The refusals every entry point over the table makes, behind its own test for null pointers
inline bool table_call_ok(const char* name, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride, int32_t kind,
                          int32_t T, int64_t n0, int64_t n1) {
  const char* rule = nullptr;
  if (D < 1 || D > kObsMaxD) rule = ": 1 <= D <= 255 is required";
  else if (!trace_shape_ok(n_samples, n_chains, D, name)) return false;
  else if (row_stride < n_chains * D) rule = ": row_stride >= n_chains * D is required";
  else if (kind != 0 && kind != 1) rule = ": kind must be ARP_OBS_NORMAL or ARP_OBS_BERNOULLI";
  else if (T < 1 || T > kObsMaxT) rule = ": 1 <= T <= 4096 is required";
  else if (n0 < 0 || n1 <= n0 || n1 >= (1ll << 31)) rule = ": 0 <= n0 < n1 < 2^31 is required";
  if (rule) set_error(std::string(name) + rule);
  return !rule;
}

}  // namespace arp
