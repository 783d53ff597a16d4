// Leave-one-out predictive sums (include/autoreparam.h: arp_loo_predictive): the per-(observation, draw) predictive
// quantities of ppc.hip -- the mean mu and the variance var of y_rep given the draw, and the PIT value of the observed y --
// folded over the draws WITH the importance weights of arp_psis_weights, W = exp(lw[n][r]):
//
//   obs_sums[n][6] = { sum W, sum W^2, sum W mu, sum W (mu^2 + var), sum W pit, draws counted }    over the draws with lw != -inf
//
// from which the host forms the LOO predictive mean and sd, the LOO-PIT and the importance-sampling ESS of every
// observation (diagnostics.loo_predictive_summary; Vehtari, Gelman, Gabry 2017 section 2; loo::E_loo, loo::loo_pit).
// Model-independent; the table, the tile of draws, eta_n and s_n, and mu, var and pit of the two kinds of data are
// obs_table.h's, the very functions ppc.hip calls.
//
// Build-specific: the reference has no predictive reports.  The kernel does not care where lw came from.
//
// Shape of the work: obs_table.h's, with ppc.hip's "along the draws" direction and nothing else.  lw is read coalesced
// along r, one 8-byte load per (n, r), asked for one observation ahead.  Per (n, tile) an xor butterfly on doubles
// over the 64 lanes (wave_sum below: lane permutations in registers, no LDS; every lane ends with the same bits) gives the
// tile's five sums, the count is a ballot, lane 0 stores the six to the workspace [tile][n][6], and a second launch adds
// the tiles in ascending order (loopred_fold: the loads staged through LDS, the additions of one (n, c) a chain).
// No float atomics: two calls give bitwise equal output; the partial of (n, tile) depends on neither blockIdx.y nor
// [n0, n1), so a split observation range gives the same bits.
//
// Cost, next to ppc.hip per (n, r): no Philox call, no logf / sqrtf / cospif and no deviance; one 8-byte load and one
// float64 exp more; five float64 butterflies per (n, tile) instead of three.  Measured, with what each of the three
// choices above (the load ahead, the butterfly in registers, the staged second launch) was worth: DESIGN.md section 6.
//
// Arithmetic.  eta, s, mu, m2 = mu^2 + var and pit are float32, contraction off, and obs_table.h's: the first-order
// bounds b_h of h = mu, m2 and pit are those derived in ppc.hip.
// W = exp(lw) is ONE float64 exp of the float64 input (the device library's, good to about an ulp, 2^-52 relative);
// W^2 and W h (h the float32 value taken to float64) are one float64 product each, and every sum is a float64 sum in a
// fixed order: a column sum_r W h is off by at most sum_r W b_h plus a few 2^-52 (terms + 1) sum_r W |h|.
// Second-order terms are left out; the tests allow twice the first-order figures, as they do for ppc.hip.
//
// Things that go wrong quietly here:
//  * A draw with lw = -inf (arp_psis_weights' mark of a masked draw) enters nothing, by select -- never a product with
//    W = 0: its state may hold an inf or a NaN, and 0 * inf is NaN.  It is not counted.
//  * A NaN lw is NOT such a draw: it enters, is counted, and makes the observation's five float columns NaN.  Nothing is
//    skipped silently.  A draw whose state is non-finite while its lw is finite carries through the same way.
//  * Dead lanes of the last ragged tile take part in every shuffle and in the ballot (the butterfly needs all 64) with 0
//    by select; their lw is never loaded.
//  * Reads past the end, the table's indices: obs_table.h.  lw is read at (n - n0) * lw_stride + r for n0 <= n < n1, r < R only.
#include "obs_table.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kLpCols = 6;                       // columns of obs_sums
constexpr int kLpFoldOut = 32;                   // the second launch: (n, c) per workgroup ...
constexpr int kLpFoldTiles = 64;                 // ... and tiles staged at a time: 16 KB of LDS

// v of the lane this lane is paired with by the data-parallel-primitive control `Ctrl` (a permutation within a row of 16)
template <int Ctrl>
__device__ __forceinline__ double row_partner(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), Ctrl, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), Ctrl, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// The sum over the 64 lanes; every lane ends with the same bits.  An xor butterfly, lane i with lane i ^ m for m = 1, 2, 7,
// 15, 16, 32: within a row of 16 through the DPP lane permutations (quad_perm [1,0,3,2] and [2,3,0,1], row_half_mirror,
// row_mirror -- i ^ 7 and i ^ 15 pair a lane with the other half of its group just as i ^ 4 and i ^ 8 would), across rows
// through gfx950's row and half-wave swaps: with both operands v, v_permlane16_swap leaves rows {0, 0, 2, 2} in the first and
// {1, 1, 3, 3} in the second, v_permlane32_swap the lower half twice and the upper half twice.  Every step adds the same two
// values in every lane (a + b and b + a are the same bits), and none goes through LDS: __shfl_xor is a ds_bpermute_b32 per
// dword, twelve per sum and sixty per (n, tile), and without them the launch is a seventh shorter at election's shape
// (DESIGN.md section 6).
__device__ __forceinline__ double wave_sum(double v) {
  v += row_partner<0xB1>(v);                     // quad_perm [1, 0, 3, 2]: i ^ 1
  v += row_partner<0x4E>(v);                     // quad_perm [2, 3, 0, 1]: i ^ 2
  v += row_partner<0x141>(v);                    // row_half_mirror: i ^ 7
  v += row_partner<0x140>(v);                    // row_mirror: i ^ 15
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  v = __hiloint2double((int)h16[0], (int)l16[0]) + __hiloint2double((int)h16[1], (int)l16[1]);          // i ^ 16
  const unsigned lo2 = (unsigned)__double2loint(v), hi2 = (unsigned)__double2hiint(v);
  const auto l32 = __builtin_amdgcn_permlane32_swap(lo2, lo2, false, false);
  const auto h32 = __builtin_amdgcn_permlane32_swap(hi2, hi2, false, false);
  return __hiloint2double((int)h32[0], (int)l32[0]) + __hiloint2double((int)h32[1], (int)l32[1]);      // i ^ 32
}

__global__ __launch_bounds__(kObsThreads) void loopred_kernel(
    const float* __restrict__ x, long long R, unsigned n_chains, int D, long long stride, int kind, int T,
    const int* __restrict__ idx, const float* __restrict__ w, const float* __restrict__ y,
    const int* __restrict__ scale_idx, const float* __restrict__ log_scale, long long n0, long long n1, long long per_group,
    const double* __restrict__ lw, long long lw_stride, double* __restrict__ part) {
  extern __shared__ float tile[];                // [64][D | 1]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long r0 = (long long)blockIdx.x * kObsDraws;
  const int nrows = (int)min((long long)kObsDraws, R - r0);
  stage_tile<false>(x, r0, nrows, n_chains, D, stride, tile, nullptr);
  const bool live = lane < nrows;
  const double ninf = -__longlong_as_double(0x7ff0000000000000ll);

  const float* row = tile + lane * (D | 1);
  const long long nb = n0 + (long long)blockIdx.y * per_group, ne = min(n1, nb + per_group);
  // the log weight of the NEXT observation is asked for before this one's arithmetic: the load's latency (the only
  // per-lane global load of the loop) is then hidden behind a whole iteration and not paid in front of the exp
  double l_next = ninf;
  if (live && nb + wave < ne) l_next = lw[(nb + wave - n0) * lw_stride + r0 + lane];
  for (long long n = nb + wave; n < ne; n += kObsWaves) {
    const double l = l_next;                     // (a dead lane holds -inf)
    l_next = ninf;
    if (live && n + kObsWaves < ne) l_next = lw[(n + kObsWaves - n0) * lw_stride + r0 + lane];
    const float eta = obs_eta(row, idx, w, n, T, D);
    const float yn = y[n];
    PredTerms pt;
    if (kind == 0) {
      const float s = obs_log_scale(row, scale_idx, log_scale, n, D);
      pt = normal_terms(eta, yn, expf(s), expf(-s));
    } else {
      pt = bernoulli_terms(eta, yn);
    }
    const bool in = l != ninf;                   // (a NaN enters)
    const double W = exp(l);
    // every lane takes part, one that does not count with 0 by select
    const double s_w = wave_sum(in ? W : 0.0);
    const double s_ww = wave_sum(in ? W * W : 0.0);
    const double s_mu = wave_sum(in ? W * (double)pt.mu : 0.0);
    const double s_m2 = wave_sum(in ? W * (double)pt.m2 : 0.0);
    const double s_pit = wave_sum(in ? W * (double)pt.pit : 0.0);
    const unsigned long long counted = __ballot(in);
    if (lane == 0) {
      double* po = part + ((long long)blockIdx.x * (n1 - n0) + (n - n0)) * kLpCols;
      po[0] = s_w; po[1] = s_ww; po[2] = s_mu; po[3] = s_m2; po[4] = s_pit; po[5] = (double)__popcll(counted);
    }
  }
}

// obs_sums[n][c] over the tiles in ascending order.  The order makes the additions of one (n, c) a chain, but not its
// loads: a workgroup takes kLpFoldOut adjacent (n, c) and stages kLpFoldTiles tiles of them in LDS at a time, every thread
// with its loads in flight together (rows of 256 contiguous bytes), and thread j < kLpFoldOut then adds column j in order.
// (One thread per (n, c) walking the tiles by itself, ppc.hip's third launch, waits for memory once per tile: at 1 024 tiles
// and 2 046 (n, c) that was about 0.19 ms a call whatever the first launch took)
__global__ __launch_bounds__(kObsThreads) void loopred_fold(const double* __restrict__ part, long long total, long long ntiles,
                                                           double* __restrict__ obs_sums) {
  __shared__ double stage[kLpFoldTiles][kLpFoldOut];
  const int t = threadIdx.x;
  const int col = t % kLpFoldOut, row0 = t / kLpFoldOut;
  const long long i = (long long)blockIdx.x * kLpFoldOut + col;
  double acc = 0.0;
  for (long long t0 = 0; t0 < ntiles; t0 += kLpFoldTiles) {
    const int nt = (int)min((long long)kLpFoldTiles, ntiles - t0);
    __syncthreads();                             // (the chunk before this one has been added)
#pragma unroll
    for (int r = row0; r < kLpFoldTiles; r += kObsThreads / kLpFoldOut)
      if (r < nt && i < total) stage[r][col] = part[(t0 + r) * total + i];
    __syncthreads();
    if (t < kLpFoldOut && i < total) {
      int r = 0;
      if (t0 == 0) acc = stage[r++][col];        // (the first tile as it is: no 0 + x)
      for (; r < nt; ++r) acc += stage[r][col];
    }
  }
  if (t < kLpFoldOut && i < total) obs_sums[i] = acc;
}

}  // namespace
}  // namespace arp

extern "C" int64_t arp_loo_predictive_workspace_bytes(int64_t n_obs, int64_t n_draws) {
  using namespace arp;
  if (!obs_shape_ok(n_obs, n_draws)) return 0;
  Carve c;
  c.take(split_of(n_obs, n_draws).ntiles * n_obs * kLpCols * (int64_t)sizeof(double));
  return c.bytes();
}

extern "C" int arp_loo_predictive(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                                  int32_t kind, const int32_t* idx, const float* w, int32_t T, const float* y,
                                  const int32_t* scale_idx, const float* log_scale, int64_t n0, int64_t n1, const double* lw,
                                  int64_t lw_stride, double* obs_sums, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace arp;
  const char* name = "arp_loo_predictive";
  const std::string who = name;
  if (!x || !idx || !w || !y || !scale_idx || !log_scale || !lw || !obs_sums) {
    set_error(who + ": x, the table (idx, w, y, scale_idx, log_scale), lw and obs_sums are required");
    return 1;
  }
  if (!table_call_ok(name, n_samples, n_chains, D, row_stride, kind, T, n0, n1)) return 1;
  const long long R = n_samples * n_chains;
  if (lw_stride < R) { set_error(who + ": lw_stride >= n_samples * n_chains is required"); return 1; }
  const long long nobs = n1 - n0;
  const int64_t need = arp_loo_predictive_workspace_bytes(nobs, R);
  if (!workspace_size_ok(need > 0 && workspace && workspace_bytes >= need, name, "see arp_loo_predictive_workspace_bytes")) return 1;
  if (!workspace_aligned(workspace, name)) return 1;
  const Split sp = split_of(nobs, R);
  double* part = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(loopred_kernel, dim3((unsigned)sp.ntiles, (unsigned)sp.groups), dim3(kObsThreads), tile_lds_bytes(D), st, x, R,
                     (unsigned)n_chains, (int)D, (long long)row_stride, (int)kind, (int)T, idx, w, y, scale_idx, log_scale, (long long)n0, (long long)n1,
                     sp.per_group, lw, (long long)lw_stride, part);
  ARP_HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(loopred_fold, dim3(blocks_for(nobs * kLpCols, kLpFoldOut)), dim3(kObsThreads), 0, st, (const double*)part,
                     nobs * kLpCols, sp.ntiles, obs_sums);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
