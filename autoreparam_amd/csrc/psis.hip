// Pareto-smoothed importance-sampling leave-one-out cross-validation and WAIC, one observation per workgroup
// (include/autoreparam.h: arp_psis_loo): from the pointwise log-likelihoods ll[n][r] of loglik.hip, per observation
//
//   out[n] = {elpd_loo, pareto_k, lppd, p_waic, tail_len, cutoff, gpd_sigma, draws_used}        (float64)
//
// as tests/psis_ref.py defines them (Vehtari, Gelman, Gabry 2017; Vehtari, Simpson, Gelman, Yao, Gabry 2024; the
// generalised Pareto fit of Zhang & Stephens 2009 with the prior of loo::gpdfit).  Build-specific: the reference has no
// model criticism at all.
//
// Shape of the work, for one row of R draws of which R' are kept (mask == 0):
//   pass A      R', NaN / inf flags, min and max of ll, sum of ll                                  (1 read of the row)
//   select      M = min(R' / 5, m), m^2 >= 9 R': the key of rank M in ascending ll -- the cut-off, the largest log
//               ratio NOT in the tail -- by a radix select, 8 bits a pass, on the order-preserving integer key of the
//               float32 value; with it c_lt, the number of keys below it, and c_eq, the number equal to it (4 reads)
//   gather      (M >= 5) the c_lt values below the cut-off into LDS, M - c_lt copies of the cut-off value behind
//               them, sorted there (a bitonic network whose comparators all point upwards, so that a length that is
//               no power of two needs no padding)                                                   (1 read)
//   fit         x_j = exp(lw_j) - exp(cutoff) ascending into the caller's workspace (float64, M per observation);
//               the grid of 30 + floor(sqrt(M)) profile points, one per wave at a time; weights; k, sigma
//   smooth      the j-th smallest tail weight becomes min(log(exp(cutoff) + sigma / k ((1 - p_j)^-k - 1)), 0), written
//               over x_j
//   pass E      the two log-sum-exps of elpd_loo over the draws ABOVE the cut-off key, the ties at the key by their
//               count, the tail from LDS; lppd and p_waic over all kept draws                        (1 read)
// The kernel reads the ll matrix seven times (six for a row that is not fitted) and writes 64 bytes per observation; the
// workspace traffic is 8 M bytes written and about 30 + sqrt(M) + 4 times that read back, from L2.
//
// Selection is exact for any R' <= 2^24: integer histograms (LDS integer atomics: a count does not depend on the order
// of its increments).  Only the tail goes into LDS, at most 12 288 floats.
// Ties.  A rejected transition repeats a row, so equal values are ordinary, also across the cut-off.  Equal ll means
// equal weight, so WHICH of the tied draws are in the tail changes no output: the tail is "every key below the cut-off
// key and M - c_lt copies of it", the rest of the ties enter pass E as one term times c_eq - (M - c_lt).  -0 and +0 are
// one key.
// No float atomics.  Every sum is a per-thread partial over i = t, t + 256, ... added up by a fixed tree; the order in
// which the gather fills LDS is erased by the sort.  Two calls give bitwise equal results.
//
// Arithmetic.  Everything after the float32 load is float64.  Against the float64 definition:
//   lppd    a log-sum-exp over R' terms:  |d| <= (R' + 32) 2^-53 + 4 2^-53 max|ll|
//   p_waic  two-pass variance:            |d| <= (R' + 8) 2^-52 p_waic + R' (2^-52 max|ll|)^2
// tail_len, cutoff and draws_used are exact.  pareto_k and gpd_sigma go through the profile weights
// 1 / sum_j exp(L_j - L_i) with L of the order of M, which amplify the roundings of the M-term means by about M: no
// useful a-priori bound; elpd_loo inherits that through the smoothed weights.  Float64 predicts about M^2 2^-53
// (7 10^-11 at M = 768); the measured figures are in DESIGN.md section 6 and tests/test_gpu_psis.py.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include "diag_host.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kPsThreads = 256;
constexpr int kPsWaves = kPsThreads / 64;
constexpr long long kPsMaxR = 1ll << 24;
constexpr int kPsMaxGrid = 160;                  // 30 + floor(sqrt(12 288)) = 140 profile points at the most

// min(R / 5, m), m the smallest integer with m^2 >= 9 R
__host__ __device__ inline long long tail_length(long long R) {
  long long m = (long long)sqrt((double)(9 * R));
  while (m * m < 9 * R) ++m;
  while (m > 0 && (m - 1) * (m - 1) >= 9 * R) --m;
  return R / 5 < m ? R / 5 : m;
}

__device__ __forceinline__ unsigned key_of(float v) {
  const unsigned u = __float_as_uint(v + 0.0f);                // (-0 + 0 = +0: one key for both zeros)
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Fixed-order block reductions through `buf` [256]; every thread returns the result.
__device__ __forceinline__ double block_sum(double v, double* buf) {
  const int t = threadIdx.x;
  __syncthreads();
  buf[t] = v;
  __syncthreads();
  for (int s = kPsThreads / 2; s > 0; s >>= 1) {
    if (t < s) buf[t] = buf[t] + buf[t + s];
    __syncthreads();
  }
  return buf[0];
}
__device__ __forceinline__ double block_max(double v, double* buf) {
  const int t = threadIdx.x;
  __syncthreads();
  buf[t] = v;
  __syncthreads();
  for (int s = kPsThreads / 2; s > 0; s >>= 1) {
    if (t < s) buf[t] = fmax(buf[t], buf[t + s]);
    __syncthreads();
  }
  return buf[0];
}
// a wave's sum in a fixed order (xor butterflies: every lane ends with the same bits)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void cswap(float* a, int lo, int hi) {
  const float x = a[lo], y = a[hi];
  if (y < x) { a[lo] = y; a[hi] = x; }
}

// ascending sort of a[0 .. n) in LDS: a bitonic network in the form whose comparators all put the smaller value at the
// lower index (the first step of a merge mirrors, the others are half-cleaners), so that the missing entries of a length
// that is no power of two act as +inf by being skipped
__device__ void sort_lds(float* a, int n) {
  const int t = threadIdx.x;
  int p2 = 1;
  while (p2 < n) p2 <<= 1;
  for (int k = 2; k <= p2; k <<= 1) {
    const int h = k >> 1;
    __syncthreads();
    for (int i = t; i < p2 / 2; i += kPsThreads) {
      const int blk = i / h, off = i - blk * h;
      const int lo = blk * k + off, hi = blk * k + k - 1 - off;
      if (hi < n) cswap(a, lo, hi);
    }
    for (int j = h >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = t; i < p2 / 2; i += kPsThreads) {
        const int lo = 2 * j * (i / j) + (i % j), hi = lo + j;
        if (hi < n) cswap(a, lo, hi);
      }
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kPsThreads) void psis_kernel(const float* __restrict__ ll, long long R, long long stride,
                                                          const unsigned char* __restrict__ mask, double* __restrict__ out,
                                                          double* ws, long long ws_stride) {
  extern __shared__ float tail[];                // the M smallest ll of the row, ascending after the sort
  __shared__ double buf[kPsThreads];
  __shared__ double gb[kPsMaxGrid], gk[kPsMaxGrid], gL[kPsMaxGrid], gw[kPsMaxGrid];
  __shared__ int hist[256];
  __shared__ unsigned sh_prefix;
  __shared__ int sh_rank, sh_lt, sh_eq, sh_fill;
  __shared__ double sh_fit[2];
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const float* row = ll + (long long)blockIdx.x * stride;
  double* o = out + (long long)blockIdx.x * 8;
  double* xs = ws + (long long)blockIdx.x * ws_stride;
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);

  // ---- pass A ----
  double cnt = 0.0, sum = 0.0, vmin = inf, vmax = -inf, fl_nan = 0.0, fl_inf = 0.0;
  for (long long i = t; i < R; i += kPsThreads) {
    if (mask && mask[i]) continue;
    const float v = row[i];
    cnt += 1.0;
    if (v != v) fl_nan = 1.0;
    else if (!(v - v == 0.0f)) fl_inf = 1.0;
    else { sum += (double)v; vmin = fmin(vmin, (double)v); vmax = fmax(vmax, (double)v); }
  }
  const long long Rk = (long long)block_sum(cnt, buf);                 // (counts below 2^53 are exact in float64)
  const bool any_nan = block_max(fl_nan, buf) > 0.0, any_inf = block_max(fl_inf, buf) > 0.0;
  if (Rk == 0) {
    if (t == 0) { o[0] = nan; o[1] = inf; o[2] = nan; o[3] = nan; o[4] = 0.0; o[5] = nan; o[6] = nan; o[7] = 0.0; }
    return;
  }
  const long long M = tail_length(Rk);
  if (any_nan || any_inf) {
    if (t == 0) {
      o[0] = any_nan ? nan : -inf; o[1] = inf; o[2] = nan; o[3] = nan; o[4] = (double)M; o[5] = nan; o[6] = nan;
      o[7] = (double)Rk;
    }
    return;
  }
  const double total = block_sum(sum, buf);
  const double mean = total / (double)Rk;
  const double llmin = -block_max(-vmin, buf), llmax = block_max(vmax, buf);

  // ---- select: the key of rank M (0-based) among the kept draws in ascending order ----
  if (t == 0) { sh_prefix = 0u; sh_rank = (int)M; sh_lt = 0; sh_eq = 0; }
  unsigned prefmask = 0u;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[t] = 0;
    __syncthreads();
    const unsigned prefix = sh_prefix;
    for (long long i = t; i < R; i += kPsThreads) {
      if (mask && mask[i]) continue;
      const unsigned k = key_of(row[i]);
      if (((k ^ prefix) & prefmask) == 0u) atomicAdd(&hist[(k >> shift) & 255u], 1);
    }
    __syncthreads();
    if (t == 0) {
      int cum = 0, b = 0;
      const int rank = sh_rank;
      while (b < 255 && cum + hist[b] <= rank) { cum += hist[b]; ++b; }
      sh_lt += cum;
      sh_rank = rank - cum;
      sh_prefix = prefix | ((unsigned)b << shift);
      sh_eq = hist[b];
    }
    __syncthreads();
    prefmask |= 255u << shift;
  }
  const unsigned kc = sh_prefix;
  const int c_lt = sh_lt, c_eq = sh_eq;
  const int n_tie_in = (int)M - c_lt;            // copies of the cut-off value inside the tail, < c_eq
  const float vc = value_of(kc);
  const double cutoff = llmin - (double)vc;      // lw = -ll - max(-ll) = llmin - ll, exact where the reference's is

  // ---- gather, sort, fit, smooth ----
  bool fitted = false;
  double khat = inf, sigma = nan;
  const int Mi = (int)M;
  if (Mi >= 5) {
    if (t == 0) sh_fill = 0;
    __syncthreads();
    for (long long i = t; i < R; i += kPsThreads) {
      if (mask && mask[i]) continue;
      const float v = row[i];
      if (key_of(v) < kc) {                      // (c_lt <= M of them; the sort erases the order)
        const int at = atomicAdd(&sh_fill, 1);
        if (at < Mi) tail[at] = v;
      }
    }
    for (int i = c_lt + t; i < Mi; i += kPsThreads) tail[i] = vc;
    sort_lds(tail, Mi);
    // ascending exceedances: x_j, j = 0 ... M - 1, from the descending end of the sorted ll
    const double ec = exp(cutoff);
    for (int j = t; j < Mi; j += kPsThreads) xs[j] = exp(llmin - (double)tail[Mi - 1 - j]) - ec;
    __syncthreads();
    int rt = (int)sqrt((double)Mi);
    while (rt * rt > Mi) --rt;
    while ((rt + 1) * (rt + 1) <= Mi) ++rt;
    const int mg = 30 + rt;
    const double xM = xs[Mi - 1], xq = xs[(int)floor((double)Mi / 4.0 + 0.5) - 1];
    for (int i0 = 0; i0 < mg; i0 += kPsWaves) {
      const int i = i0 + wave;                   // one profile point per wave
      if (i < mg) {
        const double b = 1.0 / xM + (1.0 - sqrt((double)mg / ((double)(i + 1) - 0.5))) / (3.0 * xq);
        double s = 0.0;
        for (int j = lane; j < Mi; j += 64) s += log1p(-b * xs[j]);
        s = wave_sum(s);
        if (lane == 0) {
          const double k = s / (double)Mi;
          gb[i] = b;
          gk[i] = k;
          gL[i] = (double)Mi * (log(-b / k) - k - 1.0);
        }
      }
    }
    __syncthreads();
    if (t < mg) {
      double s = 0.0;
      const double Li = gL[t];
      for (int j = 0; j < mg; ++j) s += exp(gL[j] - Li);
      gw[t] = 1.0 / s;
    }
    __syncthreads();
    if (t == 0) {
      double sw = 0.0, bb = 0.0;
      for (int i = 0; i < mg; ++i) sw += gw[i];
      for (int i = 0; i < mg; ++i) bb += gb[i] * (gw[i] / sw);
      sh_fit[0] = bb;
    }
    __syncthreads();
    const double bb = sh_fit[0];
    double s = 0.0;
    for (int j = t; j < Mi; j += kPsThreads) s += log1p(-bb * xs[j]);
    const double kk = block_sum(s, buf) / (double)Mi;
    sigma = -kk / bb;
    khat = ((double)Mi * kk + 5.0) / ((double)Mi + 10.0);
    fitted = (khat - khat == 0.0) && (sigma - sigma == 0.0);
    if (!fitted) { khat = inf; sigma = nan; }
    if (fitted) {
      // the j-th smallest tail weight, j = 0 ... M - 1, over x_j (its ll is tail[M - 1 - j])
      for (int j = t; j < Mi; j += kPsThreads) {
        const double p = ((double)(j + 1) - 0.5) / (double)Mi;
        const double q = khat == 0.0 ? -sigma * log1p(-p) : sigma * expm1(-khat * log1p(-p)) / khat;
        xs[j] = fmin(log(ec + q), 0.0);
      }
      __syncthreads();
    }
  }

  // ---- pass E ----
  // shifts of the two log-sum-exps: any value near the largest term does
  double m1 = llmin, m2 = cutoff;
  if (fitted) {
    double a1 = -inf, a2 = -inf;
    for (int j = t; j < Mi; j += kPsThreads) {
      a1 = fmax(a1, xs[j] + (double)tail[Mi - 1 - j]);
      a2 = fmax(a2, xs[j]);
    }
    m1 = fmax(m1, block_max(a1, buf));
    m2 = fmax(m2, block_max(a2, buf));
  } else {
    m2 = 0.0;                                    // raw weights: the largest is 0
  }
  double s1 = 0.0, s2 = 0.0, sl = 0.0, ss = 0.0;
  for (long long i = t; i < R; i += kPsThreads) {
    if (mask && mask[i]) continue;
    const float v = row[i];
    const double d = (double)v;
    sl += exp(d - llmax);
    ss += (d - mean) * (d - mean);
    if (fitted && key_of(v) <= kc) continue;     // the tail, and the ties at the cut-off: below
    const double lw = llmin - d;
    s1 += exp((lw + d) - m1);
    s2 += exp(lw - m2);
  }
  if (fitted) {
    for (int j = t; j < Mi; j += kPsThreads) {
      s1 += exp((xs[j] + (double)tail[Mi - 1 - j]) - m1);
      s2 += exp(xs[j] - m2);
    }
    if (t == 0) {                                // the ties at the cut-off that stayed outside the tail, by count
      const double d = (double)vc, n_out = (double)(c_eq - n_tie_in);
      s1 += n_out * exp((cutoff + d) - m1);
      s2 += n_out * exp(cutoff - m2);
    }
  }
  const double S1 = block_sum(s1, buf), S2 = block_sum(s2, buf), SL = block_sum(sl, buf), SS = block_sum(ss, buf);
  if (t == 0) {
    o[0] = (m1 + log(S1)) - (m2 + log(S2));
    o[1] = khat;
    o[2] = (llmax + log(SL)) - log((double)Rk);
    o[3] = Rk > 1 ? SS / (double)(Rk - 1) : nan;
    o[4] = (double)M;
    o[5] = cutoff;
    o[6] = sigma;
    o[7] = (double)Rk;
  }
}

bool psis_shape_ok(int64_t n_obs, int64_t n_draws) {
  return n_obs >= 1 && n_obs < (1ll << 31) && n_draws >= 1 && n_draws <= kPsMaxR;
}

// doubles per observation in the workspace: the tail of a row without a masked draw, rounded up to 256 bytes
long long ws_stride_of(int64_t n_draws) { return (tail_length(n_draws) + 31) / 32 * 32; }

}  // namespace

// psis_weights.hip: the second launch of arp_psis_weights (kept out of this file so that psis_kernel's code object is
// the one arp_psis_loo has always launched, instruction for instruction: tools/listing_diff.py)
int psis_weights_launch(const float* ll, long long n_obs, long long R, long long stride, const unsigned char* mask,
                        const double* out, const double* ws, unsigned long long* members, long long ws_stride, double* lw,
                        long long lw_stride, hipStream_t stream);

}  // namespace arp

extern "C" int64_t arp_psis_workspace_bytes(int64_t n_obs, int64_t n_draws) {
  using namespace arp;
  if (!psis_shape_ok(n_obs, n_draws)) return 0;
  return align256(std::max<long long>(32, n_obs * ws_stride_of(n_draws)) * 8);
}

extern "C" int arp_psis_loo(const float* ll, int64_t n_obs, int64_t n_draws, int64_t ll_stride, const uint8_t* mask,
                            double* out, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace arp;
  const char* who = "arp_psis_loo";
  if (!ll || !out) { set_error(std::string(who) + ": ll and out are required"); return 1; }
  if (n_obs < 1 || n_obs >= (1ll << 31) || n_draws < 1) {
    set_error(std::string(who) + ": 1 <= n_obs < 2^31 and n_draws >= 1 are required");
    return 1;
  }
  if (n_draws > kPsMaxR) { set_error(std::string(who) + ": at most 2^24 draws per observation"); return 1; }
  if (ll_stride < n_draws) { set_error(std::string(who) + ": ll_stride >= n_draws is required"); return 1; }
  const int64_t need = arp_psis_workspace_bytes(n_obs, n_draws);
  if (!workspace_size_ok(workspace && workspace_bytes >= need, who, "see arp_psis_workspace_bytes")) return 1;
  if (!workspace_aligned(workspace, who)) return 1;
  const size_t lds = (size_t)std::max<long long>(1, tail_length(n_draws)) * sizeof(float);
  hipLaunchKernelGGL(psis_kernel, dim3((unsigned)n_obs), dim3(kPsThreads), lds, (hipStream_t)stream, ll, (long long)n_draws,
                     (long long)ll_stride, (const unsigned char*)mask, out, (double*)workspace, ws_stride_of(n_draws));
  ARP_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int64_t arp_psis_weights_workspace_bytes(int64_t n_obs, int64_t n_draws) {
  using namespace arp;
  if (!psis_shape_ok(n_obs, n_draws)) return 0;
  Carve c;
  c.take(arp_psis_workspace_bytes(n_obs, n_draws));
  c.take(n_obs * ws_stride_of(n_draws) * 8);
  return c.bytes();
}

extern "C" int arp_psis_weights(const float* ll, int64_t n_obs, int64_t n_draws, int64_t ll_stride, const uint8_t* mask,
                                double* out, double* lw, int64_t lw_stride, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  using namespace arp;
  const char* who = "arp_psis_weights";
  if (!ll || !out || !lw) { set_error(std::string(who) + ": ll, out and lw are required"); return 1; }
  if (n_obs < 1 || n_obs >= (1ll << 31) || n_draws < 1) {
    set_error(std::string(who) + ": 1 <= n_obs < 2^31 and n_draws >= 1 are required");
    return 1;
  }
  if (n_draws > kPsMaxR) { set_error(std::string(who) + ": at most 2^24 draws per observation"); return 1; }
  if (ll_stride < n_draws) { set_error(std::string(who) + ": ll_stride >= n_draws is required"); return 1; }
  if (lw_stride < n_draws) { set_error(std::string(who) + ": lw_stride >= n_draws is required"); return 1; }
  const int64_t need = arp_psis_weights_workspace_bytes(n_obs, n_draws);
  if (!workspace_size_ok(workspace && workspace_bytes >= need, who, "see arp_psis_weights_workspace_bytes")) return 1;
  if (!workspace_aligned(workspace, who)) return 1;
  Carve c;
  double* xs = (double*)((char*)workspace + c.take(arp_psis_workspace_bytes(n_obs, n_draws)));
  unsigned long long* members = (unsigned long long*)((char*)workspace + c.take(n_obs * ws_stride_of(n_draws) * 8));
  // the launch of arp_psis_loo, argument for argument: out is its out
  const size_t lds = (size_t)std::max<long long>(1, tail_length(n_draws)) * sizeof(float);
  hipLaunchKernelGGL(psis_kernel, dim3((unsigned)n_obs), dim3(kPsThreads), lds, (hipStream_t)stream, ll, (long long)n_draws,
                     (long long)ll_stride, (const unsigned char*)mask, out, xs, ws_stride_of(n_draws));
  ARP_HIP_OK(hipGetLastError());
  return psis_weights_launch(ll, (long long)n_obs, (long long)n_draws, (long long)ll_stride, (const unsigned char*)mask, out, xs,
                             members, ws_stride_of(n_draws), lw, (long long)lw_stride, (hipStream_t)stream);
}
