// The smoothed log weight of every draw (include/autoreparam.h: arp_psis_weights): the launch that follows psis_kernel
// (psis.hip) on the same rows.  A translation unit of its own, so that psis.hip's device code stays what arp_psis_loo has
// always launched; key_of and the block maximum are psis.hip's, restated (the cut-off key must be the same key).
//
// psis_kernel leaves its columns in out[n] and, for a fitted row, the M smoothed tail weights in ascending order in xs.
// What is still missing is WHICH draw takes which: the draw at position i < M of the stable ascending-ll order (ties in
// ascending draw index) takes xs[M - 1 - i], every other kept draw its raw weight llmin - ll.  psis_kernel never needs
// that (equal ll, equal weight: its sums do not depend on who is who), so it is found here, one workgroup per row:
//   raw       llmin and the non-finite flag again (min is exact: the same bits); lw = -inf for a masked draw, NaN for
//             every kept draw of a row with a non-finite kept ll, llmin - ll otherwise                      (2 reads)
//   select    psis_kernel's radix select again: the cut-off key kc and c_lt                                 (4 reads)
//   members   the tail is every key below kc and the first M - c_lt draws AT kc in draw order: thread t counts the
//             draws at kc in rows [t L, (t + 1) L), a prefix over the 256 counts gives every such draw its ordinal; the
//             members go to the workspace as 64-bit words (key << 32 | draw), in any order            (2 strided reads)
//   rank      by counting: a member's position in the stable order is the number of members whose word is smaller; the
//             words pass through LDS 2048 at a time, one member per thread and round.  M^2 comparisons, 1.5 10^8 at the
//             largest tail; integers only, so the order of the gather does not matter.
// Integer atomics for the histogram and the fill position only: two calls give bitwise equal lw.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "diag_host.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kPsThreads = 256;
constexpr int kPwChunk = 2048;

__device__ __forceinline__ unsigned key_of(float v) {
  const unsigned u = __float_as_uint(v + 0.0f);                // (-0 + 0 = +0: one key for both zeros)
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the largest of the 256 threads' values by a fixed tree through `buf`; every thread returns it
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

__global__ __launch_bounds__(kPsThreads) void psis_weights_kernel(const float* __restrict__ ll, long long R, long long stride,
                                                                  const unsigned char* __restrict__ mask,
                                                                  const double* __restrict__ out, const double* __restrict__ ws,
                                                                  unsigned long long* members, long long ws_stride,
                                                                  double* lw, long long lw_stride) {
  __shared__ double buf[kPsThreads];
  __shared__ unsigned long long chunk[kPwChunk];
  __shared__ int hist[256];
  __shared__ int seg[kPsThreads];
  __shared__ unsigned sh_prefix;
  __shared__ int sh_rank, sh_lt, sh_fill;
  const int t = threadIdx.x;
  const float* row = ll + (long long)blockIdx.x * stride;
  const double* o = out + (long long)blockIdx.x * 8;
  const double* xs = ws + (long long)blockIdx.x * ws_stride;
  unsigned long long* mem = members + (long long)blockIdx.x * ws_stride;
  double* lwr = lw + (long long)blockIdx.x * lw_stride;
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);

  // ---- raw ----
  double vmin = inf, fl_bad = 0.0;
  for (long long i = t; i < R; i += kPsThreads) {
    if (mask && mask[i]) continue;
    const float v = row[i];
    if (!(v - v == 0.0f)) fl_bad = 1.0;
    else vmin = fmin(vmin, (double)v);
  }
  const bool any_bad = block_max(fl_bad, buf) > 0.0;
  const double llmin = -block_max(-vmin, buf);
  for (long long i = t; i < R; i += kPsThreads)
    lwr[i] = (mask && mask[i]) ? -inf : any_bad ? nan : llmin - (double)row[i];
  const int Mi = (int)o[4];
  const double khat = o[1];
  if (any_bad || Mi < 5 || !(khat - khat == 0.0)) return;          // not fitted: raw weights

  // ---- select: psis_kernel's ----
  if (t == 0) { sh_prefix = 0u; sh_rank = Mi; sh_lt = 0; sh_fill = 0; }
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
    }
    __syncthreads();
    prefmask |= 255u << shift;
  }
  const unsigned kc = sh_prefix;
  const int n_tie_in = Mi - sh_lt;

  // ---- members ----
  const long long L = (R + kPsThreads - 1) / kPsThreads;
  const long long lo = min(R, (long long)t * L), hi = min(R, lo + L);
  int ties = 0;
  for (long long i = lo; i < hi; ++i)
    if (!(mask && mask[i]) && key_of(row[i]) == kc) ++ties;
  seg[t] = ties;
  __syncthreads();
  int ord = 0;
  for (int j = 0; j < t; ++j) ord += seg[j];
  for (long long i = lo; i < hi; ++i) {
    if (mask && mask[i]) continue;
    const unsigned k = key_of(row[i]);
    bool in = k < kc;
    if (k == kc) { in = ord < n_tie_in; ++ord; }
    if (in) {
      const int at = atomicAdd(&sh_fill, 1);
      if (at < Mi) mem[at] = ((unsigned long long)k << 32) | (unsigned long long)i;
    }
  }

  // ---- rank ----
  for (int m0 = 0; m0 < Mi; m0 += kPsThreads) {
    const int m = m0 + t;
    int below = 0;
    unsigned long long mine = 0ull;
    for (int c0 = 0; c0 < Mi; c0 += kPwChunk) {
      const int n = min(kPwChunk, Mi - c0);
      __syncthreads();                           // (the first also orders the members' stores before their loads)
      for (int j = t; j < n; j += kPsThreads) chunk[j] = mem[c0 + j];
      if (c0 == 0 && m < Mi) mine = mem[m];
      __syncthreads();
      if (m < Mi)
        for (int j = 0; j < n; ++j) below += chunk[j] < mine ? 1 : 0;
    }
    const long long at = (long long)(mine & 0xffffffffull);
    if (m < Mi && at < R) lwr[at] = xs[Mi - 1 - below];
  }
}

}  // namespace

int psis_weights_launch(const float* ll, long long n_obs, long long R, long long stride, const unsigned char* mask,
                        const double* out, const double* ws, unsigned long long* members, long long ws_stride, double* lw,
                        long long lw_stride, hipStream_t stream) {
  hipLaunchKernelGGL(psis_weights_kernel, dim3((unsigned)n_obs), dim3(kPsThreads), 0, stream, ll, R, stride, mask, out, ws,
                     members, ws_stride, lw, lw_stride);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace arp
