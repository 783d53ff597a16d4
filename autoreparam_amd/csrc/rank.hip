// Rank normalisation of a recorded trace (include/autoreparam.h: arp_rank_normalize): the average rank of every draw
// within its element's pooled draws, as a normal score, and order statistics of the pool (median, quantiles) -- what the
// rank-normalised, folded split R-hat of Vehtari et al. 2021 needs below the moments kernels of diag.hip
// (autoreparam_amd/diagnostics.py: rank_rhat).  Build-specific: the reference reports the within-chain ESS only.
//
// Every output is a function of the sorted multiset of an element's values, so nothing here depends on the grid, on the
// order workgroups run in or on the order atomics resolve in (the only atomics are integer counts in LDS).  Launches:
//   1. key pass      [S][C][D] floats -> D segments of N = S C order-preserving 32-bit keys (tile transpose through LDS):
//                    sign-flipped bits, -0 as +0; with fold the value is |x - median[d]| in float32
//   2. sort          keys-only LSD radix sort of every segment (segment_sort.h), 4 passes of 8 bits, each pass three
//                    launches: per-tile digit histograms (LDS), one exclusive scan per (segment, digit) row, and a stable
//                    scatter (ranks within a wave from ballots, waves and tiles from the scanned counts; the tile is
//                    ordered in LDS first so that a digit's run leaves as contiguous bytes)
//   3. order stats   median and quantiles straight from the sorted RAW keys (fold: the raw sort comes first, for the
//                    median, then 1. and 2. again on the folded values -- the same code)
//   4. rank pass     every draw's key again, lower bound by binary search in its segment's sorted keys, upper bound by
//                    galloping from there (ties are short runs), rank2 = lower + upper, z = Phi^-1 of
//                    (4 rank2 + 1) / (8 N + 2) from the integers in float64, taken from whichever tail is nearer
// No hand-off inside a launch; all indices of a segment fit 32 bits (N < 2^31).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include "diag_host.h"

#pragma clang fp contract(off)

#include "segment_sort.h"                         // 1. and 2.: the key pass and the sort (shared with psens.hip)

namespace arp {
namespace {

constexpr int kRankPerThread = 8;                  // draws per thread of the rank pass

// 3. out[d] = the order statistic at 0-based index k_lo of segment d, or (mean2) 0.5f * (x[k_lo] + x[k_hi]) in float32
__global__ __launch_bounds__(kThreads) void rank_order_stat_kernel(const uint32_t* __restrict__ sorted, uint32_t N, int D,
                                                                   uint32_t k_lo, uint32_t k_hi, int mean2,
                                                                   float* __restrict__ out) {
  const int d = blockIdx.x * kThreads + threadIdx.x;
  if (d >= D) return;
  const float a = value_of(sorted[(long long)d * N + k_lo]);
  if (!mean2) { out[d] = a; return; }
  const float b = value_of(sorted[(long long)d * N + k_hi]);
  out[d] = __fmul_rn(0.5f, __fadd_rn(a, b));
}

// Phi^-1 of num / den for 0 < num < den, from the nearer tail: Phi^-1(q) = -sqrt(2) erfcinv(2 q), q <= 1/2
__device__ __forceinline__ float normal_score(unsigned long long num, unsigned long long den) {
  const unsigned long long other = den - num;
  if (num == other) return 0.0f;
  const bool lower = num < other;
  const double q = (double)(lower ? num : other) / (double)den;
  // float32 start, then one Newton step on the upper tail 0.5 erfc(z / sqrt 2) = q in float64 (the float64 erfcinv of the
  // device library is an out-of-line call that costs the kernel its occupancy)
  const double z0 = 1.4142135623730951 * (double)erfcinvf((float)(2.0 * q));        // >= 0
  const double tail = 0.5 * erfc(0.7071067811865476 * z0);
  const double dens = 0.3989422804014327 * exp(-0.5 * z0 * z0);
  const double zq = z0 + (tail - q) / dens;
  return (float)(lower ? -zq : zq);
}

// 4. rank pass: thread t of workgroup b takes the values b 2048 + k 256 + t of the contiguous [S][C][D] outputs
__global__ __launch_bounds__(kThreads) void rank_score_kernel(const float* __restrict__ trace, long long stride, uint32_t N,
                                                              uint32_t C, int D, long long n_values,
                                                              const float* __restrict__ med,
                                                              const uint32_t* __restrict__ sorted, float* __restrict__ z,
                                                              uint32_t* __restrict__ rank2) {
  const long long cd = (long long)C * D;
  const long long e0 = (long long)blockIdx.x * (kThreads * kRankPerThread) + threadIdx.x;
#pragma unroll 1                                  // (latency is hidden by resident waves, not by eight searches in registers)
  for (int k = 0; k < kRankPerThread; ++k) {
    const long long e = e0 + (long long)k * kThreads;
    if (e >= n_values) return;
    const long long s = e / cd, rem = e - s * cd;
    const int d = (int)(rem % D);
    const uint32_t key = key_of(ranked_value(trace[s * stride + rem], med, d));
    const uint32_t* a = sorted + (long long)d * N;
    // lower bound: the number of keys below `key`
    uint32_t lo = 0, n = N;
    while (n > 0) {
      const uint32_t half = n >> 1, mid = lo + half;
      if (a[mid] < key) { lo = mid + 1; n -= half + 1; } else { n = half; }
    }
    // upper bound, galloping from the lower bound (a[lo] == key: the key is one of the pool's)
    long long pos = lo < N ? lo : (long long)N - 1, step = 1;
    while (pos + step < (long long)N && a[pos + step] <= key) { pos += step; step <<= 1; }
    long long l = pos + 1, m = min(pos + step, (long long)N) - l;
    while (m > 0) {
      const long long half = m >> 1, mid = l + half;
      if (a[mid] <= key) { l = mid + 1; m -= half + 1; } else { m = half; }
    }
    const uint32_t r2 = lo + (uint32_t)l;
    if (rank2) rank2[e] = r2;
    z[e] = normal_score(4ull * r2 + 1ull, 8ull * N + 2ull);
  }
}

struct Layout {
  int64_t keys_a, keys_b, hist, totals, med, bytes;
  uint32_t tiles;
  Layout(int64_t N, int64_t D) : tiles(blocks_for(N, kTile)) {
    Carve w;
    keys_a = w.take(N * D * 4);
    keys_b = w.take(N * D * 4);
    hist = w.take(D * kBins * (int64_t)tiles * 4);
    totals = w.take(D * kBins * 4);
    med = w.take(D * 4);
    bytes = w.bytes();
  }
};

}  // namespace
}  // namespace arp

extern "C" int64_t arp_rank_workspace_bytes(int64_t n_samples, int64_t n_chains, int32_t D, int fold) {
  using namespace arp;
  (void)fold;                                   // the folded sort reuses the raw sort's buffers
  if (!trace_shape_ok(n_samples, n_chains, D, "arp_rank_workspace_bytes")) return 0;
  return Layout(n_samples * n_chains, D).bytes;
}

extern "C" int arp_rank_normalize(const float* trace, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                                  int fold, float* z, uint32_t* rank2, float* median, const double* probs, int32_t n_probs,
                                  float* quantiles, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace arp;
  if (!trace_shape_ok(n_samples, n_chains, D, "arp_rank_normalize")) return 1;
  if (!trace || !z || row_stride < n_chains * D) {
    set_error("arp_rank_normalize: trace, z and row_stride >= n_chains * D are required");
    return 1;
  }
  const bool want_q = quantiles && n_probs > 0;
  if (n_probs < 0 || (want_q && !probs)) { set_error("arp_rank_normalize: quantiles need n_probs >= 0 and probs"); return 1; }
  const int64_t N64 = n_samples * n_chains;
  const Layout L(N64, D);
  if (!workspace_size_ok(workspace && workspace_bytes >= L.bytes, "arp_rank_normalize", "see arp_rank_workspace_bytes")) return 1;
  if (!workspace_aligned(workspace, "arp_rank_normalize")) return 1;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint32_t* keys_a = (uint32_t*)(ws + L.keys_a);
  uint32_t* keys_b = (uint32_t*)(ws + L.keys_b);
  uint32_t* hist = (uint32_t*)(ws + L.hist);
  uint32_t* totals = (uint32_t*)(ws + L.totals);
  float* med = median ? median : (float*)(ws + L.med);
  const uint32_t N = (uint32_t)N64, C = (uint32_t)n_chains;
  const int dt = std::min<int>(D, kCols);
  const dim3 key_grid(blocks_for(N64, kRows), blocks_for(D, dt));
  if (key_grid.y > 65535u) { set_error("arp_rank_normalize: at most 65 535 * 128 elements per draw"); return 1; }
  const unsigned d_blocks = blocks_for(D, kThreads);

  // the raw pool, sorted: the order statistics, and the ranks themselves without fold
  hipLaunchKernelGGL(rank_key_kernel, key_grid, dim3(kThreads), 0, st, trace, (long long)row_stride, N, C, (int)D, dt,
                     (const float*)nullptr, keys_a);
  sort_segments<false>(keys_a, keys_b, nullptr, nullptr, hist, totals, N, D, L.tiles, st);
  if (median || fold)
    hipLaunchKernelGGL(rank_order_stat_kernel, dim3(d_blocks), dim3(kThreads), 0, st, (const uint32_t*)keys_a, N, (int)D,
                       (N - 1) / 2, N / 2, 1, med);
  if (want_q) {
    for (int q = 0; q < n_probs; ++q) {
      const double pk = ceil(probs[q] * (double)N64);
      const uint32_t k = !(pk >= 1.0) ? 1u : pk >= (double)N64 ? N : (uint32_t)pk;
      hipLaunchKernelGGL(rank_order_stat_kernel, dim3(d_blocks), dim3(kThreads), 0, st, (const uint32_t*)keys_a, N, (int)D,
                         k - 1, k - 1, 0, quantiles + (long long)q * D);
    }
  }
  if (fold) {
    hipLaunchKernelGGL(rank_key_kernel, key_grid, dim3(kThreads), 0, st, trace, (long long)row_stride, N, C, (int)D, dt,
                       (const float*)med, keys_a);
    sort_segments<false>(keys_a, keys_b, nullptr, nullptr, hist, totals, N, D, L.tiles, st);
  }
  const long long n_values = (long long)N64 * D;
  const long long per_block = (long long)kThreads * kRankPerThread;
  hipLaunchKernelGGL(rank_score_kernel, dim3(blocks_for(n_values, per_block)), dim3(kThreads), 0, st, trace,
                     (long long)row_stride, N, C, (int)D, n_values, fold ? (const float*)med : (const float*)nullptr,
                     (const uint32_t*)keys_a, z, rank2);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
