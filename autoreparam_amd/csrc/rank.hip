// Rank normalisation of a recorded trace (include/autoreparam.h: arp_rank_normalize): the average rank of every draw
// within its element's pooled draws, as a normal score, and order statistics of the pool (median, quantiles) -- what the
// rank-normalised, folded split R-hat of Vehtari et al. 2021 needs below the moments kernels of diag.hip
// (autoreparam_amd/diagnostics.py: rank_rhat).  Build-specific: the reference reports the within-chain ESS only.
//
// Every output is a function of the sorted multiset of an element's values, so nothing here depends on the grid, on the
// order workgroups run in or on the order atomics resolve in (the only atomics are integer counts in LDS).  Launches:
//   1. key pass      [S][C][D] floats -> D segments of N = S C order-preserving 32-bit keys (tile transpose through LDS):
//                    sign-flipped bits, -0 as +0; with fold the value is |x - median[d]| in float32
//   2. sort          keys-only LSD radix sort of every segment, 4 passes of 8 bits, each pass three launches: per-tile
//                    digit histograms (LDS), one exclusive scan per (segment, digit) row over the tiles, and a stable
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

namespace arp {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kKeysPerThread = 16;
constexpr int kTile = kThreads * kKeysPerThread;   // keys of one sort tile (4 096)
constexpr int kBins = 256;                         // 8-bit digits
constexpr int kRows = 64;                          // rows (draws) of one key-pass tile
constexpr int kCols = 128;                         // elements of one key-pass tile at most
constexpr int kRankPerThread = 8;                  // draws per thread of the rank pass

// order-preserving key of a float: negative values bit-inverted, the others with the sign bit set; -0 is +0
__device__ __forceinline__ uint32_t key_of(float v) {
  const uint32_t u = v == 0.0f ? 0u : __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// the value that is ranked: x, or (fold) its distance from the element's median, float32
__device__ __forceinline__ float ranked_value(float x, const float* __restrict__ med, int d) {
  return med ? fabsf(__fsub_rn(x, med[d])) : x;
}

// 1. key pass.  blockIdx.x: tile of kRows consecutive draws i = s C + c; blockIdx.y: block of `dt` elements from d0.
__global__ __launch_bounds__(kThreads) void rank_key_kernel(const float* __restrict__ trace, long long stride, uint32_t N,
                                                            uint32_t C, int D, int dt, const float* __restrict__ med,
                                                            uint32_t* __restrict__ keys) {
  __shared__ uint32_t sh[kRows * (kCols + 1)];
  const int t = threadIdx.x;
  const uint32_t i0 = blockIdx.x * (uint32_t)kRows;
  const int d0 = blockIdx.y * dt;
  const int cols = min(dt, D - d0);
  const int pitch = cols | 1;
  const int rows = (int)min((uint32_t)kRows, N - i0);
  for (int e = t; e < rows * cols; e += kThreads) {
    const int r = e / cols, dd = e - r * cols;
    const uint32_t i = i0 + (uint32_t)r;
    const uint32_t s = i / C, c = i - s * C;
    const float x = trace[(long long)s * stride + (long long)c * D + d0 + dd];
    sh[r * pitch + dd] = key_of(ranked_value(x, med, d0 + dd));
  }
  __syncthreads();
  for (int e = t; e < cols * kRows; e += kThreads) {
    const int dd = e / kRows, r = e - dd * kRows;
    if (r < rows) keys[(long long)(d0 + dd) * N + i0 + r] = sh[r * pitch + dd];
  }
}

// exclusive scan of one value per thread over the workgroup; `total` = the sum.  sh: kWaves words.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t n = __shfl_up(incl, off, 64);
    if (lane >= off) incl += n;
  }
  if (lane == 63) sh[w] = incl;
  __syncthreads();
  uint32_t base = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    if (k < w) base += sh[k];
    total += sh[k];
  }
  __syncthreads();
  return base + incl - v;
}

// 2a. digit histogram of every tile: hist[(seg 256 + digit) tiles + tile].  blockIdx.x = seg tiles + tile.
__global__ __launch_bounds__(kThreads) void rank_hist_kernel(const uint32_t* __restrict__ keys, uint32_t N, uint32_t tiles,
                                                             int shift, uint32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[kBins];
  const int t = threadIdx.x;
  const uint32_t seg = blockIdx.x / tiles, tile = blockIdx.x - seg * tiles;
  cnt[t] = 0;
  __syncthreads();
  const uint32_t* src = keys + (long long)seg * N;
  const uint32_t i0 = tile * (uint32_t)kTile;
#pragma unroll
  for (int k = 0; k < kKeysPerThread; ++k) {
    const uint32_t i = i0 + (uint32_t)(k * kThreads + t);
    if (i < N) atomicAdd(&cnt[(src[i] >> shift) & (kBins - 1)], 1u);
  }
  __syncthreads();
  hist[((long long)seg * kBins + t) * tiles + tile] = cnt[t];
}

// 2b. one workgroup per (segment, digit) row: exclusive scan over its tiles in place, the row's sum to totals
__global__ __launch_bounds__(kThreads) void rank_scan_kernel(uint32_t* __restrict__ hist, uint32_t tiles,
                                                             uint32_t* __restrict__ totals) {
  __shared__ uint32_t sh[kWaves];
  uint32_t* row = hist + (long long)blockIdx.x * tiles;
  uint32_t carry = 0;
  for (uint32_t j0 = 0; j0 < tiles; j0 += kThreads) {
    const uint32_t j = j0 + threadIdx.x;
    const uint32_t v = j < tiles ? row[j] : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(v, sh, total);
    if (j < tiles) row[j] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// 2c. stable scatter of one tile by the digit at `shift`.  Wave w holds keys [1024 w, 1024 (w + 1)) of the tile, round r
// of it the 64 keys from 64 r on, one per lane: the order within a digit is (wave, round, lane).  Slots past the
// segment's end hold the largest key: they sort behind every real key of the tile and are never written.
__global__ __launch_bounds__(kThreads) void rank_scatter_kernel(const uint32_t* __restrict__ keys_in, uint32_t* __restrict__ keys_out,
                                                                uint32_t N, uint32_t tiles, int shift,
                                                                const uint32_t* __restrict__ hist,
                                                                const uint32_t* __restrict__ totals) {
  __shared__ uint32_t sorted[kTile];
  __shared__ uint32_t cnt[kWaves][kBins];
  __shared__ uint32_t tile_start[kBins];
  __shared__ uint32_t out_base[kBins];
  __shared__ uint32_t sh[kWaves];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t seg = blockIdx.x / tiles, tile = blockIdx.x - seg * tiles;
  const uint32_t* src = keys_in + (long long)seg * N;
  uint32_t* dst = keys_out + (long long)seg * N;
  const uint32_t i0 = tile * (uint32_t)kTile;
  const uint32_t valid = min((uint32_t)kTile, N - i0);

  uint32_t key[kKeysPerThread], rank[kKeysPerThread];
#pragma unroll
  for (int r = 0; r < kKeysPerThread; ++r) {
    const uint32_t j = (uint32_t)(w * (kTile / kWaves) + r * 64 + lane);
    key[r] = j < valid ? src[i0 + j] : 0xffffffffu;
  }
#pragma unroll
  for (int k = 0; k < kWaves; ++k) cnt[k][t] = 0;
  __syncthreads();

  const unsigned long long below_mask = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < kKeysPerThread; ++r) {
    const uint32_t digit = (key[r] >> shift) & (kBins - 1);
    unsigned long long peers = ~0ull;             // lanes of this round with the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (digit >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t before = cnt[w][digit];
    rank[r] = before + (uint32_t)__popcll(peers & below_mask);
    __builtin_amdgcn_wave_barrier();
    if ((peers >> lane) == 1ull) cnt[w][digit] = before + (uint32_t)__popcll(peers);   // the highest peer
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();

  // thread t = digit t: its count per wave -> the waves' offsets, the tile's start of the digit, where the run goes
  {
    uint32_t c[kWaves], sum = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) { c[k] = cnt[k][t]; }
#pragma unroll
    for (int k = 0; k < kWaves; ++k) { cnt[k][t] = sum; sum += c[k]; }
    uint32_t unused;
    const uint32_t start = block_exclusive_scan(sum, sh, unused);
    const uint32_t digit_base = block_exclusive_scan(totals[(long long)seg * kBins + t], sh, unused);
    tile_start[t] = start;
    out_base[t] = digit_base + hist[((long long)seg * kBins + t) * tiles + tile] - start;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kKeysPerThread; ++r) {
    const uint32_t digit = (key[r] >> shift) & (kBins - 1);
    sorted[tile_start[digit] + cnt[w][digit] + rank[r]] = key[r];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kKeysPerThread; ++k) {
    const uint32_t j = (uint32_t)(k * kThreads + t);
    if (j < valid) {
      const uint32_t v = sorted[j];
      dst[out_base[(v >> shift) & (kBins - 1)] + j] = v;
    }
  }
}

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

// keys (segments of N) sorted ascending; the result is in `a` again (four passes)
void sort_segments(uint32_t* a, uint32_t* b, uint32_t* hist, uint32_t* totals, uint32_t N, int D, uint32_t tiles,
                   hipStream_t st) {
  const unsigned blocks = (unsigned)D * tiles;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    hipLaunchKernelGGL(rank_hist_kernel, dim3(blocks), dim3(kThreads), 0, st, (const uint32_t*)a, N, tiles, shift, hist);
    hipLaunchKernelGGL(rank_scan_kernel, dim3((unsigned)D * kBins), dim3(kThreads), 0, st, hist, tiles, totals);
    hipLaunchKernelGGL(rank_scatter_kernel, dim3(blocks), dim3(kThreads), 0, st, (const uint32_t*)a, b, N, tiles, shift,
                       (const uint32_t*)hist, (const uint32_t*)totals);
    std::swap(a, b);
  }
}

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
  sort_segments(keys_a, keys_b, hist, totals, N, D, L.tiles, st);
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
    sort_segments(keys_a, keys_b, hist, totals, N, D, L.tiles, st);
  }
  const long long n_values = (long long)N64 * D;
  const long long per_block = (long long)kThreads * kRankPerThread;
  hipLaunchKernelGGL(rank_score_kernel, dim3(blocks_for(n_values, per_block)), dim3(kThreads), 0, st, trace,
                     (long long)row_stride, N, C, (int)D, n_values, fold ? (const float*)med : (const float*)nullptr,
                     (const uint32_t*)keys_a, z, rank2);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
