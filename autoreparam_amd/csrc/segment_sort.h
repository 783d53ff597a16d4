// The segmented radix sort the rank diagnostics share (rank.hip: keys only; psens.hip: every key carries the index of its
// draw).  D segments of N order-preserving 32-bit keys, sorted ascending by an LSD radix sort, 4 passes of 8 bits, each
// pass three launches: per-tile digit histograms (LDS), one exclusive scan per (segment, digit) row over the tiles, and a
// stable scatter (ranks within a wave from ballots, waves and tiles from the scanned counts; the tile is ordered in LDS
// first so that a digit's run leaves as contiguous bytes).  Stable: keys that are equal keep the order they came in, so
// with the payload of the first pass -- a key's own position in its segment -- ties end in ascending position.
// Nothing depends on the grid or on the order atomics resolve in (the only atomics are integer counts in LDS); all
// indices of a segment fit 32 bits (N < 2^31).  The payload is a template parameter: without it the kernels are the
// keys-only sort, instruction for instruction.  Everything is in an unnamed namespace: every translation unit that includes
// this has kernels of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

namespace arp {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kKeysPerThread = 16;
constexpr int kTile = kThreads * kKeysPerThread;   // keys of one sort tile (4 096)
constexpr int kBins = 256;                         // 8-bit digits
constexpr int kRows = 64;                          // rows (draws) of one key-pass tile
constexpr int kCols = 128;                         // elements of one key-pass tile at most

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

// key pass: [S][C][D] floats -> D segments of N = S C keys (tile transpose through LDS).  blockIdx.x: tile of kRows
// consecutive draws i = s C + c; blockIdx.y: block of `dt` elements from d0.
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

// a. digit histogram of every tile: hist[(seg 256 + digit) tiles + tile].  blockIdx.x = seg tiles + tile.
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

// b. one workgroup per (segment, digit) row: exclusive scan over its tiles in place, the row's sum to totals
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

// c. stable scatter of one tile by the digit at `shift`.  Wave w holds keys [1024 w, 1024 (w + 1)) of the tile, round r
// of it the 64 keys from 64 r on, one per lane: the order within a digit is (wave, round, lane).  Slots past the
// segment's end hold the largest key: they sort behind every real key of the tile and are never written.
// kPayload: a 32-bit word travels with every key (pay_in == nullptr: the key's position in its segment, the first pass).
template <bool kPayload>
__global__ __launch_bounds__(kThreads) void rank_scatter_kernel(const uint32_t* __restrict__ keys_in, uint32_t* __restrict__ keys_out,
                                                                const uint32_t* __restrict__ pay_in, uint32_t* __restrict__ pay_out,
                                                                uint32_t N, uint32_t tiles, int shift,
                                                                const uint32_t* __restrict__ hist,
                                                                const uint32_t* __restrict__ totals) {
  __shared__ uint32_t sorted[kTile];
  __shared__ uint32_t sorted_pay[kPayload ? kTile : 1];
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

  uint32_t key[kKeysPerThread], rank[kKeysPerThread], pay[kPayload ? kKeysPerThread : 1];
#pragma unroll
  for (int r = 0; r < kKeysPerThread; ++r) {
    const uint32_t j = (uint32_t)(w * (kTile / kWaves) + r * 64 + lane);
    key[r] = j < valid ? src[i0 + j] : 0xffffffffu;
    if constexpr (kPayload) pay[r] = (pay_in && j < valid) ? pay_in[(long long)seg * N + i0 + j] : i0 + j;
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
    const uint32_t at = tile_start[digit] + cnt[w][digit] + rank[r];
    sorted[at] = key[r];
    if constexpr (kPayload) sorted_pay[at] = pay[r];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kKeysPerThread; ++k) {
    const uint32_t j = (uint32_t)(k * kThreads + t);
    if (j < valid) {
      const uint32_t v = sorted[j];
      const uint32_t to = out_base[(v >> shift) & (kBins - 1)] + j;
      dst[to] = v;
      if constexpr (kPayload) pay_out[(long long)seg * N + to] = sorted_pay[j];
    }
  }
}

// keys (segments of N) sorted ascending; the result is in `a` again (four passes).  kPayload: pay_a, pay_b are two buffers
// of the keys' size, neither read before it is written, and pay_a ends as the position every sorted key came from.
template <bool kPayload>
inline void sort_segments(uint32_t* a, uint32_t* b, uint32_t* pay_a, uint32_t* pay_b, uint32_t* hist, uint32_t* totals,
                          uint32_t N, int D, uint32_t tiles, hipStream_t st) {
  const unsigned blocks = (unsigned)D * tiles;
  const uint32_t* pay_in = nullptr;
  uint32_t* pay_out = pay_b;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    hipLaunchKernelGGL(rank_hist_kernel, dim3(blocks), dim3(kThreads), 0, st, (const uint32_t*)a, N, tiles, shift, hist);
    hipLaunchKernelGGL(rank_scan_kernel, dim3((unsigned)D * kBins), dim3(kThreads), 0, st, hist, tiles, totals);
    hipLaunchKernelGGL(rank_scatter_kernel<kPayload>, dim3(blocks), dim3(kThreads), 0, st, (const uint32_t*)a, b, pay_in,
                       pay_out, N, tiles, shift, (const uint32_t*)hist, (const uint32_t*)totals);
    if (kPayload) {
      pay_in = pay_out;
      pay_out = pay_out == pay_b ? pay_a : pay_b;
    }
    std::swap(a, b);
  }
}

}  // namespace
}  // namespace arp
