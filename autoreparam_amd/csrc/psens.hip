// Power-scaling sensitivity (include/autoreparam.h: arp_loglik_total, arp_element_order, arp_cjs_sums; Kallioinen,
// Paananen, Buerkner, Vehtari 2023; priorsense, ArviZ psens): what the report needs below the smoothed weights of
// arp_psis_weights (autoreparam_amd/diagnostics.py: psens_summary).  Build-specific.
//   arp_loglik_total   one thread per draw adds that draw's column of a tile of pointwise log-likelihoods to a float64
//                      total, observations ascending: strictly sequential, so tiles compose bit for bit.
//   arp_element_order  the key pass and the radix sort of segment_sort.h with every key carrying its draw's index
//                      r = s C + c (the payload of the first pass is the key's own position), then, on request, the sorted
//                      keys as values.  Stable: ties in ascending r.  Integers only.
//   arp_cjs_sums       one workgroup per (element d, weight row k) walks the element's sorted draws in chunks of 256, one
//                      position per thread, twice.  Per chunk: W = exp(lw[order]) (0 by select where lw = -inf), an
//                      inclusive scan of W over the chunk -- Hillis-Steele over the 64 lanes of a wave, then the four
//                      waves' sums in ascending order -- added to the prefix carried from the chunks before; the kept
//                      count likewise from ballots.  The first sweep gives n' and S = sum W (the carried prefix after the
//                      last chunk: the very value the second sweep's last position sees) and the two weighted moments; the
//                      second forms P = count / n', Q = prefix / S at every position and adds
//                      (x[j + 1] - x[j]) f(P, Q) for every position j with 1 <= count < n'.  P and Q do not change at a
//                      position that is left out, so the gaps between two kept draws add up to b_i and the sums are those
//                      of the definition.  Every thread adds its own positions in ascending order; the 256 partial sums
//                      meet in an xor butterfly over the lanes and then wave by wave: orders that depend on N alone.
// Error bounds of arp_cjs_sums, first order, u = 2^-53, c = ceil(N / 256), finite inputs:  exp and log2 are within one ulp
// (2 u relative); a prefix of non-negative W takes at most c + 10 roundings (c carried additions, 6 within the wave, 3
// wave sums, 1 join), so Q = prefix / S is within (2 c + 25) u relative; a thread's partial sum and the joins take at most
// c + 10 roundings.  Hence, with the sums of absolute terms taken over the same positions,
//   |sum W - ref|      <= (c + 64) 2^-52 sum W              (likewise sum W u and sum W u^2 against sum |W u|, sum W u^2)
//   |I_p - ref|        <= (c + 64) 2^-52 I_p,    |I_q - ref| <= (c + 64) 2^-52 2 I_q
//   |A_pq - ref|, |A_qp - ref|
//                      <= (c + 64) 2^-52 (sum b (|P log2 P| + |Q log2 Q| + (P + Q) |log2 M|) + 2 (I_p + I_q) / ln 2)
// where the last term carries Q's relative error through Q log2 Q and through log2 M (dM / M <= dQ / Q, P / (2 M) <= 1).
// The count n' is exact.  (The constant is c + 64, not n' + 64: the carried prefix rounds once per chunk whether or not the
// chunk's draws are kept.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include "diag_host.h"

#pragma clang fp contract(off)

#include "segment_sort.h"

namespace arp {
namespace {

constexpr int kCjsColumns = 8;
constexpr int kCjsMaxRows = 8;

__global__ __launch_bounds__(kThreads) void loglik_total_kernel(const float* __restrict__ ll, long long n_obs, long long R,
                                                                long long stride, double* __restrict__ total) {
  const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (r >= R) return;
  double acc = total[r];
  for (long long n = 0; n < n_obs; ++n) acc += (double)ll[n * stride + r];
  total[r] = acc;
}

__global__ __launch_bounds__(kThreads) void order_values_kernel(const uint32_t* __restrict__ keys, long long n,
                                                                float* __restrict__ sorted) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) sorted[i] = value_of(keys[i]);
}

// log2 of 0 taken as 0 (the arguments are never negative; a NaN stays one)
__device__ __forceinline__ double log2_or_zero(double v) { return v == 0.0 ? 0.0 : log2(v); }

// One chunk's scan: `incl` = the sum of W over the chunk's positions up to this thread's, `count` = the kept ones among
// them; `total`, `kept_total`: over the whole chunk (total is bitwise the last thread's incl).  par: the chunk's parity,
// which LDS slot the waves meet in (one barrier per chunk).
__device__ __forceinline__ void chunk_scan(double W, bool kept, int par, double (*sh_w)[kWaves], uint32_t (*sh_c)[kWaves],
                                           double& incl, uint32_t& count, double& total, uint32_t& kept_total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double a = W;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double n = __shfl_up(a, off, 64);
    if (lane >= off) a += n;
  }
  const unsigned long long b = __ballot(kept);
  const uint32_t ci = (uint32_t)__popcll(b & ((2ull << lane) - 1ull));
  if (lane == 63) { sh_w[par][w] = a; sh_c[par][w] = ci; }
  __syncthreads();
  double base = sh_w[par][0];
  uint32_t cb = sh_c[par][0];
  double mine = 0.0;
  uint32_t cmine = 0;
#pragma unroll
  for (int k = 1; k < kWaves; ++k) {
    if (k == w) { mine = base; cmine = cb; }
    base += sh_w[par][k];
    cb += sh_c[par][k];
  }
  total = base;
  kept_total = cb;
  incl = w == 0 ? a : mine + a;
  count = cmine + ci;
}

// the workgroup's sum of one value per thread, in a fixed order; valid in thread 0.  sh: kWaves doubles, free again after.
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
#pragma unroll
  for (int k = 1; k < kWaves; ++k) s += sh[k];
  __syncthreads();
  return s;
}

// blockIdx.x = element d, blockIdx.y = weight row k
__global__ __launch_bounds__(kThreads) void cjs_kernel(const float* __restrict__ sorted, const uint32_t* __restrict__ order,
                                                       uint32_t N, const double* __restrict__ lw, long long lw_stride,
                                                       const float* __restrict__ shift, int D, double* __restrict__ out) {
  __shared__ double sh_w[2][kWaves];
  __shared__ uint32_t sh_c[2][kWaves];
  __shared__ double sh_r[kWaves];
  const int d = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
  const float* xs = sorted + (long long)d * N;
  const uint32_t* od = order + (long long)d * N;
  const double* lwk = lw + (long long)k * lw_stride;
  const double centre = shift ? (double)shift[d] : 0.0;
  const uint32_t chunks = (N + (uint32_t)kThreads - 1u) / (uint32_t)kThreads;
  const double ninf = -__builtin_huge_val();

  // first sweep: n', S, sum W u, sum W u^2
  double carry = 0.0, s_wu = 0.0, s_wuu = 0.0;
  uint32_t carry_n = 0;
  for (uint32_t c = 0; c < chunks; ++c) {
    const uint32_t i = c * (uint32_t)kThreads + (uint32_t)t;
    bool kept = false;
    double W = 0.0, u = 0.0;
    if (i < N) {
      const double l = lwk[min(od[i], N - 1u)];
      kept = !(l == ninf);
      if (kept) { W = exp(l); u = (double)xs[i] - centre; }
    }
    double incl, total;
    uint32_t count, kept_total;
    chunk_scan(W, kept, (int)(c & 1u), sh_w, sh_c, incl, count, total, kept_total);
    if (kept) { const double wu = W * u; s_wu += wu; s_wuu += wu * u; }
    carry += total;
    carry_n += kept_total;
  }
  const double S = carry;
  const uint32_t n_kept = carry_n;
  __syncthreads();

  // second sweep: the four integrals over the positions between the first and the last kept draw
  double a_pq = 0.0, a_qp = 0.0, i_p = 0.0, i_q = 0.0;
  carry = 0.0;
  carry_n = 0;
  for (uint32_t c = 0; c < chunks; ++c) {
    const uint32_t i = c * (uint32_t)kThreads + (uint32_t)t;
    bool kept = false;
    double W = 0.0;
    if (i < N) {
      const double l = lwk[min(od[i], N - 1u)];
      kept = !(l == ninf);
      if (kept) W = exp(l);
    }
    double incl, total;
    uint32_t count, kept_total;
    chunk_scan(W, kept, (int)(c & 1u), sh_w, sh_c, incl, count, total, kept_total);
    const uint32_t n_here = carry_n + count;
    if (i + 1u < N && n_here >= 1u && n_here < n_kept) {
      const double gap = (double)xs[i + 1u] - (double)xs[i];
      const double P = (double)n_here / (double)n_kept;
      const double Q = (carry + incl) / S;
      const double M = 0.5 * (P + Q);
      const double lm = log2_or_zero(M);
      a_pq += gap * (P * (log2_or_zero(P) - lm));
      a_qp += gap * (Q * (log2_or_zero(Q) - lm));
      i_p += gap * P;
      i_q += gap * Q;
    }
    carry += total;
    carry_n += kept_total;
  }
  __syncthreads();
  const double r0 = block_sum(s_wu, sh_r), r1 = block_sum(s_wuu, sh_r), r2 = block_sum(a_pq, sh_r);
  const double r3 = block_sum(a_qp, sh_r), r4 = block_sum(i_p, sh_r), r5 = block_sum(i_q, sh_r);
  if (t == 0) {
    double* o = out + ((long long)k * D + d) * kCjsColumns;
    o[0] = (double)n_kept; o[1] = S; o[2] = r0; o[3] = r1; o[4] = r2; o[5] = r3; o[6] = r4; o[7] = r5;
  }
}

struct OrderLayout {
  int64_t keys_a, keys_b, pay_b, hist, totals, bytes;
  uint32_t tiles;
  OrderLayout(int64_t N, int64_t D) : tiles(blocks_for(N, kTile)) {
    Carve w;
    keys_a = w.take(N * D * 4);
    keys_b = w.take(N * D * 4);
    pay_b = w.take(N * D * 4);
    hist = w.take(D * kBins * (int64_t)tiles * 4);
    totals = w.take(D * kBins * 4);
    bytes = w.bytes();
  }
};

}  // namespace
}  // namespace arp

extern "C" int arp_loglik_total(const float* ll, int64_t n_obs, int64_t n_draws, int64_t ll_stride, double* total,
                                void* stream) {
  using namespace arp;
  if (!ll || !total || n_obs < 1 || n_draws < 1 || n_draws >= (1ll << 31) || ll_stride < n_draws) {
    set_error("arp_loglik_total: ll, total, n_obs >= 1, 1 <= n_draws < 2^31 and ll_stride >= n_draws are required");
    return 1;
  }
  hipLaunchKernelGGL(loglik_total_kernel, dim3(blocks_for(n_draws, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, ll,
                     (long long)n_obs, (long long)n_draws, (long long)ll_stride, total);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int64_t arp_element_order_workspace_bytes(int64_t n_samples, int64_t n_chains, int32_t D) {
  using namespace arp;
  if (!trace_shape_ok(n_samples, n_chains, D, "arp_element_order_workspace_bytes")) return 0;
  return OrderLayout(n_samples * n_chains, D).bytes;
}

extern "C" int arp_element_order(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                                 uint32_t* order, float* sorted, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace arp;
  if (!trace_shape_ok(n_samples, n_chains, D, "arp_element_order")) return 1;
  if (!x || !order || row_stride < n_chains * D) {
    set_error("arp_element_order: x, order and row_stride >= n_chains * D are required");
    return 1;
  }
  const int64_t N64 = n_samples * n_chains;
  const OrderLayout L(N64, D);
  if (!workspace_size_ok(workspace && workspace_bytes >= L.bytes, "arp_element_order", "see arp_element_order_workspace_bytes"))
    return 1;
  if (!workspace_aligned(workspace, "arp_element_order")) return 1;
  const int dt = std::min<int>(D, kCols);
  const dim3 key_grid(blocks_for(N64, kRows), blocks_for(D, dt));
  if (key_grid.y > 65535u) { set_error("arp_element_order: at most 65 535 * 128 elements per draw"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint32_t* keys_a = (uint32_t*)(ws + L.keys_a);
  const uint32_t N = (uint32_t)N64;
  hipLaunchKernelGGL(rank_key_kernel, key_grid, dim3(kThreads), 0, st, x, (long long)row_stride, N, (uint32_t)n_chains, (int)D,
                     dt, (const float*)nullptr, keys_a);
  sort_segments<true>(keys_a, (uint32_t*)(ws + L.keys_b), order, (uint32_t*)(ws + L.pay_b), (uint32_t*)(ws + L.hist),
                (uint32_t*)(ws + L.totals), N, D, L.tiles, st);
  if (sorted) {
    const long long n = (long long)N64 * D;
    hipLaunchKernelGGL(order_values_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, st, (const uint32_t*)keys_a, n,
                       sorted);
  }
  ARP_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int arp_cjs_sums(const float* sorted, const uint32_t* order, int64_t N, int32_t D, const double* lw,
                            int64_t lw_stride, int32_t K, const float* shift, double* out, void* stream) {
  using namespace arp;
  if (!sorted || !order || !lw || !out) { set_error("arp_cjs_sums: sorted, order, lw and out are required"); return 1; }
  if (N < 1 || N >= (1ll << 31) || D < 1 || N * D > (1ll << 35)) {
    set_error("arp_cjs_sums: 1 <= N < 2^31 draws of D >= 1 elements, at most 2^35 values, are required");
    return 1;
  }
  if (K < 1 || K > kCjsMaxRows || lw_stride < N) {
    set_error("arp_cjs_sums: 1 <= K <= 8 weight rows with lw_stride >= N are required");
    return 1;
  }
  hipLaunchKernelGGL(cjs_kernel, dim3((unsigned)D, (unsigned)K), dim3(kThreads), 0, (hipStream_t)stream, sorted, order,
                     (uint32_t)N, lw, (long long)lw_stride, shift, (int)D, out);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
