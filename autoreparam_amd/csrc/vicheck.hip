// Check of a mean-field normal fit q = N(loc, diag(scale^2)) against the density it was fitted to (include/autoreparam.h:
// arp_vi_draws, arp_vi_fold; Yao, Vehtari, Simpson, Gelman 2018).  Two ends of one pipeline whose middle the library
// already has: draws from q here, their log joint and gradient from arp_logp_grad, their centred image from
// arp_transform, the Pareto-smoothed weights of the log ratios from arp_psis_weights (psis.hip), and here again one pass
// that folds all of it into per-element sums.  Build-specific: the reference judges a fit by its ELBO alone.
//
// arp_vi_draws.  Counter based, as ppc.hip: ONE philox4x32_10(counter (e, lo32 g, hi32 g, 0), key (lo32 seed, hi32 seed))
// per draw g = draw_offset + r and group of four elements e; words (0, 1) give z[4 e] = rho cospi(2 a) and z[4 e + 1] =
// rho sinpi(2 a), words (2, 3) the next two the same way, with ppc.hip's u' in (0, 1], its angle a in [1, 2) revolutions
// and rho = sqrt(-2 log u'), through the device library's logf, sqrtf, cospif and sinpif (ppc.hip's reason: a per-element
// test needs a bound; its 18 u |z| carries over, sinpi has cospi's ulp figure).  x = fma(scale, z, loc).  One thread per
// (r, e), e fastest, so a wave stores adjacent 16-byte pieces of a row.  logq[r] = -sum_d (z_d^2 / 2 + log scale_d) -
// (D / 2) log 2 pi comes from a second launch, one thread per draw over the float32 z just stored, in float64 and in
// ascending d; log scale_d is staged in LDS, 256 elements at a time.  No result depends on the launch shape or on where a
// call's first draw lies.
//
// arp_vi_fold.  One pass over z, grad and e.  The rows are tiled (a tile is a multiple of 256 rows, at most 1024 tiles);
// within a tile thread t owns element blockIdx.y * 256 + t and walks the rows in ascending order, 256 at a time, whose
// weight exp(lw) and kept flag (lw > -inf) sit in LDS; tot comes from the same staging, thread t carrying rows t, t + 256,
// ... and a fixed tree adding the 256 threads.  A second launch adds the tiles in ascending order.  Everything in float64,
// no float atomics: two calls give bitwise equal output.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include "arp_device.h"
#include "diag_host.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kVcThreads = 256;
constexpr long long kVcMaxR = 1ll << 24;
constexpr long long kVcMaxTiles = 1024;
constexpr int kVcElemCols = 9;
constexpr int kVcTotCols = 5;
constexpr int kVcTotPitch = 8;                   // doubles per tile in the workspace's tot part
constexpr double kHalfLog2Pi = 0.91893853320467274178;

__global__ __launch_bounds__(kVcThreads) void vi_draw_kernel(const float* __restrict__ loc, const float* __restrict__ scale, int D,
                                                             int E, long long R, unsigned key0, unsigned key1,
                                                             unsigned long long draw_offset, float* __restrict__ x,
                                                             float* __restrict__ z, long long stride) {
  const long long i = (long long)blockIdx.x * kVcThreads + threadIdx.x;
  if (i >= R * E) return;
  const long long r = i / E;
  const int e = (int)(i - r * E);
  const unsigned long long g = draw_offset + (unsigned long long)r;
  uint32_t rnd[4];
  philox4x32_10((uint32_t)e, (unsigned)g, (unsigned)(g >> 32), 0u, key0, key1, rnd);
  float zz[4];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float up = fmaf((float)rnd[2 * p], 2.3283064365386963e-10f, 1.1641532182693481e-10f);
    const float rho = sqrtf(-2.0f * logf(up));
    const float a2 = 2.0f * angle_rev(rnd[2 * p + 1]);
    zz[2 * p] = rho * cospif(a2);
    zz[2 * p + 1] = rho * sinpif(a2);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = 4 * e + k;
    if (d < D) {
      z[r * stride + d] = zz[k];
      x[r * stride + d] = fmaf(scale[d], zz[k], loc[d]);
    }
  }
}

__global__ __launch_bounds__(kVcThreads) void vi_logq_kernel(const float* __restrict__ z, const float* __restrict__ scale, int D,
                                                             long long R, long long stride, double* __restrict__ logq) {
  __shared__ double ls[kVcThreads];
  const int t = threadIdx.x;
  const long long r = (long long)blockIdx.x * kVcThreads + t;
  const bool live = r < R;
  const float* row = z + (live ? r : 0) * stride;
  double acc = 0.0;
  for (int d0 = 0; d0 < D; d0 += kVcThreads) {
    const int n = min(kVcThreads, D - d0);
    __syncthreads();
    if (t < n) ls[t] = log((double)scale[d0 + t]);
    __syncthreads();
    if (live)
      for (int j = 0; j < n; ++j) {
        const double v = (double)row[d0 + j];
        acc += 0.5 * (v * v) + ls[j];
      }
  }
  if (live) logq[r] = -acc - (double)D * kHalfLog2Pi;
}

struct FoldShape { long long tile_rows, ntiles; unsigned col_blocks; };
inline FoldShape fold_shape(long long R, int D) {
  FoldShape s;
  const long long chunks = (R + kVcThreads - 1) / kVcThreads;
  s.tile_rows = (chunks + kVcMaxTiles - 1) / kVcMaxTiles * kVcThreads;
  s.ntiles = (R + s.tile_rows - 1) / s.tile_rows;
  s.col_blocks = blocks_for(D, kVcThreads);
  return s;
}
inline bool fold_shape_ok(int64_t n_draws, int32_t D) { return n_draws >= 1 && n_draws <= kVcMaxR && D >= 1 && D <= (1 << 24); }

// `op` over the 256 threads' values by a fixed tree through buf; every thread returns the result
template <bool kMin>
__device__ __forceinline__ double block_fold(double v, double* buf) {
  const int t = threadIdx.x;
  __syncthreads();
  buf[t] = v;
  __syncthreads();
  for (int s = kVcThreads / 2; s > 0; s >>= 1) {
    if (t < s) buf[t] = kMin ? fmin(buf[t], buf[t + s]) : buf[t] + buf[t + s];
    __syncthreads();
  }
  return buf[0];
}

__global__ __launch_bounds__(kVcThreads) void vi_fold_kernel(
    const float* __restrict__ z, const float* __restrict__ grad, const float* __restrict__ e, long long stride,
    const float* __restrict__ ll, const double* __restrict__ lw, const float* __restrict__ scale, const float* __restrict__ e0,
    long long R, int D, long long tile_rows, double* __restrict__ part_elem, double* __restrict__ part_tot) {
  __shared__ double sw[kVcThreads];
  __shared__ int skept[kVcThreads];
  const int t = threadIdx.x;
  const int d = (int)blockIdx.y * kVcThreads + t;
  const bool have = d < D;
  const double sc = have ? (double)scale[d] : 0.0, c0 = have ? (double)e0[d] : 0.0;
  const long long rb = (long long)blockIdx.x * tile_rows, re = min(R, rb + tile_rows);
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double a[kVcElemCols];
#pragma unroll
  for (int c = 0; c < kVcElemCols; ++c) a[c] = 0.0;
  double t_n = 0.0, t_w = 0.0, t_ww = 0.0, t_ll = 0.0, t_min = inf;
  for (long long r0 = rb; r0 < re; r0 += kVcThreads) {
    const long long r = r0 + t;
    const double lwv = r < re ? lw[r] : -inf;
    const bool kept = lwv > -inf;                // (false for NaN as well)
    const double w = kept ? exp(lwv) : 0.0;
    __syncthreads();
    sw[t] = w;
    skept[t] = kept ? 1 : 0;
    if (kept && blockIdx.y == 0) {
      const double l = (double)ll[r];
      t_n += 1.0; t_w += w; t_ww += w * w; t_ll += l; t_min = fmin(t_min, l);
    }
    __syncthreads();
    if (have) {
      const int n = (int)min((long long)kVcThreads, re - r0);
      for (int j = 0; j < n; ++j) {
        if (!skept[j]) continue;                 // (uniform over the workgroup)
        const long long at = (r0 + j) * stride + d;
        const double wj = sw[j], zz = (double)z[at], u = sc * (double)grad[at], c = (double)e[at] - c0;
        const double uz = u * zz, upz = u + zz;
        a[0] += u; a[1] += u * u; a[2] += uz; a[3] += uz * uz; a[4] += upz * upz;
        a[5] += wj * zz; a[6] += wj * (zz * zz); a[7] += wj * c; a[8] += wj * (c * c);
      }
    }
  }
  if (have) {
    double* pe = part_elem + ((long long)blockIdx.x * D + d) * kVcElemCols;
#pragma unroll
    for (int c = 0; c < kVcElemCols; ++c) pe[c] = a[c];
  }
  if (blockIdx.y == 0) {
    const double n = block_fold<false>(t_n, sw), w = block_fold<false>(t_w, sw), ww = block_fold<false>(t_ww, sw);
    const double sl = block_fold<false>(t_ll, sw), mn = block_fold<true>(t_min, sw);
    if (t == 0) {
      double* pt = part_tot + (long long)blockIdx.x * kVcTotPitch;
      pt[0] = n; pt[1] = w; pt[2] = ww; pt[3] = sl; pt[4] = mn;
    }
  }
}

// the tiles in ascending order; one thread per entry of elem, then one per entry of tot
__global__ __launch_bounds__(kVcThreads) void vi_fold_tiles(const double* __restrict__ part_elem, const double* __restrict__ part_tot,
                                                            long long n_elem, long long ntiles, double* __restrict__ elem,
                                                            double* __restrict__ tot) {
  const long long i = (long long)blockIdx.x * kVcThreads + threadIdx.x;
  if (i < n_elem) {
    double v = part_elem[i];
    for (long long ti = 1; ti < ntiles; ++ti) v += part_elem[ti * n_elem + i];
    elem[i] = v;
  } else if (i < n_elem + kVcTotCols) {
    const int c = (int)(i - n_elem);
    double v = part_tot[c];
    for (long long ti = 1; ti < ntiles; ++ti) {
      const double p = part_tot[ti * kVcTotPitch + c];
      v = c == 4 ? fmin(v, p) : v + p;
    }
    tot[c] = v;
  }
}

}  // namespace
}  // namespace arp

extern "C" int arp_vi_draws(const float* loc, const float* scale, int32_t D, int64_t n_draws, uint64_t seed, int64_t draw_offset,
                            float* x, float* z, int64_t row_stride, double* logq, void* stream) {
  using namespace arp;
  const std::string who = "arp_vi_draws";
  if (!loc || !scale || !x || !z || !logq) { set_error(who + ": loc, scale, x, z and logq are required"); return 1; }
  if (D < 1) { set_error(who + ": D >= 1 is required"); return 1; }
  if (n_draws < 1 || n_draws > kVcMaxR) { set_error(who + ": 1 <= n_draws <= 2^24 is required"); return 1; }
  if (row_stride < D) { set_error(who + ": row_stride >= D is required"); return 1; }
  if (n_draws * (int64_t)D > (1ll << 35)) { set_error(who + ": at most 2^35 values per call"); return 1; }
  if (draw_offset < 0) { set_error(who + ": draw_offset >= 0 is required"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  const int E = (D + 3) / 4;
  hipLaunchKernelGGL(vi_draw_kernel, dim3(blocks_for(n_draws * E, kVcThreads)), dim3(kVcThreads), 0, st, loc, scale, (int)D, E,
                     (long long)n_draws, (unsigned)seed, (unsigned)(seed >> 32), (unsigned long long)draw_offset, x, z,
                     (long long)row_stride);
  ARP_HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(vi_logq_kernel, dim3(blocks_for(n_draws, kVcThreads)), dim3(kVcThreads), 0, st, (const float*)z, scale, (int)D,
                     (long long)n_draws, (long long)row_stride, logq);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int64_t arp_vi_fold_workspace_bytes(int64_t n_draws, int32_t D) {
  using namespace arp;
  if (!fold_shape_ok(n_draws, D)) return 0;
  const FoldShape s = fold_shape(n_draws, D);
  Carve c;
  c.take(s.ntiles * (int64_t)D * kVcElemCols * (int64_t)sizeof(double));
  c.take(s.ntiles * kVcTotPitch * (int64_t)sizeof(double));
  return c.bytes();
}

extern "C" int arp_vi_fold(const float* z, const float* grad, const float* e, int64_t row_stride, const float* ll,
                           const double* lw, const float* scale, const float* e0, int64_t n_draws, int32_t D, double* elem,
                           double* tot, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace arp;
  const char* name = "arp_vi_fold";
  const std::string who = name;
  if (!z || !grad || !e || !ll || !lw || !scale || !e0 || !elem || !tot) {
    set_error(who + ": z, grad, e, ll, lw, scale, e0, elem and tot are required");
    return 1;
  }
  if (D < 1 || D > (1 << 24)) { set_error(who + ": 1 <= D <= 2^24 is required"); return 1; }
  if (n_draws < 1 || n_draws > kVcMaxR) { set_error(who + ": 1 <= n_draws <= 2^24 is required"); return 1; }
  if (row_stride < D) { set_error(who + ": row_stride >= D is required"); return 1; }
  const int64_t need = arp_vi_fold_workspace_bytes(n_draws, D);
  if (!workspace_size_ok(need > 0 && workspace && workspace_bytes >= need, name, "see arp_vi_fold_workspace_bytes")) return 1;
  if (!workspace_aligned(workspace, name)) return 1;
  const FoldShape s = fold_shape(n_draws, D);
  Carve c;
  double* part_elem = (double*)((char*)workspace + c.take(s.ntiles * (int64_t)D * kVcElemCols * (int64_t)sizeof(double)));
  double* part_tot = (double*)((char*)workspace + c.take(s.ntiles * kVcTotPitch * (int64_t)sizeof(double)));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(vi_fold_kernel, dim3((unsigned)s.ntiles, s.col_blocks), dim3(kVcThreads), 0, st, z, grad, e,
                     (long long)row_stride, ll, lw, scale, e0, (long long)n_draws, (int)D, s.tile_rows, part_elem, part_tot);
  ARP_HIP_OK(hipGetLastError());
  const long long n_elem = (long long)D * kVcElemCols;
  hipLaunchKernelGGL(vi_fold_tiles, dim3(blocks_for(n_elem + kVcTotCols, kVcThreads)), dim3(kVcThreads), 0, st,
                     (const double*)part_elem, (const double*)part_tot, n_elem, s.ntiles, elem, tot);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
