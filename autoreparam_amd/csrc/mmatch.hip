// Moment matching for importance sampling (include/autoreparam.h: arp_weighted_moments, arp_affine_rows; Paananen,
// Piironen, Buerkner, Vehtari 2021, "Implicitly adaptive importance sampling"; loo::loo_moment_match): the two device
// pieces the host loop (autoreparam_amd/diagnostics.py: moment_match) needs besides the densities and the tail fit.
// Model-independent; no model handle.  Build-specific: the reference has no importance sampling.
//
//   arp_weighted_moments  for B targets at once, the first two weighted moments of every column of one [R][D] float32
//                         matrix of draws about a caller-given centre, each target with its own row of float64 log
//                         weights.  Three launches:
//     head   one workgroup per target walks the target's lw row: lw_max (NaN entries skipped; exact) and the number of
//            draws kept (lw != -inf; exact), from per-thread chains joined by an xor butterfly and a wave-by-wave pass.
//     chunk  workgroup (c, j) takes the 256 rows of chunk c and the (up to) 8 targets of group j.  It first writes
//            W[k][i] = exp(lw[r] - lw_max) (0 by select where lw = -inf) for its rows and targets into LDS, one float64 exp
//            per (target, row), then walks the chunk of x ONCE for all 8 targets: thread t owns column d = t % D and the row
//            lane q = t / D of L = 256 / D row lanes, reads x[r][d] for r = q, q + L, ... (adjacent threads read adjacent
//            floats of a row; a row is never read past its D-th element, so a row_stride > D and the end of x are
//            safe), forms e = (double)x - (double)centre[d] and adds W e and (W e) e into 2 x 8 registers.  The L row
//            lanes of a column meet in LDS and are added in ascending q by the thread with q = 0.  sum W and sum W^2 of a
//            target: wave v takes targets v and v + 4, lane l adds rows l, l + 64, l + 128, l + 192 in that order, then an
//            xor butterfly.  The chunk's 2 + 2 D partial sums of every target go to the workspace.
//     fold   one workgroup per target adds the chunks' partials of every column in ascending c and writes the row.
//   Every order above is a function of (R, D) alone -- not of B, not of where among the targets b stands (a target's
//   position in its group of 8 picks a register and an LDS row, not an order) -- and there are no float atomics: two calls
//   give the same bits, and target b's row is the same alone or among many.  x is re-read once per group of 8 targets.
//
//   arp_affine_rows       out[b][r][d] = (x[r][d] - m[b][d]) * s[b][d] + u[b][d] in float32, three roundings in that order
//                         (contraction off), for the rows the parity picks; the other rows are copied as bits (through a
//                         uint32 load and store: a NaN's payload survives).  A workgroup takes 64 rows; a thread loads an
//                         element of x once and stores it B times, adjacent threads adjacent floats.  The forward map, the
//                         split and the inverse map of the host loop are all this kernel with other (m, s, u).
//
// Error bound of arp_weighted_moments, first order, u = 2^-53.  A kept draw's weight is w = exp(fl(lw - lw_max)); the
// device's exp is within one unit in the last place (2 u relative).  e = x - centre rounds once (u), W e once more, (W e) e
// once more: a term is within 5 u of the exact product of the same w and the exact e, 4 u for the first moment.  A sum of R'
// kept terms takes at most R' roundings whatever the tree (an addition of a left-out draw's exact 0 does not round, nor
// does a join with an empty partial).  Hence, for every output sum s = sum w t (t = 1, w, e or e^2 -- sum w^2 squares the
// error of w: 4 u and one rounding),
//   |s_dev - s| <= (R' + 32) 2 u sum w |t|
// against the exact sum of the same weights w_r = exp(fl(lw_r - lw_max)) -- the subtraction in front of exp is part of
// the definition (it is exact within a factor of two of the maximum, and an argument of size a carries u |a| into w
// otherwise, whichever way the weights are formed in float64).  Measured: DESIGN.md section 6.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "diag_host.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kMmThreads = 256;
constexpr int kMmWaves = kMmThreads / 64;
constexpr int kMmChunk = 256;      // rows a workgroup of the chunk kernel takes
constexpr int kMmGroup = 8;        // targets a workgroup of the chunk kernel takes
constexpr int kMmMaxD = 255;
constexpr int kMmMaxTargets = 4096;
constexpr int kMmHead = 4;         // lw_max, sum w, sum w^2, draws kept
constexpr int kAffineRows = 64;    // rows a workgroup of the affine kernel takes

// What the workspace holds: head [B][2] double (lw_max, kept) and partial [chunks][B][2 + 2 D] double.
struct MomentsLayout {
  int64_t head, partial, bytes, chunks;
  MomentsLayout(int64_t R, int64_t D, int64_t B) : chunks((R + kMmChunk - 1) / kMmChunk) {
    Carve w;
    head = w.take(B * 2 * 8);
    partial = w.take(chunks * B * (2 + 2 * D) * 8);
    bytes = w.bytes();
  }
};

__global__ __launch_bounds__(kMmThreads) void mm_head_kernel(const double* __restrict__ lw, long long lw_stride, long long R,
                                                             double* __restrict__ head) {
  __shared__ double sh_m[kMmWaves];
  __shared__ unsigned long long sh_n[kMmWaves];
  const int b = blockIdx.x, t = threadIdx.x;
  const double* row = lw + (long long)b * lw_stride;
  const double ninf = -__builtin_huge_val();
  double m = ninf;
  unsigned long long n = 0;
  for (long long r = t; r < R; r += kMmThreads) {
    const double l = row[r];
    if (l > m) m = l;            // false for a NaN: skipped
    n += (l == ninf) ? 0ull : 1ull;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double om = __shfl_xor(m, off, 64);
    if (om > m) m = om;
    n += __shfl_xor(n, off, 64);
  }
  if ((t & 63) == 0) { sh_m[t >> 6] = m; sh_n[t >> 6] = n; }
  __syncthreads();
  if (t == 0) {
    for (int k = 1; k < kMmWaves; ++k) { if (sh_m[k] > m) m = sh_m[k]; n += sh_n[k]; }
    head[2 * b] = m;
    head[2 * b + 1] = (double)n;
  }
}

// blockIdx.x = chunk c, blockIdx.y = target group j
__global__ __launch_bounds__(kMmThreads) void mm_chunk_kernel(const float* __restrict__ x, long long R, int D,
                                                              long long row_stride, const double* __restrict__ lw,
                                                              long long lw_stride, int B, const float* __restrict__ centre,
                                                              const double* __restrict__ head, double* __restrict__ partial) {
  __shared__ double sh_w[kMmGroup][kMmChunk];
  __shared__ double sh_p[kMmThreads];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long r0 = (long long)blockIdx.x * kMmChunk;
  const int rows = (int)((R - r0) < (long long)kMmChunk ? (R - r0) : (long long)kMmChunk);
  const int b0 = blockIdx.y * kMmGroup;
  const int nb = (B - b0) < kMmGroup ? (B - b0) : kMmGroup;
  const double ninf = -__builtin_huge_val();
  const int cols = 2 + 2 * D;

  // the weights of this chunk: thread t = row i, every target of the group
  for (int k = 0; k < kMmGroup; ++k) {
    double W = 0.0;
    if (k < nb && t < rows) {
      const double l = lw[(long long)(b0 + k) * lw_stride + r0 + t];
      const double e = exp(l - head[2 * (b0 + k)]);
      W = (l == ninf) ? 0.0 : e;
    }
    sh_w[k][t] = W;
  }
  __syncthreads();

  // sum W and sum W^2: wave v takes targets v and v + 4
  for (int k = wave; k < nb; k += kMmWaves) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < kMmChunk; i += 64) {
      const double W = sh_w[k][i + lane];
      s1 += W;
      s2 += W * W;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      s1 += __shfl_xor(s1, off, 64);
      s2 += __shfl_xor(s2, off, 64);
    }
    if (lane == 0) {
      double* p = partial + ((long long)blockIdx.x * B + (b0 + k)) * cols;
      p[0] = s1;
      p[1] = s2;
    }
  }

  // the two moments of every column: thread t = (row lane q, column d)
  const int L = kMmThreads / D;          // D <= 255: L >= 1
  const int q = t / D, d = t - q * D;
  const bool active = q < L;
  double a1[kMmGroup], a2[kMmGroup];
#pragma unroll
  for (int k = 0; k < kMmGroup; ++k) { a1[k] = 0.0; a2[k] = 0.0; }
  if (active) {
    const double c = (double)centre[d];
    for (int i = q; i < rows; i += L) {
      const double e = (double)x[(r0 + i) * row_stride + d] - c;
#pragma unroll
      for (int k = 0; k < kMmGroup; ++k) {
        const double W = sh_w[k][i];
        // a left-out draw enters nothing, whatever its state holds
        const double we = (W == 0.0) ? 0.0 : W * e;
        a1[k] += we;
        a2[k] += (W == 0.0) ? 0.0 : we * e;
      }
    }
  }
  // the row lanes of a column, ascending q
#pragma unroll
  for (int k = 0; k < kMmGroup; ++k) {
    if (k >= nb) break;                  // uniform
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      __syncthreads();
      sh_p[t] = which == 0 ? a1[k] : a2[k];
      __syncthreads();
      if (t < D) {
        double s = sh_p[t];
        for (int qq = 1; qq < L; ++qq) s += sh_p[qq * D + t];
        partial[((long long)blockIdx.x * B + (b0 + k)) * cols + 2 + 2 * t + which] = s;
      }
    }
  }
}

// blockIdx.x = target b
__global__ __launch_bounds__(kMmThreads) void mm_fold_kernel(const double* __restrict__ head, const double* __restrict__ partial,
                                                             long long chunks, int B, int D, double* __restrict__ out) {
  const int b = blockIdx.x, cols = 2 + 2 * D;
  double* o = out + (long long)b * (kMmHead + 2 * D);
  if (threadIdx.x == 0) { o[0] = head[2 * b]; o[3] = head[2 * b + 1]; }
  for (int j = threadIdx.x; j < cols; j += kMmThreads) {
    double s = 0.0;
    for (long long c = 0; c < chunks; ++c) s += partial[(c * B + b) * cols + j];
    o[j < 2 ? 1 + j : 2 + j] = s;
  }
}

// blockIdx.x = tile of kAffineRows rows
__global__ __launch_bounds__(kMmThreads) void affine_rows_kernel(const float* __restrict__ x, long long R, int D,
                                                                 long long row_stride, const float* __restrict__ m,
                                                                 const float* __restrict__ s, const float* __restrict__ u, int B,
                                                                 int parity, float* __restrict__ out) {
  const long long r0 = (long long)blockIdx.x * kAffineRows;
  const int rows = (int)((R - r0) < (long long)kAffineRows ? (R - r0) : (long long)kAffineRows);
  const int n = rows * D;
  const long long plane = R * (long long)D;
  for (int i = threadIdx.x; i < n; i += kMmThreads) {
    const int ri = i / D, d = i - ri * D;
    const long long r = r0 + ri;
    const float v = x[r * row_stride + d];
    const bool mapped = parity < 0 || (int)(r & 1) == parity;
    float* o = out + r0 * D + i;
    if (mapped) {
      for (int b = 0; b < B; ++b) {
        const float a = v - m[b * D + d];
        const float p = a * s[b * D + d];
        o[(long long)b * plane] = p + u[b * D + d];
      }
    } else {
      const uint32_t bits = __float_as_uint(v);
      for (int b = 0; b < B; ++b) reinterpret_cast<uint32_t*>(o)[(long long)b * plane] = bits;
    }
  }
}

bool moments_shape_ok(int64_t R, int32_t D, int64_t B, const char* who) {
  const bool ok = R >= 1 && R < (1ll << 31) && D >= 1 && D <= kMmMaxD && B >= 1 && B <= kMmMaxTargets;
  if (!ok) set_error(std::string(who) + ": 1 <= n_rows < 2^31, 1 <= D <= 255 and 1 <= n_targets <= 4096 are required");
  return ok;
}

}  // namespace
}  // namespace arp

extern "C" int64_t arp_weighted_moments_workspace_bytes(int64_t n_rows, int32_t D, int64_t n_targets) {
  using namespace arp;
  if (!moments_shape_ok(n_rows, D, n_targets, "arp_weighted_moments_workspace_bytes")) return 0;
  return MomentsLayout(n_rows, D, n_targets).bytes;
}

extern "C" int arp_weighted_moments(const float* x, int64_t n_rows, int32_t D, int64_t row_stride, const double* lw,
                                    int64_t n_targets, int64_t lw_stride, const float* centre, double* out, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  using namespace arp;
  const char* who = "arp_weighted_moments";
  if (!x || !lw || !centre || !out) { set_error("arp_weighted_moments: x, lw, centre and out are required"); return 1; }
  if (!moments_shape_ok(n_rows, D, n_targets, who)) return 1;
  if (row_stride < D || lw_stride < n_rows) {
    set_error("arp_weighted_moments: row_stride >= D and lw_stride >= n_rows are required");
    return 1;
  }
  const MomentsLayout L(n_rows, D, n_targets);
  if (!workspace_size_ok(workspace && workspace_bytes >= L.bytes, who, "see arp_weighted_moments_workspace_bytes")) return 1;
  if (!workspace_aligned(workspace, who)) return 1;
  hipStream_t st = (hipStream_t)stream;
  double* head = (double*)((char*)workspace + L.head);
  double* partial = (double*)((char*)workspace + L.partial);
  const int B = (int)n_targets;
  hipLaunchKernelGGL(mm_head_kernel, dim3((unsigned)B), dim3(kMmThreads), 0, st, lw, (long long)lw_stride, (long long)n_rows,
                     head);
  hipLaunchKernelGGL(mm_chunk_kernel, dim3((unsigned)L.chunks, blocks_for(B, kMmGroup)), dim3(kMmThreads), 0, st, x,
                     (long long)n_rows, (int)D, (long long)row_stride, lw, (long long)lw_stride, B, centre,
                     (const double*)head, partial);
  hipLaunchKernelGGL(mm_fold_kernel, dim3((unsigned)B), dim3(kMmThreads), 0, st, (const double*)head, (const double*)partial,
                     (long long)L.chunks, B, (int)D, out);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int arp_affine_rows(const float* x, int64_t n_rows, int32_t D, int64_t row_stride, const float* m, const float* s,
                               const float* u, int64_t n_targets, int32_t parity, float* out, void* stream) {
  using namespace arp;
  if (!x || !m || !s || !u || !out) { set_error("arp_affine_rows: x, m, s, u and out are required"); return 1; }
  if (!moments_shape_ok(n_rows, D, n_targets, "arp_affine_rows")) return 1;
  if (row_stride < D || parity > 1 || out == x || n_targets * n_rows * D > (1ll << 35)) {
    set_error("arp_affine_rows: row_stride >= D, parity <= 1, out != x and at most 2^35 values written are required");
    return 1;
  }
  hipLaunchKernelGGL(affine_rows_kernel, dim3(blocks_for(n_rows, kAffineRows)), dim3(kMmThreads), 0, (hipStream_t)stream, x,
                     (long long)n_rows, (int)D, (long long)row_stride, m, s, u, (int)n_targets, (int)parity, out);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
