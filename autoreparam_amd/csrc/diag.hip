// Convergence diagnostics across chains (include/autoreparam.h: arp_split_moments, arp_moments_fold): the per-series
// first and second moments of a recorded trace, whole or per half, and their column sums over chains, from which the
// host forms the potential scale reduction factor R-hat (autoreparam_amd/diagnostics.py).  Build-specific: the
// reference reports the within-chain ESS only.
//
// arp_split_moments reads the trace once and is an HBM-streaming kernel.  Lanes run along the series axis, so every
// wave instruction reads contiguous bytes of one row: 16 B per lane (four adjacent series) where the trace pointer and
// the row stride are multiples of 16 B, 4 B per lane otherwise and for the last n_series % 4 columns; eight rows are
// loaded before the first of them is used, 8 KiB in flight per wave.
//
// Arithmetic (the same for every series whichever way it is reached, so a result does not depend on the vector width,
// the grid or the route): a part of n rows is cut into chunks of kChunk rows counted from the part's first row.  A chunk
// accumulates the shifted sums s1 = sum (x - ref), s2 = sum (x - ref)^2 with ref = its first row -- the traces hold
// elements whose mean is 10^3 - 10^4 standard deviations, where sum x^2 in float32 has no variance left -- and gives
// (mean, M2) = (ref + s1 / c, s2 - s1^2 / c).  Chunks are merged left to right with the pairwise update of Chan et al.
// Means are carried as offsets from the part's first row (ref0) and ref0 is added once at the end: a running mean of
// magnitude 10^3 would be rounded to 6e-5 at every merge, which over the 98 chunks of a 25 000-row half adds up to
// several thousandths of a standard deviation of 0.1.
// Every operation is written out (no contraction left to the compiler), there are no atomics.
//
// Two routes.  WIDE (>= kWideThreads lanes of series: the sampler's own [1 000][65 536 x 85] trace): one launch, a lane
// walks all chunks of its series and merges them in registers.  LONG (fewer series, many rows: the [50 000][1 024 x 125]
// kept trace of a streaming run): the chunk axis is cut over workgroups as well, every chunk's (mean, M2) goes to the
// caller's workspace, and a second launch merges them in the same order.  Two launches; no hand-off inside a launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "diag_host.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kChunk = 256;                  // rows per chunk
constexpr int kRowsInFlight = 8;             // rows loaded ahead per lane
constexpr int kThreads = 256;
constexpr long long kWideThreads = 128 * 1024;   // lanes of series from which the series axis alone fills the device
constexpr long long kLongTargetBlocks = 4096;    // workgroups the long route aims at

template <int V> struct Vec;
template <> struct Vec<1> { using T = float; };
template <> struct Vec<4> { using T = float4; };

template <int V> __device__ __forceinline__ void unpack(const typename Vec<V>::T& v, float (&x)[V]);
template <> __device__ __forceinline__ void unpack<1>(const float& v, float (&x)[1]) { x[0] = v; }
template <> __device__ __forceinline__ void unpack<4>(const float4& v, float (&x)[4]) { x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }

template <int V> __device__ __forceinline__ void store(float* p, const float (&x)[V]);
template <> __device__ __forceinline__ void store<1>(float* p, const float (&x)[1]) { p[0] = x[0]; }
template <> __device__ __forceinline__ void store<4>(float* p, const float (&x)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
}

// (mean - ref0, M2) of `rows` >= 1 rows starting at `p` (V adjacent series per lane)
template <int V>
__device__ __forceinline__ void chunk_moments(const float* __restrict__ p, long long stride, int rows, const float (&ref0)[V],
                                              float (&mean)[V], float (&m2)[V]) {
  using T = typename Vec<V>::T;
  float ref[V], s1[V], s2[V];
  unpack<V>(*reinterpret_cast<const T*>(p), ref);
#pragma unroll
  for (int v = 0; v < V; ++v) { s1[v] = 0.0f; s2[v] = 0.0f; }
  int r = 1;                                  // row 0 is the reference level: it adds 0 to both sums
  for (; r + kRowsInFlight <= rows; r += kRowsInFlight) {
    T buf[kRowsInFlight];
#pragma unroll
    for (int k = 0; k < kRowsInFlight; ++k) buf[k] = *reinterpret_cast<const T*>(p + (long long)(r + k) * stride);
#pragma unroll
    for (int k = 0; k < kRowsInFlight; ++k) {
      float x[V];
      unpack<V>(buf[k], x);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float d = __fsub_rn(x[v], ref[v]);
        s1[v] = __fadd_rn(s1[v], d);
        s2[v] = __fmaf_rn(d, d, s2[v]);
      }
    }
  }
  for (; r < rows; ++r) {
    float x[V];
    unpack<V>(*reinterpret_cast<const T*>(p + (long long)r * stride), x);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float d = __fsub_rn(x[v], ref[v]);
      s1[v] = __fadd_rn(s1[v], d);
      s2[v] = __fmaf_rn(d, d, s2[v]);
    }
  }
  const float c = (float)rows;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const float a = __fdiv_rn(s1[v], c);
    mean[v] = __fadd_rn(__fsub_rn(ref[v], ref0[v]), a);
    m2[v] = fmaxf(__fsub_rn(s2[v], __fmul_rn(s1[v], a)), 0.0f);
  }
}

// (na, mean, m2) <- merged with a following chunk (nb, mb, m2b); na >= 1, nb >= 1
__device__ __forceinline__ void chan_merge(float na, float& mean, float& m2, float nb, float mb, float m2b) {
  const float n = __fadd_rn(na, nb);
  const float delta = __fsub_rn(mb, mean);
  const float w = __fdiv_rn(nb, n);
  mean = __fmaf_rn(delta, w, mean);
  m2 = __fadd_rn(__fadd_rn(m2, m2b), __fmul_rn(__fmul_rn(delta, delta), __fmul_rn(na, w)));
}

__device__ __forceinline__ float var_of(float m2, long long n) {
  return n > 1 ? __fdiv_rn(m2, (float)(n - 1)) : __builtin_nanf("");
}

struct Parts {
  long long start[2];      // first row of each part
  long long rows;          // rows per part (0: an empty part)
  int P;                   // parts
  int chunks;              // chunks per part
};

// WIDE: one lane = V adjacent series, all chunks of all parts.  Series [s0, s0 + V * lanes) of the trace.
template <int V>
__global__ __launch_bounds__(kThreads) void moments_wide_kernel(const float* __restrict__ trace, long long stride, long long s0,
                                                                long long lanes, long long n_series, Parts pt,
                                                                float* __restrict__ mean_out, float* __restrict__ var_out) {
  const long long lane = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (lane >= lanes) return;
  const long long col = s0 + lane * V;
  for (int p = 0; p < pt.P; ++p) {
    float mean[V], m2[V], ref0[V];
    float na = 0.0f;
    const float* base = trace + pt.start[p] * stride + col;
    if (pt.chunks) unpack<V>(*reinterpret_cast<const typename Vec<V>::T*>(base), ref0);
    for (int j = 0; j < pt.chunks; ++j) {
      const long long r0 = (long long)j * kChunk;
      const int rows = (int)min((long long)kChunk, pt.rows - r0);
      float mb[V], m2b[V];
      chunk_moments<V>(base + r0 * stride, stride, rows, ref0, mb, m2b);
      if (j == 0) {
#pragma unroll
        for (int v = 0; v < V; ++v) { mean[v] = mb[v]; m2[v] = m2b[v]; }
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) chan_merge(na, mean[v], m2[v], (float)rows, mb[v], m2b[v]);
      }
      na += (float)rows;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      mean_out[(long long)p * n_series + col + v] = pt.chunks ? __fadd_rn(ref0[v], mean[v]) : __builtin_nanf("");
      var_out[(long long)p * n_series + col + v] = pt.chunks ? var_of(m2[v], pt.rows) : __builtin_nanf("");
    }
  }
}

// LONG, first launch: blockIdx.y takes `per_block` consecutive chunks of the P * chunks of a lane's series and writes each
// chunk's (mean - ref0, M2) to the workspace planes [P * chunks][ns_pad].
template <int V>
__global__ __launch_bounds__(kThreads) void moments_chunk_kernel(const float* __restrict__ trace, long long stride, long long s0,
                                                                 long long lanes, Parts pt, int per_block, long long ns_pad,
                                                                 float* __restrict__ ws_mean, float* __restrict__ ws_m2) {
  const long long lane = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (lane >= lanes) return;
  const long long col = s0 + lane * V;
  const int total = pt.P * pt.chunks;
  const int c0 = (int)blockIdx.y * per_block;
  const int c1 = min(c0 + per_block, total);
  for (int c = c0; c < c1; ++c) {
    const int p = c / pt.chunks, j = c - p * pt.chunks;
    const long long r0 = (long long)j * kChunk;
    const int rows = (int)min((long long)kChunk, pt.rows - r0);
    float mb[V], m2b[V], ref0[V];
    unpack<V>(*reinterpret_cast<const typename Vec<V>::T*>(trace + pt.start[p] * stride + col), ref0);
    chunk_moments<V>(trace + (pt.start[p] + r0) * stride + col, stride, rows, ref0, mb, m2b);
    store<V>(ws_mean + (long long)c * ns_pad + col, mb);
    store<V>(ws_m2 + (long long)c * ns_pad + col, m2b);
  }
}

// LONG, second launch: one lane per series merges its chunks in the order the wide route takes them.
__global__ __launch_bounds__(kThreads) void moments_merge_kernel(const float* __restrict__ trace, long long stride,
                                                                 const float* __restrict__ ws_mean, const float* __restrict__ ws_m2,
                                                                 long long ns_pad, long long n_series, Parts pt,
                                                                 float* __restrict__ mean_out, float* __restrict__ var_out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_series) return;
  for (int p = 0; p < pt.P; ++p) {
    const long long c0 = (long long)p * pt.chunks;
    float mean = ws_mean[c0 * ns_pad + i], m2 = ws_m2[c0 * ns_pad + i];
    float na = (float)min((long long)kChunk, pt.rows);
    for (int j = 1; j < pt.chunks; ++j) {
      const float nb = (float)min((long long)kChunk, pt.rows - (long long)j * kChunk);
      chan_merge(na, mean, m2, nb, ws_mean[(c0 + j) * ns_pad + i], ws_m2[(c0 + j) * ns_pad + i]);
      na += nb;
    }
    mean_out[(long long)p * n_series + i] = __fadd_rn(trace[pt.start[p] * stride + i], mean);
    var_out[(long long)p * n_series + i] = var_of(m2, pt.rows);
  }
}

constexpr int kFoldThreads = 512;

// One workgroup per column d: thread t takes rows t, t + 512, ... in ascending order, then a fixed tree over the threads.
__global__ __launch_bounds__(kFoldThreads) void moments_fold_kernel(const float* __restrict__ mean, const float* __restrict__ var,
                                                                    long long n_rows, int D, double* __restrict__ sums) {
  __shared__ double sh[5][kFoldThreads];
  const int d = blockIdx.x, t = threadIdx.x;
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long r = t; r < n_rows; r += kFoldThreads) {
    const float v = var[r * D + d];
    if (v - v == 0.0f) {                      // finite
      const double m = (double)mean[r * D + d];
      a[0] += 1.0;
      a[1] += m;
      a[2] += m * m;
      a[3] += (double)v;
      if (v == 0.0f) a[4] += 1.0;
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) sh[k][t] = a[k];
  __syncthreads();
  for (int s = kFoldThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < 5; ++k) sh[k][t] += sh[k][t + s];
    }
    __syncthreads();
  }
  if (t < 5) sums[(long long)t * D + d] = sh[t][0];
}

Parts make_parts(int64_t n_samples, int split) {
  Parts pt;
  pt.P = split ? 2 : 1;
  pt.rows = split ? n_samples / 2 : n_samples;
  pt.start[0] = 0;
  pt.start[1] = n_samples - pt.rows;
  pt.chunks = (int)((pt.rows + kChunk - 1) / kChunk);
  return pt;
}

// experiments and tests (ARP_DEBUG=1 only): ARP_MOMENTS_ROUTE=long | wide overrides the library's choice of route
int forced_route() {
  const char* e = debug_switch("ARP_MOMENTS_ROUTE");
  return !e ? 0 : e[0] == 'l' ? 2 : e[0] == 'w' ? 1 : 0;
}

bool long_route(const Parts& pt, int64_t n_series) {
  const int f = forced_route();
  if (pt.chunks < 1) return false;
  if (f) return f == 2;
  return pt.chunks >= 2 && (n_series + 3) / 4 < kWideThreads;
}

int64_t ns_padded(int64_t n_series) { return (n_series + 63) & ~(int64_t)63; }

}  // namespace
}  // namespace arp

extern "C" int64_t arp_moments_workspace_bytes(int64_t n_samples, int64_t n_series, int split) {
  using namespace arp;
  if (n_samples <= 0 || n_series <= 0) return 0;
  const Parts pt = make_parts(n_samples, split);
  if (!long_route(pt, n_series)) return 0;
  return (int64_t)2 * pt.P * pt.chunks * ns_padded(n_series) * 4;
}

extern "C" int arp_split_moments(const float* trace, int64_t n_samples, int64_t n_series, int64_t row_stride, int split,
                                 float* mean, float* var, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace arp;
  if (!trace || !mean || !var || n_samples <= 0 || n_series <= 0 || row_stride < n_series) {
    set_error("arp_split_moments: trace/mean/var, n_samples > 0, n_series > 0 and row_stride >= n_series are required");
    return 1;
  }
  if (n_series >= (1ll << 30)) { set_error("arp_split_moments: at most 2^30 - 1 series per call"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  const Parts pt = make_parts(n_samples, split ? 1 : 0);
  if ((int64_t)pt.P * pt.chunks > (1 << 24)) { set_error("arp_split_moments: at most 2^32 samples per series"); return 1; }
  // 16 B per lane over the columns [0, n4) where every row's first column is 16-byte aligned; 4 B per lane for the rest
  const bool aligned = ((uintptr_t)trace & 15) == 0 && (row_stride & 3) == 0;
  const long long n4 = aligned ? (n_series & ~3ll) : 0;
  // the long route needs its workspace; without one (or with one too small) the wide route takes any shape
  const int64_t need = arp_moments_workspace_bytes(n_samples, n_series, split ? 1 : 0);
  const bool use_long = need > 0 && workspace && workspace_bytes >= need;
  if (need > 0 && workspace && workspace_bytes < need && forced_route() == 2)
    return !workspace_size_ok(false, "arp_split_moments", "see arp_moments_workspace_bytes");
  if (use_long) {
    if (!workspace_aligned(workspace, "arp_split_moments")) return 1;
    const long long ns_pad = ns_padded(n_series);
    const int total = pt.P * pt.chunks;
    float* ws_mean = (float*)workspace;
    float* ws_m2 = ws_mean + (long long)total * ns_pad;
    const long long lanes_all = n4 / 4 + (n_series - n4);
    const long long sblocks = blocks_for(lanes_all, kThreads);
    int per_block = (int)std::max<long long>(1, (long long)total * sblocks / kLongTargetBlocks);
    while ((total + per_block - 1) / per_block > 65535) ++per_block;
    const unsigned gy = blocks_for(total, per_block);
    if (n4 > 0) {
      const long long lanes = n4 / 4;
      hipLaunchKernelGGL(moments_chunk_kernel<4>, dim3(blocks_for(lanes, kThreads), gy), dim3(kThreads), 0, st,
                         trace, (long long)row_stride, 0ll, lanes, pt, per_block, ns_pad, ws_mean, ws_m2);
    }
    if (n_series > n4) {
      const long long lanes = n_series - n4;
      hipLaunchKernelGGL(moments_chunk_kernel<1>, dim3(blocks_for(lanes, kThreads), gy), dim3(kThreads), 0, st,
                         trace, (long long)row_stride, n4, lanes, pt, per_block, ns_pad, ws_mean, ws_m2);
    }
    hipLaunchKernelGGL(moments_merge_kernel, dim3(blocks_for(n_series, kThreads)), dim3(kThreads), 0, st,
                       trace, (long long)row_stride, (const float*)ws_mean, (const float*)ws_m2, ns_pad, (long long)n_series, pt, mean, var);
    ARP_HIP_OK(hipGetLastError());
    return 0;
  }
  if (n4 > 0) {
    const long long lanes = n4 / 4;
    hipLaunchKernelGGL(moments_wide_kernel<4>, dim3(blocks_for(lanes, kThreads)), dim3(kThreads), 0, st, trace,
                       (long long)row_stride, 0ll, lanes, (long long)n_series, pt, mean, var);
  }
  if (n_series > n4) {
    const long long lanes = n_series - n4;
    hipLaunchKernelGGL(moments_wide_kernel<1>, dim3(blocks_for(lanes, kThreads)), dim3(kThreads), 0, st, trace,
                       (long long)row_stride, n4, lanes, (long long)n_series, pt, mean, var);
  }
  ARP_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int arp_moments_fold(const float* mean, const float* var, int64_t n_rows, int32_t D, double* sums, void* stream) {
  using namespace arp;
  if (!sums || n_rows < 0 || D <= 0 || (n_rows > 0 && (!mean || !var))) {
    set_error("arp_moments_fold: sums, D > 0, n_rows >= 0 and (with rows) mean/var are required");
    return 1;
  }
  hipLaunchKernelGGL(moments_fold_kernel, dim3((unsigned)D), dim3(kFoldThreads), 0, (hipStream_t)stream, mean, var,
                     (long long)n_rows, (int)D, sums);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
