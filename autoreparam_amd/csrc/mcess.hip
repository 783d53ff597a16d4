// Multi-chain effective sample size of every element of a recorded trace (include/autoreparam.h: arp_ess_multichain):
// the estimator behind the bulk-ESS, the tail-ESS and the Monte-Carlo standard error of the mean of Vehtari, Gelman,
// Simpson, Carpenter, Buerkner 2021 (autoreparam_amd/diagnostics.py: bulk_tail_ess).  Build-specific: the reference
// reports the within-chain ESS only (ess.hip), which stops every series at its own first negative lag, normalises by the
// chain's own variance and divides by S - k; here the chains' autocovariances (divisor n) are averaged, the variance
// between the chains' means is added and only the pooled sequence decides where the sum is cut (Geyer).
//
// Rows: with split, every chain gives two rows of n = S / 2 draws, [0, n) and [S - n, S); without, one row of n = S.
// Row (p, c) of element d is thread i = c D + d of workgroup i / 256 in grid row p: a workgroup takes 256 consecutive
// series, so every trace row is read coalesced.  The work goes in blocks of kLags = 16 lags, two launches per block:
//   sweep   lags kb .. kb + 15 (kb = 16 b) of every row whose element is still open: the centred values
//           y = float(double(x) - mean) of the leading stream meet a 16-deep register window of the lagged stream
//           (block 0: the same stream, and the row's mean first, summed in double in a pass of its own); float products
//           in windows of 128, every window flushed into double.  The lanes of a workgroup that hold the same element
//           (its chains) are then added in lane order through LDS: one partial per (workgroup, element, lag).
//           D > 256: a workgroup holds an element at most once and every lane's sums are the partial.
//   fold    one workgroup per open element: the partials in a fixed order (float64, no floating-point atomics),
//           rho(k) = 1 - (mean_var - Gamma(k)) / var_plus, and Geyer's loop advanced over the block's pairs; the state
//           (t, E, O, the running sum, the last pair sum of the monotone sequence) waits in the workspace for the next
//           block.  An element that has been cut is marked finished: its lanes issue no further trace loads, and a launch
//           whose block no element entered leaves at once (an integer count per block, written by the fold before it).
// The monotone sequence is formed as the loop goes: a pair is final once the loop has moved past it, and it is compared
// with the (already lowered) pair before it -- the array form of the definition, in one pass.
// The host enqueues every block the longest possible cut can need and never synchronises; no workgroup waits for another
// inside a launch.  Every sum has a fixed order that depends on (S, C, D, split) alone: results are bitwise reproducible,
// and the same for a block of chains taken in place as for its contiguous copy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include "diag_host.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kMcThreads = 256;
constexpr int kLags = 16;                 // lags per block (even: a Geyer pair never straddles two blocks)
constexpr int kFlush = 128;               // float products per window
constexpr long long kMcMaxRow = 1ll << 20;  // draws per row: at most 2^16 blocks, two launches each, are enqueued

// what the Geyer loop of one element carries from block to block
struct McState {
  double E, O;          // rho(t), rho(t + 1) of the current pair
  double acc;           // sum of r[k], k < t, after the monotone step
  double prev;          // r[t-2] + r[t-1] after the monotone step
  double mean_var, var_plus;
  int t;
  int done;
};

struct McGeom {
  long long stride;     // floats between two draws
  long long n_series;   // C D
  long long n_wg;       // workgroups per half
  int n;                // draws per row
  int D;
  int P;                // rows per chain (1 + split)
  long long second;     // first draw of the second half (S - n)
  long long C;
};

__device__ __forceinline__ float mc_value(float x, bool use_thr, float thr) {
  return use_thr ? (x <= thr ? 1.0f : 0.0f) : x;
}

// lags kb .. kb + kLags - 1 of one row: sum over t of y_t y_{t - k}.  NEAR: kb = 0, the lagged stream is the leading one.
template <bool NEAR>
__device__ __forceinline__ void mc_sweep(const float* __restrict__ px, long long stride, int n, int kb, double mu,
                                         bool use_thr, float thr, double (&dacc)[kLags]) {
  float acc[kLags], w[kLags];
#pragma unroll
  for (int j = 0; j < kLags; ++j) { acc[j] = 0.0f; w[j] = 0.0f; dacc[j] = 0.0; }
  int nb = 0;
  // (products before t = kb meet a lagged value from before the row's start: nothing to add)
  for (int t0 = kb; t0 < n; t0 += kLags) {
    float xv[kLags], xl[kLags];
    if (t0 + kLags <= n) {
#pragma unroll
      for (int tt = 0; tt < kLags; ++tt) {
        xv[tt] = px[(long long)(t0 + tt) * stride];
        xl[tt] = NEAR ? xv[tt] : px[(long long)(t0 + tt - kb) * stride];
      }
    } else {
#pragma unroll
      for (int tt = 0; tt < kLags; ++tt) {
        const bool in = t0 + tt < n;
        xv[tt] = in ? px[(long long)(t0 + tt) * stride] : 0.0f;
        xl[tt] = NEAR ? xv[tt] : (in ? px[(long long)(t0 + tt - kb) * stride] : 0.0f);
      }
    }
#pragma unroll
    for (int tt = 0; tt < kLags; ++tt) {
      const bool in = t0 + tt < n;
      const float y = in ? (float)((double)mc_value(xv[tt], use_thr, thr) - mu) : 0.0f;
      const float yl = NEAR ? y : (in ? (float)((double)mc_value(xl[tt], use_thr, thr) - mu) : 0.0f);
      w[tt] = yl;                                  // w[(tt - j) mod 16] = the lagged stream j draws back
#pragma unroll
      for (int j = 0; j < kLags; ++j) acc[j] = fmaf(y, w[(tt - j + kLags) % kLags], acc[j]);
    }
    if (++nb == kFlush / kLags) {
#pragma unroll
      for (int j = 0; j < kLags; ++j) { dacc[j] += (double)acc[j]; acc[j] = 0.0f; }
      nb = 0;
    }
  }
#pragma unroll
  for (int j = 0; j < kLags; ++j) dacc[j] += (double)acc[j];
}

// the mean of one row, summed in double in draw order
__device__ __forceinline__ double mc_row_mean(const float* __restrict__ px, long long stride, int n, bool use_thr, float thr) {
  double s = 0.0;
  int t = 0;
  for (; t + 8 <= n; t += 8) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = px[(long long)(t + q) * stride];
#pragma unroll
    for (int q = 0; q < 8; ++q) s += (double)mc_value(v[q], use_thr, thr);
  }
  for (; t < n; ++t) s += (double)mc_value(px[(long long)t * stride], use_thr, thr);
  return s / (double)n;
}

// partial of (plane j, half p, workgroup g, slot s): slots = min(D, 256)
__device__ __forceinline__ long long mc_part_at(const McGeom& G, int slots, int j, int p, long long g, int s) {
  return (((long long)j * G.P + p) * G.n_wg + g) * slots + s;
}

// blockIdx.x: 256 consecutive series; blockIdx.y: the half.  block = the lag block b; active: elements that entered it.
template <bool NEAR>
__global__ __launch_bounds__(kMcThreads) void mcess_sweep_kernel(const float* __restrict__ trace, McGeom G, int block,
                                                                 const float* __restrict__ thr_of,
                                                                 const McState* __restrict__ state,
                                                                 const int* __restrict__ active,
                                                                 double* __restrict__ row_mean, double* __restrict__ part) {
  __shared__ double red[kLags][kMcThreads];
  if (!NEAR && active[block] == 0) return;                       // nothing is open: the trace is not touched
  const int tid = threadIdx.x, p = blockIdx.y;
  const long long i0 = (long long)blockIdx.x * kMcThreads, i = i0 + tid;
  const bool valid = i < G.n_series;
  const int d = valid ? (int)(i % G.D) : 0;
  const bool open = valid && (NEAR || state[d].done == 0);       // a finished element's lanes issue no trace loads
  const bool shared = G.D <= kMcThreads;                         // an element can sit in several lanes: add them in LDS
  // (thread e < D writes element e's partial even where no lane of this workgroup holds it: the fold reads every workgroup)
  const bool writes = shared && tid < G.D && (NEAR || state[tid].done == 0);
  if (!__syncthreads_or((open || writes) ? 1 : 0)) return;
  double dacc[kLags], mu = 0.0;
#pragma unroll
  for (int j = 0; j < kLags; ++j) dacc[j] = 0.0;
  if (open) {
    const bool use_thr = thr_of != nullptr;
    const float thr = use_thr ? thr_of[d] : 0.0f;
    const float* px = trace + (p ? G.second : 0ll) * G.stride + i;
    if (NEAR) {
      mu = mc_row_mean(px, G.stride, G.n, use_thr, thr);
      row_mean[(long long)p * G.n_series + i] = mu;
    } else {
      mu = row_mean[(long long)p * G.n_series + i];
    }
    mc_sweep<NEAR>(px, G.stride, G.n, block * kLags, mu, use_thr, thr, dacc);
  }
  if (!shared) {
    if (open) {
#pragma unroll
      for (int j = 0; j < kLags; ++j) part[mc_part_at(G, kMcThreads, j, p, blockIdx.x, tid)] = dacc[j];
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < kLags; ++j) red[j][tid] = dacc[j];          // (lanes that are not open hold zeros)
  __syncthreads();
  // thread e < D: element e, its lanes in ascending order (= ascending chain).  An element that no lane of the last
  // workgroup holds gets a zero partial, so that the fold reads every workgroup alike.
  if (writes) {
    const int first = (int)(((long long)tid - i0 % G.D + G.D) % G.D);
    for (int j = 0; j < kLags; ++j) {
      double s = 0.0;
      for (int l = first; l < kMcThreads; l += G.D) s += red[j][l];
      part[mc_part_at(G, G.D, j, p, blockIdx.x, tid)] = s;
    }
  }
}

// One workgroup per element.  n_rho rows of rho are written as far as the loop reads them (the host has filled it with NaN).
__global__ __launch_bounds__(kMcThreads) void mcess_fold_kernel(McGeom G, int block, int last, const double* __restrict__ part,
                                                                const double* __restrict__ row_mean,
                                                                McState* __restrict__ state, int* __restrict__ active,
                                                                float* __restrict__ ess, int32_t* __restrict__ max_t,
                                                                float* __restrict__ rho_out, int n_rho) {
  constexpr int kPlanes = kLags + 2;     // the lags, then (block 0) the sum and the sum of squares of the rows' shifted means
  __shared__ double red[kPlanes][kMcThreads];
  __shared__ double tot[kPlanes];
  if (block > 0 && active[block] == 0) return;
  const int d = blockIdx.x, tid = threadIdx.x;
  if (block > 0 && state[d].done != 0) return;                    // (uniform over the workgroup)
  const int planes = block == 0 ? kPlanes : kLags;
  const bool shared = G.D <= kMcThreads;
  const int slots = shared ? G.D : kMcThreads;
  // contributions: (half, workgroup) where workgroups hold whole elements' sums, (half, chain) otherwise
  const long long per_half = shared ? G.n_wg : G.C;
  const long long count = per_half * G.P;
  double s[kPlanes];
#pragma unroll
  for (int j = 0; j < kPlanes; ++j) s[j] = 0.0;
  for (long long q = tid; q < count; q += kMcThreads) {
    const int p = (int)(q / per_half);
    const long long u = q - (long long)p * per_half;
    long long g = u;
    int slot = d;
    if (!shared) {
      const long long i = u * G.D + d;
      g = i / kMcThreads;
      slot = (int)(i - g * kMcThreads);
    }
#pragma unroll
    for (int j = 0; j < kLags; ++j) s[j] += part[mc_part_at(G, slots, j, p, g, slot)];
  }
  if (block == 0) {
    // the rows' means about the first row's (a constant element gives exact zeros), in row order
    const double mu0 = row_mean[d];
    for (long long q = tid; q < G.C * G.P; q += kMcThreads) {
      const int p = (int)(q / G.C);
      const long long c = q - (long long)p * G.C;
      const double dm = row_mean[(long long)p * G.n_series + c * G.D + d] - mu0;
      s[kLags] += dm;
      s[kLags + 1] += dm * dm;
    }
  }
#pragma unroll
  for (int j = 0; j < kPlanes; ++j) red[j][tid] = s[j];
  __syncthreads();
  if (tid < planes) {
    double a = 0.0;
    for (int l = 0; l < kMcThreads; ++l) a += red[tid][l];
    tot[tid] = a;
  }
  __syncthreads();
  if (tid != 0) return;

  const double n = (double)G.n, m = (double)(G.C * G.P);
  McState st;
  if (block == 0) {
    const double gamma0 = tot[0] / (n * m);
    st.mean_var = gamma0 * n / (n - 1.0);
    st.var_plus = gamma0;
    if (m > 1.0) {
      const double between = (tot[kLags + 1] - tot[kLags] * tot[kLags] / m) / (m - 1.0);
      st.var_plus += between < 0.0 ? 0.0 : between;                // (rounding only; a NaN stays one)
    }
    st.t = 0; st.acc = 0.0; st.prev = 0.0; st.done = 0;
    st.E = 1.0; st.O = 0.0;
  } else {
    st = state[d];
  }
  auto rho_at = [&](int k) {                                       // k within this block
    const double r = 1.0 - (st.mean_var - tot[k - block * kLags] / (n * m)) / st.var_plus;
    if (k < n_rho) rho_out[(long long)k * G.D + d] = (float)r;
    return r;
  };
  bool nan_out = false, finished = false;
  if (block == 0) {
    if (!(st.var_plus > 0.0)) { nan_out = true; finished = true; }
    else { rho_at(0); st.O = rho_at(1); }
  }
  if (!finished) {
    const int end = (block + 1) * kLags;                           // first lag this block does not hold
    for (;;) {
      if (!(st.t < G.n - 5 && st.E + st.O > 0.0)) { finished = true; break; }
      if (st.t + 2 >= end) break;                                  // the next pair is the next block's
      // the loop moves on: the pair at t is final -- lowered to the pair before it where it exceeds that
      double pair = st.E + st.O;
      if (st.t >= 2 && pair > st.prev) pair = st.prev;
      st.acc += pair;
      st.prev = pair;
      st.t += 2;
      st.E = rho_at(st.t);
      st.O = rho_at(st.t + 1);
    }
    if (!finished && last) finished = true;                        // (the host enqueues every block the loop can reach)
  }
  if (finished) {
    float out = __builtin_nanf("");
    int mt = 0;
    if (!nan_out) {
      mt = st.t;
      const double r_max = (st.E + st.O >= 0.0) ? st.E : (st.E > 0.0 ? st.E : 0.0);
      const double N = n * m;
      double tau = -1.0 + 2.0 * st.acc + r_max;
      const double floor_tau = 1.0 / log10(N);
      if (!(tau >= floor_tau)) tau = floor_tau;                    // (a NaN ends at the floor, as fmax would)
      out = (float)(N / tau);
    }
    ess[d] = out;
    if (max_t) max_t[d] = mt;
    st.done = 1;
  } else {
    atomicAdd(&active[block + 1], 1);                              // an integer count: the next block has work
  }
  state[d] = st;
}

struct McLayout {
  int64_t state, active, mean, part, bytes;
  int n, P, blocks;
  long long n_wg;
  // blocks: the last pair the loop can reach starts at the even lag after the largest even t < n - 5
  McLayout(int64_t S, int64_t C, int64_t D, int split) {
    P = split ? 2 : 1;
    n = (int)(split ? S / 2 : S);
    const long long n_series = C * D;
    n_wg = (n_series + kMcThreads - 1) / kMcThreads;
    int t_last = 0;
    if (n > 5) t_last = 2 * ((n - 6) / 2) + 2;
    blocks = t_last / kLags + 1;
    const int64_t slots = std::min<int64_t>(D, kMcThreads);
    Carve w;
    state = w.take(D * (int64_t)sizeof(McState));
    active = w.take(((int64_t)blocks + 1) * 4);
    mean = w.take((int64_t)P * n_series * 8);
    part = w.take((int64_t)kLags * P * n_wg * slots * 8);
    bytes = w.bytes();
  }
};

bool mc_shape_ok(int64_t n_samples, int64_t n_chains, int32_t D, int split, const char* who) {
  if (!trace_shape_ok(n_samples, n_chains, D, who)) return false;
  if ((split ? n_samples / 2 : n_samples) > kMcMaxRow) {
    set_error(std::string(who) + ": at most 2^20 draws per row (n_samples, or n_samples / 2 with split)");
    return false;
  }
  return true;
}

}  // namespace
}  // namespace arp

extern "C" int64_t arp_ess_multichain_workspace_bytes(int64_t n_samples, int64_t n_chains, int32_t D, int split) {
  using namespace arp;
  if (!mc_shape_ok(n_samples, n_chains, D, split, "arp_ess_multichain_workspace_bytes")) return 0;
  return McLayout(n_samples, n_chains, D, split).bytes;
}

extern "C" int arp_ess_multichain(const float* trace, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                                  int split, const float* threshold, float* ess, int32_t* max_t, float* rho, int32_t n_rho,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace arp;
  if (!mc_shape_ok(n_samples, n_chains, D, split, "arp_ess_multichain")) return 1;
  if (!trace || !ess || row_stride < n_chains * D) {
    set_error("arp_ess_multichain: trace, ess and row_stride >= n_chains * D are required");
    return 1;
  }
  if (n_rho < 0 || (n_rho > 0 && !rho)) { set_error("arp_ess_multichain: n_rho >= 0, and rho where n_rho > 0"); return 1; }
  const McLayout L(n_samples, n_chains, D, split);
  if (!workspace_size_ok(workspace && workspace_bytes >= L.bytes, "arp_ess_multichain", "see arp_ess_multichain_workspace_bytes")) return 1;
  if (!workspace_aligned(workspace, "arp_ess_multichain")) return 1;
  if (L.n_wg > 0x7fffffffll) { set_error("arp_ess_multichain: at most 2^39 series per call"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  const int kNanBits = 0x7fc00000;
  if (!rho) n_rho = 0;
  if (n_rho > 0) ARP_HIP_OK(hipMemsetD32Async((hipDeviceptr_t)rho, kNanBits, (size_t)n_rho * (size_t)D, st));
  if (L.n < 4) {                                                  // fewer than four draws per row: NaN, nothing to launch
    ARP_HIP_OK(hipMemsetD32Async((hipDeviceptr_t)ess, kNanBits, (size_t)D, st));
    if (max_t) ARP_HIP_OK(hipMemsetAsync(max_t, 0, (size_t)D * 4, st));
    return 0;
  }
  char* ws = (char*)workspace;
  McState* state = (McState*)(ws + L.state);
  int* active = (int*)(ws + L.active);
  double* mean = (double*)(ws + L.mean);
  double* part = (double*)(ws + L.part);
  ARP_HIP_OK(hipMemsetAsync(active, 0, ((size_t)L.blocks + 1) * 4, st));
  McGeom G;
  G.stride = row_stride; G.n_series = n_chains * D; G.n_wg = L.n_wg; G.n = L.n; G.D = D; G.P = L.P;
  G.second = n_samples - L.n; G.C = n_chains;
  const dim3 sweep_grid((unsigned)L.n_wg, (unsigned)L.P);
  for (int b = 0; b < L.blocks; ++b) {
    if (b == 0)
      hipLaunchKernelGGL(mcess_sweep_kernel<true>, sweep_grid, dim3(kMcThreads), 0, st, trace, G, b, threshold,
                         (const McState*)state, (const int*)active, mean, part);
    else
      hipLaunchKernelGGL(mcess_sweep_kernel<false>, sweep_grid, dim3(kMcThreads), 0, st, trace, G, b, threshold,
                         (const McState*)state, (const int*)active, mean, part);
    hipLaunchKernelGGL(mcess_fold_kernel, dim3((unsigned)D), dim3(kMcThreads), 0, st, G, b, b + 1 == L.blocks ? 1 : 0,
                       (const double*)part, (const double*)mean, state, active, ess, max_t, rho, (int)n_rho);
  }
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
