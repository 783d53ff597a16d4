// Nested R-hat over superchains (include/autoreparam.h: arp_moments_fold_nested, arp_nested_step_sums): K superchains of M
// chains that start from one point each; the statistic compares the variance between superchain means with the variance
// inside superchains (Margossian, Hoffman, Sountsov, Riou-Durand, Vehtari, Gelman 2024) and is defined for one draw per
// chain.  The kernels give sums over superchains that are additive over ranks; the host forms the statistic from them in
// float64 (autoreparam_amd/diagnostics.py).  Build-specific: the reference has no counterpart.
//
// One kernel serves both entry points.  A superchain's values in one row are M * D contiguous floats (chain-major, element
// inner), so lanes run along that block, not along the element axis alone: with D <= threads a workgroup's lane t is
// (r, d) = (t / D, t % D) for r < R = threads / D, and every pass reads R * D adjacent floats, R whole chains, whatever D
// is (D = 9: 252 of 256 lanes, D = 71: 213).  M >= R: the R lanes of a column take the superchain's chains r, r + R, ...;
// M < R: a pass takes Q = R / M whole superchains, one chain per lane.  D > threads: column tiles of `threads`, one lane
// per column.  The step kernel (arp_nested_step_sums) reads a recorded trace once: a workgroup owns one row and a run of
// `kb` consecutive superchains, kAhead loads are issued per lane before the first is used, and where a row is cut over
// several workgroups each writes its sums to the caller's workspace and a second launch adds them in ascending order.
// The fold (arp_moments_fold_nested) is the same kernel on the [n_rows][D] per-chain means as one row, with the chains'
// variances read next to them, in ONE workgroup of 512 lanes and without a workspace: its input is small (37 MB at the
// headline size) and it is bound by the latency of a pass, 3 us per superchain, not by bytes.
//
// Arithmetic, float64 throughout.  A lane takes the deviations of its draws from the first of them (ref): n, s1 = sum
// (x - ref), s2 = sum (x - ref)^2, which give (n, mean, M2) = (n, ref + s1 / n, s2 - s1^2 / n) -- b_k is never a
// difference of raw squares.  The lanes of one column are merged with the pairwise update of Chan et al. over a fixed
// binary tree in LDS (lane m with lane m + 2^j, j descending); the superchain's g = mean, b = M2 / (M - 1),
// w = (sum of var) / M go into the lane's running sums, superchains in ascending order, then the Q lanes of a column in
// ascending order, then the workgroups of a row in ascending order.  No atomics: a result depends on the shape alone and
// is bitwise reproducible.  A superchain with a non-finite value (in that row and column) is left out whole.
//
// The sums over superchains stay raw (sum g, sum g^2), so that they add over ranks; the host takes
// B = (sum g^2 - (sum g)^2 / K) / (K - 1) in float64.  Each of the two terms is K gbar^2 (1 + B (K-1) / (K gbar^2)), known to
// 2^-52 of itself, so the relative error of B is ~ 2^-52 K gbar^2 / ((K - 1) B): 2e-12 for an element whose mean is 100
// between-superchain standard deviations (gbar^2 / B = 10^4), 2e-8 at 10^4.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "diag_host.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kStepThreads = 256;
constexpr int kFoldThreads = 512;
constexpr int kAhead = 8;                        // loads in flight per lane
constexpr long long kTargetBlocks = 16384;       // workgroups the step kernel aims at (8 rounds of 256 CUs x 8)
constexpr long long kMinBlockFloats = 65536;     // ... of at least this many floats each

struct Layout {
  int T;              // lanes that share one superchain's column
  int Q;              // superchains per pass
  int P2;             // the tree's first stride: the largest power of two below T
  int nsplit;         // workgroups per row
  long long kb;       // superchains per workgroup (a multiple of Q)
};

// min_floats = 0: one workgroup per row
Layout make_layout(int threads, int64_t S, int64_t K, int64_t M, int D, long long min_floats) {
  Layout l;
  const int R = D <= threads ? threads / D : 1;
  if (M >= R) { l.T = R; l.Q = 1; } else { l.T = (int)M; l.Q = R / (int)M; }
  l.P2 = 1;
  while (l.P2 * 2 < l.T) l.P2 *= 2;
  long long nsplit = 1;
  if (K > 0 && min_floats > 0) {
    const long long kb_min = std::max<long long>(1, (min_floats + M * D - 1) / (M * D));
    nsplit = std::max<long long>(1, std::min((kTargetBlocks + S - 1) / S, (K + kb_min - 1) / kb_min));
  }
  l.kb = std::max<long long>(1, (K + nsplit - 1) / nsplit);
  l.kb = (l.kb + l.Q - 1) / l.Q * l.Q;
  l.nsplit = (int)std::max<long long>(1, (K + l.kb - 1) / l.kb);
  return l;
}

// (na, ma, m2a, wa) <- merged with (nb, mb, m2b, wb); either side may be empty
__device__ __forceinline__ void merge(double& na, double& ma, double& m2a, double& wa, double nb, double mb, double m2b,
                                      double wb) {
  if (nb == 0.0) return;
  if (na == 0.0) { na = nb; ma = mb; m2a = m2b; wa = wb; return; }
  const double n = na + nb;
  const double delta = mb - ma;
  const double f = nb / n;
  ma = ma + delta * f;
  m2a = (m2a + m2b) + (delta * delta) * (na * f);
  wa = wa + wb;
  na = n;
}

// Row s = blockIdx.x / nsplit of x ([S] rows of `stride` floats, K superchains of M chains of D elements each), superchains
// [j kb, (j + 1) kb) for j = blockIdx.x % nsplit.  out: [nsplit][NOUT][S][D].  NOUT = 4: count, sum g, sum g^2, sum b.
// NOUT = 6: also sum w and the number left out; v (may be NULL: every variance 0) is addressed as x is.
template <int THREADS, int NOUT>
__global__ __launch_bounds__(THREADS) void nested_sums_kernel(const float* __restrict__ x, const float* __restrict__ v,
                                                              long long stride, long long S, long long K, long long M, int D,
                                                              Layout lay, double* __restrict__ out) {
  __shared__ double sh[NOUT > 4 ? NOUT : 4][THREADS];
  const int t = threadIdx.x;
  const long long s = blockIdx.x / lay.nsplit;
  const int j = (int)(blockIdx.x - s * lay.nsplit);
  const long long k0 = (long long)j * lay.kb, k1 = min(K, k0 + lay.kb);
  const float* row = x + s * stride;
  const float* vrow = (NOUT > 4 && v) ? v + s * stride : nullptr;
  double* o = out + ((long long)j * NOUT * S + s) * D;
  const long long step = (long long)lay.T * D;        // floats between a lane's consecutive chains
  const double Md = (double)M;

  for (int d0 = 0; d0 < D; d0 += THREADS) {
    const int W = min(D - d0, THREADS);                // columns of this tile (D itself where D <= THREADS)
    const int r = t / W, d = d0 + (t - r * W);
    const int q = r / lay.T, mem = r - q * lay.T;
    const bool active = r < lay.Q * lay.T;
    double acc[NOUT];
#pragma unroll
    for (int i = 0; i < NOUT; ++i) acc[i] = 0.0;

    for (long long kp = k0; kp < k1; kp += lay.Q) {
      const long long k = kp + q;
      const bool live = active && k < k1;
      double n = 0.0, ref = 0.0, s1 = 0.0, s2 = 0.0, sw = 0.0;
      if (live) {
        const long long at = (k * M + mem) * D + d;
        const float* p = row + at;
        const float* pv = vrow ? vrow + at : nullptr;
        const long long cnt = (M - mem + lay.T - 1) / lay.T;
        auto take = [&](float xv, float vv) {
          if (xv - xv == 0.0f && vv - vv == 0.0f) {     // both finite
            if (n == 0.0) ref = (double)xv;
            const double dev = (double)xv - ref;
            s1 += dev;
            s2 += dev * dev;
            sw += (double)vv;
            n += 1.0;
          }
        };
        for (long long i = 0; i < cnt; i += kAhead) {     // (a short last batch issues only the loads it has)
          float xb[kAhead], vb[kAhead];
#pragma unroll
          for (int a = 0; a < kAhead; ++a) xb[a] = i + a < cnt ? p[(i + a) * step] : 0.0f;
#pragma unroll
          for (int a = 0; a < kAhead; ++a) vb[a] = (pv && i + a < cnt) ? pv[(i + a) * step] : 0.0f;
#pragma unroll
          for (int a = 0; a < kAhead; ++a) {
            if (i + a < cnt) take(xb[a], vb[a]);
          }
        }
      }
      double mean = 0.0, m2 = 0.0;
      if (n > 0.0) {
        const double a = s1 / n;
        mean = ref + a;
        m2 = fmax(s2 - s1 * a, 0.0);
      }
      if (lay.T > 1) {                                   // (uniform) the T lanes of a column, over a fixed tree
        __syncthreads();                                 // the pass before has read its partners
        sh[0][t] = n; sh[1][t] = mean; sh[2][t] = m2; sh[3][t] = sw;
        for (int st = lay.P2; st >= 1; st >>= 1) {
          __syncthreads();
          if (active && mem < st && mem + st < lay.T) {
            const int u = t + st * W;
            merge(n, mean, m2, sw, sh[0][u], sh[1][u], sh[2][u], sh[3][u]);
            sh[0][t] = n; sh[1][t] = mean; sh[2][t] = m2; sh[3][t] = sw;
          }
        }
      }
      if (live && mem == 0) {
        if (n == Md) {
          acc[0] += 1.0;
          acc[1] += mean;
          acc[2] += mean * mean;
          acc[3] += m2 / (Md - 1.0);
          if (NOUT > 4) acc[4] += sw / Md;
        } else if (NOUT > 5) {
          acc[5] += 1.0;
        }
      }
    }

    if (lay.Q > 1) {                                     // (uniform) the Q lanes of a column, in ascending order
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NOUT; ++i) sh[i][t] = acc[i];
      __syncthreads();
      if (t < W) {
        for (int qq = 1; qq < lay.Q; ++qq) {
#pragma unroll
          for (int i = 0; i < NOUT; ++i) acc[i] += sh[i][qq * lay.T * W + t];
        }
      }
      __syncthreads();
    }
    if (t < W) {
#pragma unroll
      for (int i = 0; i < NOUT; ++i) o[(long long)i * S * D + d] = acc[i];
    }
  }
}

// sums[i] = part[0][i] + part[1][i] + ... in that order
__global__ __launch_bounds__(kStepThreads) void nested_add_kernel(const double* __restrict__ part, int nsplit, long long total,
                                                                  double* __restrict__ sums) {
  const long long i = (long long)blockIdx.x * kStepThreads + threadIdx.x;
  if (i >= total) return;
  double a = part[i];
  for (int j = 1; j < nsplit; ++j) a += part[(long long)j * total + i];
  sums[i] = a;
}

// what both step entry points ask of their arguments; K superchains on success
bool step_shape_ok(int64_t n_samples, int64_t n_chains, int32_t D, int64_t group, const char* who) {
  if (!trace_shape_ok(n_samples, n_chains, D, who)) return false;
  if (group < 2 || n_chains % group != 0) {
    set_error(std::string(who) + ": a group size M >= 2 that divides n_chains is required");
    return false;
  }
  return true;
}

}  // namespace
}  // namespace arp

extern "C" int arp_moments_fold_nested(const float* mean, const float* var, int64_t n_rows, int32_t D, int64_t group,
                                       double* sums, void* stream) {
  using namespace arp;
  if (!sums || n_rows < 0 || D <= 0 || (n_rows > 0 && !mean)) {
    set_error("arp_moments_fold_nested: sums, D > 0, n_rows >= 0 and (with rows) mean are required");
    return 1;
  }
  if (group < 2 || n_rows % group != 0) {
    set_error("arp_moments_fold_nested: a group size M >= 2 that divides n_rows is required");
    return 1;
  }
  if (n_rows >= (1ll << 31)) { set_error("arp_moments_fold_nested: at most 2^31 - 1 rows"); return 1; }
  const int64_t K = n_rows / group;
  const Layout lay = make_layout(kFoldThreads, 1, K, group, D, 0);
  hipLaunchKernelGGL((nested_sums_kernel<kFoldThreads, 6>), dim3(1), dim3(kFoldThreads), 0, (hipStream_t)stream, mean, var,
                     (long long)n_rows * D, 1ll, (long long)K, (long long)group, (int)D, lay, sums);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int64_t arp_nested_step_workspace_bytes(int64_t n_samples, int64_t n_chains, int32_t D, int64_t group) {
  using namespace arp;
  if (n_samples <= 0 || n_chains <= 0 || D <= 0 || group < 2 || n_chains % group != 0) return 0;
  const Layout lay = make_layout(kStepThreads, n_samples, n_chains / group, group, D, kMinBlockFloats);
  return lay.nsplit > 1 ? align256((int64_t)lay.nsplit * 4 * n_samples * D * 8) : 0;
}

extern "C" int arp_nested_step_sums(const float* trace, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                                    int64_t group, double* sums, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace arp;
  const char* who = "arp_nested_step_sums";
  if (!trace || !sums) { set_error(std::string(who) + ": trace and sums are required"); return 1; }
  if (!step_shape_ok(n_samples, n_chains, D, group, who)) return 1;
  if (row_stride < n_chains * D) { set_error(std::string(who) + ": row_stride >= n_chains * D is required"); return 1; }
  const int64_t K = n_chains / group;
  const Layout lay = make_layout(kStepThreads, n_samples, K, group, D, kMinBlockFloats);
  const int64_t need = arp_nested_step_workspace_bytes(n_samples, n_chains, D, group);
  if (need > 0) {
    if (!workspace_size_ok(workspace && workspace_bytes >= need, who, "see arp_nested_step_workspace_bytes")) return 1;
    if (!workspace_aligned(workspace, who)) return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  double* part = need > 0 ? (double*)workspace : sums;
  hipLaunchKernelGGL((nested_sums_kernel<kStepThreads, 4>), dim3((unsigned)(n_samples * lay.nsplit)), dim3(kStepThreads), 0, st,
                     trace, (const float*)nullptr, (long long)row_stride, (long long)n_samples, (long long)K, (long long)group,
                     (int)D, lay, part);
  if (need > 0) {
    const long long total = 4ll * n_samples * D;
    hipLaunchKernelGGL(nested_add_kernel, dim3(blocks_for(total, kStepThreads)), dim3(kStepThreads), 0, st,
                       (const double*)part, lay.nsplit, total, sums);
  }
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
