// Fold of a trajectory probe (include/autoreparam.h: arp_jump_sums; trajectory_probe.h writes its inputs): for every
// leapfrog count l = 1 ... Lmax the Metropolis-weighted squared jump of every element, summed over the probed rows, and
// the counts that go with it.  Needs no model handle.  Build-specific: the reference has no counterpart.
//
//   x0 [N][D]              centred start states
//   path [Lmax][N][D]      centred state after step l
//   energy [Lmax + 1][N][2]  {lp, ke} at l = 0 ... Lmax
//   sums [Lmax][5 + D]     rows, divergent, nonfinite, sum of alpha, left_out, J[d] = sum_r alpha_r (x_rl,d - x_r0,d)^2
//
// dH = (lp0 - lp_l) + (ke_l - ke0) in float64 from the four float32 values, as diagnostics.energy_sums forms it; alpha = 0
// where dH is not finite or above 1000, min(1, exp(-dH)) otherwise.  A row with alpha = 0 is skipped, not multiplied
// (0 * NaN would poison the sum); a term with alpha > 0 that is not finite is left out and counted in left_out.
//
// One pass over `path`, no temporary of its size.  A workgroup owns one tile of rows (256 to 1 024 of them: tile_rows) of one step l: its
// lanes first form the rows' alpha in LDS, one exp per row; then lane t is (r, d) = (t / D, t % D) for r < R = threads / D
// and takes the rows r, r + R, ... of the tile, so that a pass reads R * D adjacent floats of `path` whatever D is
// (D > threads: column tiles of `threads`, one lane per column).  Differences, squares and alpha are float64.  Reduction
// order: a lane's rows ascending in kAhead interleaved running sums, those four over a tree, the R lanes of a column over a
// fixed binary tree in LDS, the counts by wave shuffles and the waves in order, the workgroups of a step in ascending order in
// a second, compensated launch (from the caller's workspace: arp_jump_workspace_bytes; one workgroup per step writes `sums`
// itself).  No atomics: a result depends on the shape alone
// and is bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "diag_host.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kThreads = 256;
constexpr int kRows = 256;             // rows of a workgroup's tile come in units of this many ...
constexpr int kRowsMax = 4 * kRows;    // ... up to this many (tile_rows)
constexpr long long kWantBlocks = 2048;  // workgroups a launch should at least have before its tiles grow (256 CUs x 8)
constexpr int kAhead = 4;              // loads of `path` (and of x0) in flight per lane
constexpr int kHead = 5;               // scalars in front of J
constexpr double kDivergence = 1000.0; // diagnostics.DIVERGENCE_THRESHOLD

// sums of the four v over the workgroup, fixed tree: the lanes of a wave by shuffles (lane i with lane i + 32, 16, ... 1), then
// the waves in ascending order; the result is valid in lane 0 of the workgroup
__device__ __forceinline__ void block_sum4(double (&v)[4], double (*sh)[kThreads / 64]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int st = 32; st >= 1; st >>= 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += __shfl_down(v[i], st, 64);
  }
  if ((t & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) sh[i][t >> 6] = v[i];
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double a = sh[i][0];
      for (int w = 1; w < kThreads / 64; ++w) a += sh[i][w];
      v[i] = a;
    }
  }
}

// Rows of a workgroup's tile for a shape: kRows, doubled (to kRowsMax at most) while the launch keeps kWantBlocks workgroups --
// few rows give short lanes and many workgroups where the launch is small, many rows give few partials where it is large.
// A function of the shape alone.
inline int tile_rows(int64_t n_rows, int32_t n_leapfrog_max) {
  int rows = kRows;
  while (rows < kRowsMax && (n_rows * n_leapfrog_max) / (2 * rows) >= kWantBlocks) rows *= 2;
  return rows;
}

// Workgroup b: row tile b % tiles of step l = b / tiles (+ 1): neighbouring workgroups read neighbouring rows of one step's
// path (the other order, the Lmax workgroups of a tile together so that x0 stays in the cache, measured slower: 32 streams
// at once).  out: [tiles][Lmax][5 + D]
__global__ __launch_bounds__(kThreads) void jump_sums_kernel(const float* __restrict__ x0, const float* __restrict__ path,
                                                             const float* __restrict__ energy, long long N, int D,
                                                             int Lmax, int rows, double* __restrict__ out) {
  __shared__ double s_alpha[kRowsMax];
  __shared__ double sh[kThreads];
  __shared__ double sh4[4][kThreads / 64];
  const int t = threadIdx.x;
  const long long tiles = (N + rows - 1) / rows;
  const int l = (int)(blockIdx.x / tiles);             // step l + 1
  const long long tile = blockIdx.x - l * tiles;
  const long long r0 = tile * rows;
  const int nr = (int)min((long long)rows, N - r0);    // rows of this tile (>= 1)
  double* o = out + (tile * Lmax + l) * (kHead + D);

  double n_div = 0.0, n_nonf = 0.0, s_acc = 0.0;
  const float* e0 = energy + r0 * 2;
  const float* el = energy + ((long long)(l + 1) * N + r0) * 2;
  for (int r = t; r < nr; r += kThreads) {
    const double lp0 = (double)e0[r * 2], ke0 = (double)e0[r * 2 + 1];
    const double lp1 = (double)el[r * 2], ke1 = (double)el[r * 2 + 1];
    const double dh = (lp0 - lp1) + (ke1 - ke0);
    const bool finite = dh - dh == 0.0;
    const bool divergent = !finite || dh > kDivergence;
    double a = 0.0;
    if (!divergent) a = fmin(1.0, exp(-dh));
    s_alpha[r] = a;
    n_div += divergent ? 1.0 : 0.0;
    n_nonf += finite ? 0.0 : 1.0;
    s_acc += a;
  }
  __syncthreads();                   // s_alpha is written

  const float* xt = x0 + r0 * D;
  const float* pt = path + ((long long)l * N + r0) * D;
  double left = 0.0;
  for (int d0 = 0; d0 < D; d0 += kThreads) {
    const int W = min(D - d0, kThreads);               // columns of this tile (D itself where D <= kThreads)
    const int R = kThreads / W;                        // lanes per column
    const int r = t / W, d = d0 + (t - r * W);
    const bool active = r < R;
    double part[kAhead];                               // one running sum per load slot: kAhead short chains, not one long
#pragma unroll
    for (int k = 0; k < kAhead; ++k) part[k] = 0.0;
    if (active) {
      for (int i = r; i < nr; i += R * kAhead) {
        float a[kAhead], b[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
          const int row = i + k * R;
          const bool take = row < nr;
          a[k] = take ? pt[(long long)row * D + d] : 0.0f;
          b[k] = take ? xt[(long long)row * D + d] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
          const int row = i + k * R;
          if (row < nr) {
            const double al = s_alpha[row];
            if (al > 0.0) {
              const double diff = (double)a[k] - (double)b[k];
              const double term = al * (diff * diff);
              if (term - term == 0.0) part[k] += term; else left += 1.0;
            }
          }
        }
      }
    }
    static_assert(kAhead == 4, "the slots are added as a tree of two levels");
    double acc = (part[0] + part[1]) + (part[2] + part[3]);
    if (R > 1) {                                       // (uniform) the R lanes of a column, over a fixed tree
      int P2 = 1;
      while (P2 * 2 < R) P2 *= 2;
      __syncthreads();
      sh[t] = acc;
      for (int st = P2; st >= 1; st >>= 1) {
        __syncthreads();
        if (active && r < st && r + st < R) {
          acc += sh[t + st * W];
          sh[t] = acc;
        }
      }
    }
    if (t < W) o[kHead + d] = acc;
  }
  double four[4] = {n_div, n_nonf, s_acc, left};
  block_sum4(four, sh4);
  if (t == 0) {
    o[0] = (double)nr; o[1] = four[0]; o[2] = four[1]; o[3] = four[2]; o[4] = four[3];
  }
}

// sums[i] = part[0][i] + part[1][i] + ... in that order, compensated (Neumaier): a large launch has thousands of partials per
// sum, and a plain chain of that length would lose what the trees of the first stage keep
__global__ __launch_bounds__(kThreads) void jump_add_kernel(const double* __restrict__ part, int nparts, long long total,
                                                            double* __restrict__ sums) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  double a = part[i], c = 0.0;
  auto add = [&](double v) {
    const double t = a + v;
    c += fabs(a) >= fabs(v) ? (a - t) + v : (v - t) + a;
    a = t;
  };
  int j = 1;
  for (; j + kAhead <= nparts; j += kAhead) {          // kAhead loads in flight, added in ascending order
    double v[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) v[k] = part[(long long)(j + k) * total + i];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) add(v[k]);
  }
  for (; j < nparts; ++j) add(part[(long long)j * total + i]);
  sums[i] = a + c;
}

bool shape_ok(int64_t n_rows, int32_t D, int32_t n_leapfrog_max) {
  return n_rows >= 1 && D >= 1 && n_leapfrog_max >= 1 && n_leapfrog_max <= 256 && n_rows <= 0x7fffffffLL / 16;
}

}  // namespace
}  // namespace arp

extern "C" int64_t arp_jump_workspace_bytes(int64_t n_rows, int32_t D, int32_t n_leapfrog_max) {
  using namespace arp;
  if (!shape_ok(n_rows, D, n_leapfrog_max)) return 0;
  const int rows = tile_rows(n_rows, n_leapfrog_max);
  const int64_t tiles = (n_rows + rows - 1) / rows;
  return tiles > 1 ? align256(tiles * n_leapfrog_max * (int64_t)(kHead + D) * 8) : 0;
}

extern "C" int arp_jump_sums(const float* x0, const float* path, const float* energy, int64_t n_rows, int32_t D,
                             int32_t n_leapfrog_max, double* sums, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace arp;
  const char* who = "arp_jump_sums";
  if (!x0 || !path || !energy || !sums) { set_error(std::string(who) + ": x0, path, energy and sums are required"); return 1; }
  if (!shape_ok(n_rows, D, n_leapfrog_max)) {
    set_error(std::string(who) + ": n_rows in 1 ... (2^31 - 1) / 16, D >= 1 and n_leapfrog_max in 1 ... 256 are required");
    return 1;
  }
  const int64_t need = arp_jump_workspace_bytes(n_rows, D, n_leapfrog_max);
  if (need > 0) {
    if (!workspace_size_ok(workspace && workspace_bytes >= need, who, "see arp_jump_workspace_bytes")) return 1;
    if (!workspace_aligned(workspace, who)) return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  const int rows = tile_rows(n_rows, n_leapfrog_max);
  const unsigned tiles = (unsigned)((n_rows + rows - 1) / rows);
  double* part = need > 0 ? (double*)workspace : sums;
  hipLaunchKernelGGL(jump_sums_kernel, dim3(tiles * (unsigned)n_leapfrog_max), dim3(kThreads), 0, st, x0, path, energy,
                     (long long)n_rows, (int)D, (int)n_leapfrog_max, rows, part);
  if (need > 0) {
    const long long total = (long long)n_leapfrog_max * (kHead + D);
    hipLaunchKernelGGL(jump_add_kernel, dim3(blocks_for(total, kThreads)), dim3(kThreads), 0, st, (const double*)part,
                       (int)tiles, total, sums);
  }
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
