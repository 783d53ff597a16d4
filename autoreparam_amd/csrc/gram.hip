// Cross moments of a trace on the matrix cores (include/autoreparam.h: arp_gram_sums): G = sum_r u_r u_r^T over the rows
// of a [rows][D] float32 matrix, u_r = x_r - shift, next to sum_r u_r and the row counts -- what the posterior geometry
// report (autoreparam_amd/diagnostics.py: gram_sums, geometry_from_sums, scale_coupling) takes a covariance from.
// Build-specific: the reference has closed forms for a two-dimensional toy only.
//
// Shape of the work.  The columns are cut into nb = ceil(D / 32) blocks; every pair of blocks (bi <= bj), the upper
// triangle only, is one 32 x 32 accumulator of v_mfma_f32_32x32x2_f32, whose inner (k) axis is the ROW axis: one
// instruction takes two rows.  Lane l holds A[i = l & 31][k = l >> 5] = u[row k][32 bi + i] and
// B[k][j = l & 31] = u[row k][32 bj + j], one VGPR each; a diagonal pair reads the same LDS word for both.  A workgroup
// of four waves owns one CHUNK of rows (blockIdx.x) and one GROUP of 4 P pairs (blockIdx.y; a wave holds P pairs, P = 1, 2
// or 4 by the number of pairs).  It stages a tile of T whole rows (T = 64, 32 or 16 by D alone) of u in LDS, finds which
// of them are left out, and its waves multiply their pairs from LDS.  Every group stages all D columns: the row mask
// needs them.  The loads of the next tile are issued into registers before the current tile is multiplied.
//
// Arithmetic.  u = x - shift in float32, one rounding.  An accumulator runs over a window of kGramWindow rows -- bit for
// bit a k-ordered fmaf chain of that length -- and is then added into float64 registers; at the end of its chunk a wave
// writes those to the caller's workspace, and a second launch adds the chunks up in an order fixed by their number (runs
// of adjacent chunks in ascending order, then the runs in ascending order) and writes G and its mirror from ONE value.
// Chunks are whole windows, cut by the number of rows and D alone: no atomics, two calls are bitwise equal, and a block of
// chains read in place (row_stride > n_chains * D, any alignment) gives bitwise the sums of its contiguous copy -- the
// stride enters the load addresses only, never the tiling.  The column sums (row D) are float64 sums of u over the tile's
// rows, thread per column; the counts are integers.
//
//   |G_dev - G_f64|[i][j] <= (kGramWindow + 1) 2^-24 sum_r |u_ri u_rj|
//
// (G_f64: the float64 sum of the float32 u): the first-order bound of an f32 fmaf chain of window length plus one rounding
// of each product; what the float64 additions add is 2^-53 per window and chunk.
//
// Three things that go wrong quietly here:
//  * Zeroed operands.  Padding columns (d >= D in the last block), rows past the end of a chunk (the missing row of an odd
//    count among them) and rows that are left out enter the MFMA as 0 by SELECT (or were stored as 0), never by a
//    multiplication with a 0 / 1 mask: 0 * inf is NaN, and a NaN in one operand lane poisons 32 results.
//  * Reads past the end.  A load is issued for (row < end of chunk, d < D) only: nothing is read past
//    x[(n_samples - 1) * row_stride + n_chains * D - 1].  Dead lanes of the staging loop take the value 0 without a load.
//  * Rows left out.  Whether a row counts depends on all D of its elements, hence on columns that belong to other pairs:
//    the mask of a tile is complete (a barrier after staging) before any pair of any of its rows is multiplied.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "diag_host.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kGramWindow = 256;                 // rows an f32 accumulator runs over (diagnostics.GRAM_WINDOW)
constexpr int kGramMaxD = 512;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileFloats = 8192;                // the LDS tile: T rows of Dp floats, 32 KB
constexpr int kLoads = kTileFloats / kThreads;   // the most elements of a tile one lane stages
constexpr int kBatch = 8;                        // elements store() handles between two branches
constexpr long long kTargetWorkgroups = 1024;    // the grid aims at this many workgroups (256 CUs x 4)
constexpr int kBlockEntries = 32 * 32;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Plan {
  int nb;                 // column blocks of 32
  int Dp;                 // 32 nb: the tile's row pitch in floats
  int npairs;             // nb (nb + 1) / 2
  int P;                  // pairs per wave
  int ngroups;            // workgroups along y: ceil(npairs / (4 P))
  int T;                  // rows per tile, a power of two that divides kGramWindow
  long long R;            // rows in all
  long long chunk_rows;   // rows per workgroup along x, a multiple of kGramWindow
  long long nchunks;
  long long part_stride;  // doubles per chunk in the workspace: npairs * 1024, Dp column sums, 2 counts
};

// the plan depends on (rows, D) alone
Plan make_plan(long long R, int D) {
  Plan p;
  p.nb = (D + 31) / 32;
  p.Dp = 32 * p.nb;
  p.npairs = p.nb * (p.nb + 1) / 2;
  p.P = p.npairs <= kWaves ? 1 : (p.npairs <= 2 * kWaves ? 2 : 4);
  p.ngroups = (p.npairs + kWaves * p.P - 1) / (kWaves * p.P);
  p.T = 16;
  while (p.T < 64 && 2 * p.T * p.Dp <= kTileFloats) p.T *= 2;
  p.R = R;
  const long long nwin = (R + kGramWindow - 1) / kGramWindow;
  const long long target = std::max<long long>(1, kTargetWorkgroups / p.ngroups);
  const long long wpc = (nwin + target - 1) / target;
  p.chunk_rows = wpc * kGramWindow;
  p.nchunks = (nwin + wpc - 1) / wpc;
  p.part_stride = (long long)p.npairs * kBlockEntries + p.Dp + 2;
  return p;
}

// pair q of the upper triangle, row-major: (bi, bj), bi <= bj
__device__ __forceinline__ void pair_blocks(int q, int nb, int& bi, int& bj) {
  bi = 0;
  while (q >= nb - bi) { q -= nb - bi; ++bi; }
  bj = bi + q;
}

// The first N of a wave's pairs over the rows of the tile in LDS, two rows per instruction: lane l takes row 2 m + (l >> 5),
// column 32 b + (l & 31) of block b.  A row that is left out enters as 0 by select, never as a product with a mask.
template <int P, int N>
__device__ __forceinline__ void multiply(f32x16 (&acc)[P], const float* tile, int Dp, int l31, int half, unsigned long long bad,
                                         int msteps, const int (&ca)[P], const int (&cb)[P]) {
  // the operands of step m + 1 are read from LDS before the instructions of step m are issued
  float a[N], b[N];
  auto read = [&](int m, float (&ra)[N], float (&rb)[N]) {
    const int row = 2 * m + half;
    const bool zero = (bad >> row) & 1;
    const float* rp = tile + row * Dp + l31;
#pragma unroll
    for (int p = 0; p < N; ++p) {
      const float av = rp[ca[p]], bv = rp[cb[p]];
      ra[p] = zero ? 0.0f : av;
      rb[p] = zero ? 0.0f : bv;
    }
  };
  read(0, a, b);
  for (int m = 0; m < msteps; ++m) {
    float na[N], nb[N];
    read(min(m + 1, msteps - 1), na, nb);          // (the last step reads its own row again)
#pragma unroll
    for (int p = 0; p < N; ++p) acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[p], b[p], acc[p], 0, 0, 0);
#pragma unroll
    for (int p = 0; p < N; ++p) { a[p] = na[p]; b[p] = nb[p]; }
  }
}

// (the second launch bound, waves per SIMD: one and two pairs per wave sit a register or two above the next occupancy step)
template <int P>
__global__ __launch_bounds__(kThreads, (P == 1 ? 3 : P == 2 ? 2 : 1)) void gram_kernel(const float* __restrict__ x, long long n_chains, int D, long long stride,
                                                        const float* __restrict__ shift, Plan pl, double* __restrict__ part) {
  __shared__ float tile[kTileFloats];
  __shared__ float sh_shift[kGramMaxD];
  __shared__ int sh_bad[2][64];                  // per tile row: 1 where the row is left out (two tiles in flight)
  const int t = threadIdx.x;
  const int lane = t & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int T = pl.T, Dp = pl.Dp;
  const long long r0 = (long long)blockIdx.x * pl.chunk_rows, r1 = min(pl.R, r0 + pl.chunk_rows);
  const int g = blockIdx.y;
  const long long gap = stride - n_chains * D;   // floats between the end of a recorded step and the next

  for (int i = t; i < kTileFloats; i += kThreads) tile[i] = 0.0f;     // the padding columns stay 0 from here on
  for (int i = t; i < Dp; i += kThreads) sh_shift[i] = (shift && i < D) ? shift[i] : 0.0f;
  if (t < 128) sh_bad[t >> 6][t & 63] = 0;

  // Pairs interleaved over the waves, q = (g P + p) 4 + slot; the slot of a wave turns with the chunk, so that where the
  // pairs do not divide by four the heavier waves of neighbouring workgroups do not share a SIMD.
  const int slot = (wave + (int)blockIdx.x) & (kWaves - 1);
  int ca[P], cb[P];
  bool on[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int q = (g * P + p) * kWaves + slot;
    on[p] = q < pl.npairs;
    int bi = 0, bj = 0;
    if (on[p]) pair_blocks(q, pl.nb, bi, bj);
    ca[p] = 32 * bi;
    cb[p] = 32 * bj;
  }
  int nact = 0;                                  // the pairs this wave holds: p < nact
#pragma unroll
  for (int p = 0; p < P; ++p) nact += on[p] ? 1 : 0;
  nact = __builtin_amdgcn_readfirstlane(nact);
  f32x16 acc[P];
  double acc64[P][16];
#pragma unroll
  for (int p = 0; p < P; ++p) {
#pragma unroll
    for (int v = 0; v < 16; ++v) { acc[p][v] = 0.0f; acc64[p][v] = 0.0; }
  }
  // (g == 0) the column sums of d = ct and d = ct + 256: the columns start at the slots that hold the fewest pairs
  const int ct = (slot * 64 + lane) ^ 128;
  double cs0 = 0.0, cs1 = 0.0;
  long long kept = 0, left = 0;                  // (g == 0, t == 0)

  // element e = t + 256 a of a tile is (row e / D, column e % D): the same walk in every tile, without a division
  const int lr_first = t / D, d_first = t - lr_first * D;
  const int q256 = kThreads / D, rem256 = kThreads - q256 * D;
  const int nelem = T * D;
  int in_window = 0, par = 0;
  float xv[kLoads];                              // a tile's elements of this lane, loaded while the tile before is multiplied

  // the loads of the tile at row `tile0` (nrows of them alive); a dead lane takes 0 without a load
  auto issue = [&](long long tile0, int nrows) {
    if (gap == 0) {                              // rows are adjacent in memory: element e of the tile is tile0 * D + e
      const float* tb = x + tile0 * D;
      const int nlive = nrows * D;
#pragma unroll
      for (int a = 0; a < kLoads; ++a) {
        xv[a] = 0.0f;
        if (a * kThreads < nlive && a * kThreads + t < nlive) xv[a] = tb[a * kThreads + t];
      }
      return;
    }
    int lr = lr_first, d = d_first;
#pragma unroll
    for (int a = 0; a < kLoads; ++a) {
      xv[a] = 0.0f;
      if ((a / kBatch) * kBatch * kThreads < nelem) {        // (uniform; the batches of store())
        if (a * kThreads + t < nelem && lr < nrows) {
          const long long r = tile0 + lr;
          long long off = r * D + d;
          if (gap != 0) off += (long long)((unsigned)r / (unsigned)n_chains) * gap;
          xv[a] = x[off];
        }
        d += rem256;
        lr += q256;
        if (d >= D) { d -= D; ++lr; }
      }
    }
  };
  // u = x - shift into the LDS tile, and the rows it spoils into the mask; a dead row is stored as 0
  auto store = [&](int nrows, int par) {
    int lr = lr_first, d = d_first;
#pragma unroll
    for (int a0 = 0; a0 < kLoads; a0 += kBatch) {
      if (a0 * kThreads < nelem) {               // (uniform)
        float sh[kBatch];
        int at[kBatch], rr[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {       // the LDS reads of the shift, with no branch between them
          sh[k] = sh_shift[d];
          at[k] = (a0 + k) * kThreads + t < nelem ? lr * Dp + d : -1;
          rr[k] = lr < nrows ? lr : -1;
          d += rem256;
          lr += q256;
          if (d >= D) { d -= D; ++lr; }
        }
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
          if (at[k] >= 0) {
            const float u = rr[k] >= 0 ? xv[a0 + k] - sh[k] : 0.0f;
            tile[at[k]] = u;
            if (!(u - u == 0.0f)) sh_bad[par][rr[k]] = 1;                  // (only a live row can get here)
          }
        }
      }
    }
  };

  issue(r0, (int)min((long long)T, r1 - r0));
  for (long long tile0 = r0; tile0 < r1; tile0 += T, par ^= 1) {
    const int nrows = (int)min((long long)T, r1 - tile0);
    __syncthreads();                             // the tile before has been read
    store(nrows, par);
    __syncthreads();                             // the tile and its row mask are complete
    if (tile0 + T < r1) issue(tile0 + T, (int)min((long long)T, r1 - tile0 - T));      // in flight while this tile is multiplied
    const unsigned long long bad = __ballot(lane < T && sh_bad[par][lane] != 0);
    if (t < 64) sh_bad[par ^ 1][t] = 0;          // for the next tile; its last readers passed the barrier above

    if (g == 0) {
      if (t == 0) {
        const int nbad = __popcll(bad);
        left += nbad;
        kept += nrows - nbad;
      }
      if (ct < D) {                              // (dead rows hold 0; rows left out are skipped by select)
#pragma unroll 8
        for (int r = 0; r < T; ++r) {
          const float v = tile[r * Dp + ct];
          cs0 += ((bad >> r) & 1) ? 0.0 : (double)v;
        }
      }
      if (ct + kThreads < D) {
#pragma unroll 8
        for (int r = 0; r < T; ++r) {
          const float v = tile[r * Dp + ct + kThreads];
          cs1 += ((bad >> r) & 1) ? 0.0 : (double)v;
        }
      }
    }

    // (the number of pairs a wave holds is uniform; a branch INSIDE the row loop would make the accumulators loop-carried
    // values of two paths, which the compiler then copies out of and back into the accumulation registers every step)
    const int msteps = (nrows + 1) / 2;
    if (nact == P) multiply<P, P>(acc, tile, Dp, l31, half, bad, msteps, ca, cb);
    else if (P > 1 && nact == P - 1) multiply<P, (P > 1 ? P - 1 : 1)>(acc, tile, Dp, l31, half, bad, msteps, ca, cb);
    else if (P > 2 && nact == P - 2) multiply<P, (P > 2 ? P - 2 : 1)>(acc, tile, Dp, l31, half, bad, msteps, ca, cb);
    else if (P > 3 && nact == P - 3) multiply<P, (P > 3 ? P - 3 : 1)>(acc, tile, Dp, l31, half, bad, msteps, ca, cb);

    if (++in_window == kGramWindow / T || tile0 + T >= r1) {          // the window is full, or the chunk ends
      in_window = 0;
#pragma unroll
      for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int v = 0; v < 16; ++v) { acc64[p][v] += (double)acc[p][v]; acc[p][v] = 0.0f; }
      }
    }
  }

  double* o = part + (long long)blockIdx.x * pl.part_stride;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if (on[p]) {
      const int q = (g * P + p) * kWaves + slot;
#pragma unroll
      for (int v = 0; v < 16; ++v) o[(long long)q * kBlockEntries + v * 64 + lane] = acc64[p][v];
    }
  }
  if (g == 0) {
    double* oc = o + (long long)pl.npairs * kBlockEntries;
    if (ct < D) oc[ct] = cs0;
    if (ct + kThreads < D) oc[ct + kThreads] = cs1;
    if (t == 0) { oc[Dp] = (double)kept; oc[Dp + 1] = (double)left; }
  }
}

// sums = the chunks' partials added up.  A workgroup takes kMergeItems adjacent items; the chunks are cut into kMergeSlices
// contiguous runs of ceil(nchunks / kMergeSlices), one lane per (run, item) adds its run in ascending order, and the runs are
// then added in ascending order: an order that depends on the number of chunks alone.  Item i < npairs * 1024 is accumulator
// register v = (i >> 6) & 15 of lane l = i & 63 of pair i >> 10: G[32 bi + (v & 3) + 8 (v >> 2) + 4 (l >> 5)][32 bj + (l & 31)],
// written with its mirror from the one value (of a diagonal pair only the entries with row <= column are taken); then the D
// column sums; then the D entries of row D + 1.
constexpr int kMergeItems = 16, kMergeSlices = kThreads / kMergeItems;

__global__ __launch_bounds__(kThreads) void gram_merge_kernel(const double* __restrict__ part, Plan pl, int D,
                                                              double* __restrict__ sums) {
  __shared__ double run[kMergeSlices][kMergeItems];
  const int it = threadIdx.x % kMergeItems, sl = threadIdx.x / kMergeItems;
  const long long i = (long long)blockIdx.x * kMergeItems + it;
  const long long nG = (long long)pl.npairs * kBlockEntries;
  const bool live = i < nG + 2 * D;
  // where item i sits in a chunk's partials; the entries of row D + 1 past the two counts are 0
  long long at = i;
  bool zero = !live;
  if (live && i >= nG + D) {
    const int d = (int)(i - nG - D);
    at = nG + pl.Dp + d;
    zero = d >= 2;
  }
  const long long per = (pl.nchunks + kMergeSlices - 1) / kMergeSlices;
  const long long c0 = sl * per, c1 = min(pl.nchunks, c0 + per);
  double a = 0.0;
  if (!zero) {
    for (long long c = c0; c < c1; c += 8) {
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = c + k < c1 ? part[(c + k) * pl.part_stride + at] : 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (c + k < c1) a += v[k];
      }
    }
  }
  run[sl][it] = a;
  __syncthreads();
  if (sl != 0 || !live) return;
  for (int k = 1; k < kMergeSlices; ++k) a += run[k][it];
  if (i >= nG + D) { sums[(long long)(D + 1) * D + (i - nG - D)] = a; return; }
  if (i >= nG) { sums[(long long)D * D + (i - nG)] = a; return; }
  int bi, bj;
  pair_blocks((int)(i >> 10), pl.nb, bi, bj);
  const int v = (int)(i >> 6) & 15, l = (int)i & 63;
  const int row = (v & 3) + 8 * (v >> 2) + 4 * (l >> 5), col = l & 31;
  const int gi = 32 * bi + row, gj = 32 * bj + col;
  if (gi >= D || gj >= D || (bi == bj && row > col)) return;
  sums[(long long)gi * D + gj] = a;
  sums[(long long)gj * D + gi] = a;
}

bool gram_shape_ok(int64_t n_samples, int64_t n_chains, int32_t D) {
  return n_samples >= 1 && n_chains >= 1 && D >= 1 && D <= kGramMaxD && n_samples < (1ll << 31) && n_chains < (1ll << 31) &&
         n_samples * n_chains < (1ll << 31);
}

}  // namespace
}  // namespace arp

extern "C" int64_t arp_gram_workspace_bytes(int64_t n_samples, int64_t n_chains, int32_t D) {
  using namespace arp;
  if (!gram_shape_ok(n_samples, n_chains, D)) return 0;
  const Plan pl = make_plan(n_samples * n_chains, D);
  return align256(pl.nchunks * pl.part_stride * 8);
}

extern "C" int arp_gram_sums(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                             const float* shift, double* sums, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace arp;
  const char* who = "arp_gram_sums";
  if (!x || !sums) { set_error(std::string(who) + ": x and sums are required"); return 1; }
  if (D < 1 || D > kGramMaxD) { set_error(std::string(who) + ": 1 <= D <= 512 is required"); return 1; }
  if (n_samples < 1 || n_chains < 1) { set_error(std::string(who) + ": n_samples >= 1 and n_chains >= 1 are required"); return 1; }
  if (!gram_shape_ok(n_samples, n_chains, D)) {
    set_error(std::string(who) + ": at most 2^31 - 1 rows (n_samples * n_chains)");
    return 1;
  }
  if (row_stride < n_chains * D) { set_error(std::string(who) + ": row_stride >= n_chains * D is required"); return 1; }
  const int64_t need = arp_gram_workspace_bytes(n_samples, n_chains, D);
  if (!workspace_size_ok(workspace && workspace_bytes >= need, who, "see arp_gram_workspace_bytes")) return 1;
  if (!workspace_aligned(workspace, who)) return 1;
  const Plan pl = make_plan(n_samples * n_chains, D);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  const dim3 grid((unsigned)pl.nchunks, (unsigned)pl.ngroups);
  if (pl.P == 1) {
    hipLaunchKernelGGL((gram_kernel<1>), grid, dim3(kThreads), 0, st, x, (long long)n_chains, (int)D, (long long)row_stride,
                       shift, pl, part);
  } else if (pl.P == 2) {
    hipLaunchKernelGGL((gram_kernel<2>), grid, dim3(kThreads), 0, st, x, (long long)n_chains, (int)D, (long long)row_stride,
                       shift, pl, part);
  } else {
    hipLaunchKernelGGL((gram_kernel<4>), grid, dim3(kThreads), 0, st, x, (long long)n_chains, (int)D, (long long)row_stride,
                       shift, pl, part);
  }
  const long long items = (long long)pl.npairs * kBlockEntries + 2 * D;
  hipLaunchKernelGGL(gram_merge_kernel, dim3(blocks_for(items, kMergeItems)), dim3(kThreads), 0, st, (const double*)part, pl,
                     (int)D, sums);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
