// The fold of simulation-based calibration (include/autoreparam.h: arp_sbc_fold; Talts, Betancourt, Simpson, Vehtari,
// Gelman 2018): for every replicate r and every quantity q, where the replicate's truth t = truth[r][q] sits among the
// n_draws posterior draws x = draws[r][.][q] that a refit on data simulated from that truth returned --
//
//   counts[r][q] = ( #{x < t}, #{x == t} )        int32      what the rank statistic is made of
//   sums[r][q]   = ( sum (x - t), sum (x - t)^2 ) float64    what the posterior z-score is made of
//
// and left_out[r], the replicates that enter nothing.  Model-independent; needs no model handle.  Build-specific: the
// reference never refits on simulated data.  The statistics on top of these sums: diagnostics.sbc_summary.
//
// Shape of the work.  One workgroup of four waves per replicate.  It walks the replicate's rows in tiles: all 256 threads
// stage a tile of whole rows in LDS -- element e = t + 256 a of the tile is (row e / Q, column e % Q), so adjacent lanes
// load adjacent floats of a row and every draw is read once, coalesced, whatever Q is -- and thread q < Q then owns
// quantity q down the tile's rows, rows ascending.  Its LDS reads are tile[i * pitch + q]: the lanes of a wave read
// adjacent words of one row, one bank each at any pitch; the pitch is Q | 1 as obs_table.h's, whose lane-per-row reads
// need it.  A tile holds 8 192 floats / pitch rows (31 at Q = 256, 92 at Q = 89), 32 KiB: four workgroups a CU.  The
// order of every addition is a function of n_draws alone -- not of the tile, the grid or the strides.  No float atomics;
// the one atomic is the integer count n_left_out.
//
// Arithmetic.  x and t go to float64 (exact) and d = x - t is ONE float64 subtraction: its sign and its being zero are
// those of the exact difference (the smallest difference of two float32 values, 2^-149, is far inside float64's range,
// and rounding keeps the sign), so the counts are exact, denormals included, and -0.0 == 0.0 counts as equal.  s1 is the
// chain s1 <- s1 + d and s2 the chain s2 <- s2 + d d (the product rounded once, contraction off) over rows 0 ... n_draws - 1
// in that order.  Recursive summation of n terms in any order is within (n - 1) 2^-53 sum |term| of the exact sum of the
// same float64 terms, to first order; the tests hold it to n 2^-53 sum |term|.
//
// A replicate that is left out: one whose truth or any of whose n_draws x Q draws is not finite.  Its counts and sums are
// WRITTEN, as 0 by select -- never by a product with a mask, which would keep a NaN -- and left_out[r] = 1.
//
// Things that go wrong quietly here:
//  * Reads past the end.  A load is issued for (row < n_draws, column < Q) only; nothing is read past
//    draws[(n_rep - 1) rep_stride + (n_draws - 1) row_stride + Q - 1] or truth[(n_rep - 1) truth_stride + Q - 1].  The
//    padding between rows and between replicates is never read, so the result is bitwise independent of it.
//  * The flag.  A thread that stages a non-finite draw of ANOTHER thread's column must reach that thread: the flags meet
//    in one LDS word behind a barrier, after the last tile (every writer writes 1).  Until then the sums of such a
//    replicate run on with NaN; the select at the end is what keeps it out.
//  * int32 counts: n_draws <= 2^24.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "diag_host.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kSbcThreads = 256;
constexpr int kSbcMaxQ = 256;                    // a quantity per thread
constexpr int kSbcTileFloats = 8192;             // 32 KiB of LDS: at least 31 rows of pitch 257
constexpr int kSbcBatch = 16;                    // loads a thread has in flight: half of its share of a full tile
constexpr long long kSbcMaxDraws = 1ll << 24, kSbcMaxRep = 1ll << 20;

__global__ __launch_bounds__(kSbcThreads) void sbc_fold_kernel(const float* __restrict__ draws, int n_draws, int Q,
                                                               long long rep_stride, long long row_stride,
                                                               const float* __restrict__ truth, long long truth_stride,
                                                               int* __restrict__ counts, double* __restrict__ sums,
                                                               unsigned char* __restrict__ left_out,
                                                               unsigned long long* __restrict__ n_left_out) {
  __shared__ float tile[kSbcTileFloats];         // [rows][Q | 1]
  __shared__ int sh_bad;
  const int t = threadIdx.x;
  const long long r = blockIdx.x;
  const int pitch = Q | 1;
  const int rows = kSbcTileFloats / pitch;
  const float* x = draws + r * rep_stride;
  const bool own = t < Q;
  if (t == 0) sh_bad = 0;                        // (published by the first barrier of the loop: n_draws >= 1)
  bool bad = false;
  double tq = 0.0;
  if (own) {
    const float tv = truth[r * truth_stride + t];
    bad = !(tv - tv == 0.0f);
    tq = (double)tv;
  }
  // element e = t + 256 a of a tile is (row e / Q, column e % Q), kept by steps of 256 = step_r Q + step_d
  const int lr0 = t / Q, d0 = t - lr0 * Q;
  const int step_r = kSbcThreads / Q, step_d = kSbcThreads - step_r * Q;
  int less = 0, equal = 0;
  double s1 = 0.0, s2 = 0.0;
  for (int i0 = 0; i0 < n_draws; i0 += rows) {
    const int nrows = min(rows, n_draws - i0);
    __syncthreads();                             // the tile before this one has been read
    // kSbcBatch loads are issued before the first of them is waited for (one at a time, a thread's up to 32 loads of a
    // tile were 32 memory latencies in a row: 0.23 ms at N = L = 1 024, Q = 89, against 0.14 ms for a copy of the buffer)
    for (int lr = lr0, d = d0; lr < nrows;) {
      float v[kSbcBatch];
      int at[kSbcBatch];
#pragma unroll
      for (int k = 0; k < kSbcBatch; ++k) {
        const bool live = lr < nrows;            // (lr only grows: a dead slot is followed by dead slots)
        at[k] = live ? lr * pitch + d : -1;
        v[k] = live ? x[(long long)(i0 + lr) * row_stride + d] : 0.0f;
        lr += step_r;
        d += step_d;
        if (d >= Q) {
          d -= Q;
          ++lr;
        }
      }
#pragma unroll
      for (int k = 0; k < kSbcBatch; ++k) {
        if (at[k] >= 0) {
          bad = bad || !(v[k] - v[k] == 0.0f);
          tile[at[k]] = v[k];
        }
      }
    }
    __syncthreads();
    if (own) {
      const float* col = tile + t;
#pragma unroll 4
      for (int i = 0; i < nrows; ++i) {
        const double dlt = (double)col[i * pitch] - tq;
        less += dlt < 0.0 ? 1 : 0;
        equal += dlt == 0.0 ? 1 : 0;
        s1 = s1 + dlt;
        s2 = s2 + dlt * dlt;
      }
    }
  }
  if (bad) sh_bad = 1;
  __syncthreads();
  const bool out = sh_bad != 0;
  if (own) {
    const long long at = 2 * (r * Q + t);
    counts[at] = out ? 0 : less;
    counts[at + 1] = out ? 0 : equal;
    sums[at] = out ? 0.0 : s1;
    sums[at + 1] = out ? 0.0 : s2;
  }
  if (t == 0) {
    left_out[r] = out ? 1 : 0;
    if (out) atomicAdd(n_left_out, 1ull);        // (an integer count: order-free)
  }
}

}  // namespace
}  // namespace arp

extern "C" int arp_sbc_fold(const float* draws, int64_t n_rep, int64_t n_draws, int32_t Q, int64_t rep_stride,
                            int64_t row_stride, const float* truth, int64_t truth_stride, int32_t* counts, double* sums,
                            uint8_t* left_out, int64_t* n_left_out, void* stream) {
  using namespace arp;
  const std::string who = "arp_sbc_fold";
  if (!draws || !truth || !counts || !sums || !left_out || !n_left_out) {
    set_error(who + ": draws, truth, counts, sums, left_out and n_left_out are required");
    return 1;
  }
  if (Q < 1 || Q > kSbcMaxQ) { set_error(who + ": 1 <= Q <= 256 is required"); return 1; }
  if (n_draws < 1 || n_draws > kSbcMaxDraws) { set_error(who + ": 1 <= n_draws <= 2^24 is required"); return 1; }
  if (n_rep < 1 || n_rep > kSbcMaxRep) { set_error(who + ": 1 <= n_rep <= 2^20 is required"); return 1; }
  if (row_stride < Q) { set_error(who + ": row_stride >= Q is required"); return 1; }
  if (rep_stride / n_draws < row_stride) {       // (rep_stride < n_draws * row_stride, without a product that could overflow)
    set_error(who + ": rep_stride >= n_draws * row_stride is required");
    return 1;
  }
  if (truth_stride < Q) { set_error(who + ": truth_stride >= Q is required"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  ARP_HIP_OK(hipMemsetAsync(n_left_out, 0, sizeof(int64_t), st));
  hipLaunchKernelGGL(sbc_fold_kernel, dim3((unsigned)n_rep), dim3(kSbcThreads), 0, st, draws, (int)n_draws, (int)Q,
                     (long long)rep_stride, (long long)row_stride, truth, (long long)truth_stride, (int*)counts, sums,
                     (unsigned char*)left_out, (unsigned long long*)n_left_out);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
