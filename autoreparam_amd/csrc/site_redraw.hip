// Conditional redraw of recorded draws (include/autoreparam.h: arp_site_redraw): the model's latent site table
// (autoreparam_amd/models.py: ModelSpec.site_table) walked front to back over every draw of a block of the centred trace,
// the elements the caller flags drawn anew from their conditional prior given the rest of the row, the others kept as
// recorded -- what a mixed predictive check (Gelman, Meng, Stern 1996; Marshall, Spiegelhalter 2007) replicates its data
// from: the hyperparameters of the posterior draw, group effects a NEW group would have had under them.  The piece between
// prior_draw.hip (every element drawn, nothing recorded) and the kernels that read a recorded trace (prior.hip, ppc.hip).
// Model-independent; needs no model handle.  Build-specific: the reference has no predictive checks.
//
//   redraw[d] == 0:  out[r][d] = x[r][d], bit for bit
//   redraw[d] != 0:  out[r][d] = site_draw_element(row of r as built so far, d): prior_draw.hip's draw of element d -- its
//                    three forms, its float32 operation order with contraction off, its Philox counter (d, lo32 g, hi32 g,
//                    j) and key, g = draw_offset + r, its 32-attempt rejection loop and its undrawn rule -- ONE copy of
//                    the code, site_draw.h, so the error bounds of prior_draw.hip's header hold here as they stand, against
//                    the exact value of the same float32 parents, the same table and the same Philox words
//
// The parents of a redrawn element are read from the row being built: a redrawn value where the parent is flagged, the
// recorded one where it is not.  The tile is loaded with the recorded value in every unflagged column and with 0 in every
// flagged one: a flagged element reads as 0 until it is redrawn, as "not drawn yet" does in prior_draw.hip, and the
// flagged columns of x never enter a result (they are not even loaded).  With every element flagged the output is
// arp_site_prior_draws' at the same seed and offset, bit for bit; with none it is x.
//
// WHICH elements may be flagged is not policed here.  A selection that is not closed under descent -- an unflagged element
// with a term of non-zero weight at a flagged one, mua redrawn and the m drawn from it kept -- is walked like any other and
// gives rows that are draws from no distribution the model defines: that rule is the host's (diagnostics.redraw_selection).
//
// The value of (d, g) is a function of (seed, d, g), the flags and the draw's own row alone: no result depends on the
// launch shape, on where a call's first draw lies or on the other draws; no atomics; two calls give bitwise equal output.
//
// Shape of the work: prior_draw.hip's.  One wave per workgroup owns a tile of 64 draws in LDS, a draw per lane, pitch
// D | 1 (lane l reads row l at one column: 32 different banks within a half-wave whatever the column).  The tile is filled
// by the wave a row at a time, adjacent lanes on adjacent floats of the trace block (arp_pointwise_loglik's addressing:
// draw r is step r / n_chains, chain r % n_chains; one division per tile, none per element) and stored the same way.  The
// element is uniform per wave, so the table columns are scalar loads; the flags are read ONCE, a byte per lane, and kept
// as four 64-bit ballots in scalar registers, so the flag of an element is a scalar bit test and the branch around an
// unflagged element is taken by the whole wave -- every lane is inside site_draw_element's __all together, dead lanes of
// a ragged tile included.
//
// Cost: the draws of the flagged elements as in prior_draw.hip (Philox, logf, sqrtf, cospif, expf per Normal element),
// plus one read of the unflagged part of the block and one write of all of it; measured next to arp_site_prior_draws:
// DESIGN.md section 6.
//
// Things that go wrong quietly here:
//  * Reads past the end.  A load is issued for (r < n_samples * n_chains, d < D, d unflagged) only; nothing is read past
//    x[(n_samples - 1) * row_stride + n_chains * D - 1], and the padding between rows of x is never read.  Columns
//    d >= D of out and rows past the draws are never stored.  Dead lanes of the last ragged tile hold 0 in the unflagged
//    columns, draw like the others (their g is past the call's range) and store nothing.
//  * A NaN or an infinity in an unflagged column is a value like any other: it is copied, and a flagged element that
//    hangs on it is NaN (also through a term of weight 0, as in arp_site_logprior).  Nothing is masked here; the
//    kernels that read the output mask a draw with a non-finite element themselves.
//  * The table's indices are clamped into [0, D); a form other than 1 or 2 is read as 0 (site_draw.h).
//  * out must not overlap x (out == x is refused; a partial overlap is the caller's to avoid).
#include "arp_device.h"
#include "obs_table.h"
#include "site_draw.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kRows = 8;                         // rows of the tile whose loads are in flight before they are stored

// bit d of the four ballots (all wave-uniform when d is)
__device__ __forceinline__ bool flag_of(int d, unsigned long long m0, unsigned long long m1, unsigned long long m2,
                                        unsigned long long m3) {
  const unsigned long long m = d < 64 ? m0 : d < 128 ? m1 : d < 192 ? m2 : m3;
  return ((m >> (d & 63)) & 1ull) != 0;
}

__global__ __launch_bounds__(kObsDraws) void site_redraw_kernel(
    const float* __restrict__ x, long long R, unsigned n_chains, int D, long long stride, const int* __restrict__ form,
    const int* __restrict__ loc_idx, const float* __restrict__ loc_w, const float* __restrict__ loc0,
    const int* __restrict__ scale_idx, const float* __restrict__ scale_w, const float* __restrict__ log_scale0,
    const unsigned char* __restrict__ redraw, unsigned key0, unsigned key1, unsigned long long draw_offset,
    float* __restrict__ out, long long out_stride, unsigned char* __restrict__ undrawn) {
  extern __shared__ float tile[];                // [64][D | 1]
  const int lane = threadIdx.x;
  const int Dp = D | 1;
  const long long r0 = (long long)blockIdx.x * kObsDraws;
  const int nrows = (int)min((long long)kObsDraws, R - r0);
  const unsigned long long g = draw_offset + (unsigned long long)(r0 + lane);
  const unsigned g_lo = (unsigned)g, g_hi = (unsigned)(g >> 32);
  // The flags of the (at most 255) elements, read once.  This lane's columns are d = lane + 64 c: its flag of chunk c is
  // the predicate it hands ballot c, and ballot c holds the flags of d = 64 c ... 64 c + 63 for the walk below.
  const bool f0 = lane < D && redraw[min(lane, D - 1)] != 0;
  const bool f1 = lane + 64 < D && redraw[min(lane + 64, D - 1)] != 0;
  const bool f2 = lane + 128 < D && redraw[min(lane + 128, D - 1)] != 0;
  const bool f3 = lane + 192 < D && redraw[min(lane + 192, D - 1)] != 0;
  const unsigned long long m0 = __ballot(f0), m1 = __ballot(f1), m2 = __ballot(f2), m3 = __ballot(f3);
  // The tile, a row at a time: lane l takes columns l, l + 64, ... of every row -- adjacent lanes, adjacent floats of the
  // block.  A dead row and a flagged column take 0 without a load.  Where draw r0 starts in the block is the kernel's one
  // division; the rows after it follow by addition (wave-uniform).  kRows rows a pass, loads first: one wave has nobody
  // to hide a load's latency behind but its own next loads.
  const unsigned step0 = (unsigned)r0 / n_chains, chain0 = (unsigned)r0 - step0 * n_chains;
  const long long at0 = (long long)step0 * stride + (long long)chain0 * D;
  const long long next_step = stride - (long long)n_chains * D;
  const int nc = (D + kObsDraws - 1) / kObsDraws;
  for (int c = 0; c < nc; ++c) {
    const int d = lane + c * kObsDraws;
    const bool mine = d < D;
    const bool keep = mine && !(c == 0 ? f0 : c == 1 ? f1 : c == 2 ? f2 : f3);
    unsigned chain = chain0;
    long long at = at0;
#pragma unroll 1
    for (int lr0 = 0; lr0 < kObsDraws; lr0 += kRows) {
      float v[kRows];
#pragma unroll
      for (int u = 0; u < kRows; ++u) {
        v[u] = 0.0f;
        if (keep && lr0 + u < nrows) v[u] = x[at + d];
        at += D;
        if (++chain == n_chains) { chain = 0; at += next_step; }
      }
#pragma unroll
      for (int u = 0; u < kRows; ++u)
        if (mine) tile[(lr0 + u) * Dp + d] = v[u];
    }
  }
  __syncthreads();
  float* row = tile + lane * Dp;
  bool failed = false;
  for (int k = 0; k < D; ++k) {
    if (flag_of(k, m0, m1, m2, m3)) {            // (wave-uniform: the whole wave draws, or none of it)
      row[k] = site_draw_element(row, k, D, form, loc_idx, loc_w, loc0, scale_idx, scale_w, log_scale0, g_lo, g_hi, key0, key1, failed);
    }
  }
  if (undrawn && lane < nrows) undrawn[r0 + lane] = failed ? 1 : 0;
  __syncthreads();
  // the tile goes out as it came in: a row at a time, adjacent lanes on adjacent floats
  for (int c = 0; c < nc; ++c) {
    const int d = lane + c * kObsDraws;
    if (d < D) {
#pragma unroll 4
      for (int lr = 0; lr < nrows; ++lr) out[(r0 + lr) * out_stride + d] = tile[lr * Dp + d];
    }
  }
}

}  // namespace
}  // namespace arp

extern "C" int arp_site_redraw(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                               const int32_t* form, const int32_t* loc_idx, const float* loc_w, const float* loc0,
                               const int32_t* scale_idx, const float* scale_w, const float* log_scale0, const uint8_t* redraw,
                               uint64_t seed, int64_t draw_offset, float* out, int64_t out_stride, uint8_t* undrawn,
                               void* stream) {
  using namespace arp;
  const char* name = "arp_site_redraw";
  const std::string who = name;
  if (!x || !form || !loc_idx || !loc_w || !loc0 || !scale_idx || !scale_w || !log_scale0 || !redraw || !out) {
    set_error(who + ": x, the table (form, loc_idx, loc_w, loc0, scale_idx, scale_w, log_scale0), redraw and out are required");
    return 1;
  }
  if (D < 1 || D > kObsMaxD) { set_error(who + ": 1 <= D <= 255 is required"); return 1; }
  if (!trace_shape_ok(n_samples, n_chains, D, name)) return 1;
  if (row_stride < n_chains * D) { set_error(who + ": row_stride >= n_chains * D is required"); return 1; }
  const long long R = n_samples * n_chains;
  if (R > kPdMaxR) { set_error(who + ": at most 2^24 draws (n_samples * n_chains) are taken"); return 1; }
  if (out_stride < D) { set_error(who + ": out_stride >= D is required"); return 1; }
  if (draw_offset < 0) { set_error(who + ": draw_offset >= 0 is required"); return 1; }
  if (out == x) { set_error(who + ": out must not be x (the rows are rebuilt from the recorded ones)"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(site_redraw_kernel, dim3(blocks_for(R, kObsDraws)), dim3(kObsDraws), tile_lds_bytes(D), st, x, R,
                     (unsigned)n_chains, (int)D, (long long)row_stride, form, loc_idx, loc_w, loc0, scale_idx, scale_w, log_scale0,
                     (const unsigned char*)redraw, (unsigned)seed, (unsigned)(seed >> 32), (unsigned long long)draw_offset, out,
                     (long long)out_stride, (unsigned char*)undrawn);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
