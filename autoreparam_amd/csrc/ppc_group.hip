// Grouped predictive check (include/autoreparam.h: arp_group_predictive_check): the replicated observations of
// arp_predictive_check, folded per GROUP of observations and draw into the eight per-draw test statistics -- which county
// does the model fail to produce?  The groups, `order` / `group_start`, their clamps, the walk and which wave owns which
// group: group_table.h.  Model-independent; the table, the tile of draws, eta_n and s_n: obs_table.h; the per-(n, r) body:
// ppc_terms.h, which ppc.hip calls too, so y_rep of (n, r) is bit for bit arp_predictive_check's under the same seed and
// draw offset.
//
// Build-specific: the reference has no predictive checks.
//
// Random numbers.  ppc.hip's: one philox4x32_10(counter (n, lo32 g, hi32 g, 0), key (lo32 seed, hi32 seed)) per (n, r),
// g = draw_offset + r, n the observation's index in the WHOLE table (what order[j] holds), never its place in the group.
//
// Shape of the work: group_table.h's.  A wave carries its group's eight statistics in one set of registers: sums in
// float64, min and max in float32, as ppc_kernel's; a lane stores its row of eight doubles (64 adjacent bytes, the wave
// 4 096) once per group.  Two calls, a call over a sub-range of the groups and two calls over halves of the draws give
// bitwise equal rows.
//
// Cost.  Per (n, r) ppc.hip's (Philox, logf, sqrtf, cospif, two expf and erfcf, or expf, log1pf and a division) without
// its per-observation butterfly; the staging of the tile is paid once per workgroup, so a call with few, small groups (8
// schools: eight groups of one) is all staging.  Measured next to arp_predictive_check: DESIGN.md section 6.
//
// Arithmetic.  ppc.hip's per-(n, r) values and bounds; columns 0 - 3 and 7 are exact functions of the float32 y_rep
// (float64 sums of at most 2^31 float32 values and of their exact float64 squares, in ascending n).
//
// Things that go wrong quietly here:
//  * An empty group writes (0, 0, +inf, -inf, 0, 0, 0, 0): the fold's start values, not zeros -- min and max of nothing.
//  * A draw that is left out writes a zero row in every group, by select (ppc.hip: 0 * inf is NaN).
//  * Clamped order and group_start entries, a wave without a group: group_table.h.  Dead lanes of the last ragged tile
//    compute on a zero row and store nothing.
#include "arp_device.h"
#include "group_table.h"
#include "ppc_terms.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

__global__ __launch_bounds__(kObsThreads) void ppc_group_kernel(
    const float* __restrict__ x, long long R, unsigned n_chains, int D, long long stride, int kind, int T,
    const int* __restrict__ idx, const float* __restrict__ w, const float* __restrict__ y,
    const int* __restrict__ scale_idx, const float* __restrict__ log_scale, int n_obs, const int* __restrict__ order,
    int n_grouped, const int* __restrict__ group_start, long long g0, long long g1, unsigned key0, unsigned key1,
    unsigned long long draw_offset, double* __restrict__ group_stats, unsigned char* __restrict__ mask,
    unsigned long long* __restrict__ n_masked) {
  extern __shared__ float tile[];                // [64][D | 1]
  __shared__ int sh_bad[kObsDraws];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long r0 = (long long)blockIdx.x * kObsDraws;
  const int nrows = (int)min((long long)kObsDraws, R - r0);
  stage_tile<true>(x, r0, nrows, n_chains, D, stride, tile, sh_bad);
  const bool live = lane < nrows;
  const bool bad = sh_bad[lane] != 0;
  if (blockIdx.y == 0 && wave == 0) write_mask(live, bad, lane, r0, mask, n_masked);

  const unsigned long long g = draw_offset + (unsigned long long)(r0 + lane);
  const unsigned g_lo = (unsigned)g, g_hi = (unsigned)(g >> 32);
  const float* row = tile + lane * (D | 1);
  const long long hop = (long long)gridDim.y * kObsWaves;
  for (long long grp = g0 + (long long)blockIdx.y * kObsWaves + wave; grp < g1; grp += hop) {
    const int jb = group_begin(group_start, grp, n_grouped);
    const int je = group_end(group_start, grp, jb, n_grouped);
    double a_y = 0.0, a_yy = 0.0, a_dr = 0.0, a_do = 0.0, a_mu = 0.0, a_n = 0.0;
    float a_min = __builtin_inff(), a_max = -__builtin_inff();
    int next = first_member(order, jb, je);
    for (int j = jb; j < je; ++j) {
      const long long n = member_obs(next, n_obs);
      next = next_member(order, j, je, next);
      const PpcTerms pc = ppc_terms(row, kind, T, D, idx, w, y, scale_idx, log_scale, n, g_lo, g_hi, key0, key1);
      a_y += (double)pc.yr;
      a_yy += (double)pc.yr * (double)pc.yr;
      a_dr += (double)pc.dev_r;
      a_do += (double)pc.dev_o;
      a_mu += (double)pc.pt.mu;
      a_n += 1.0;
      a_min = fminf(a_min, pc.yr);
      a_max = fmaxf(a_max, pc.yr);
    }
    if (live) {
      double* pd = group_stats + ((grp - g0) * R + r0 + lane) * kPcCols;
      pd[0] = bad ? 0.0 : a_y; pd[1] = bad ? 0.0 : a_yy; pd[2] = bad ? 0.0 : (double)a_min; pd[3] = bad ? 0.0 : (double)a_max;
      pd[4] = bad ? 0.0 : a_dr; pd[5] = bad ? 0.0 : a_do; pd[6] = bad ? 0.0 : a_mu; pd[7] = bad ? 0.0 : a_n;
    }
  }
}

}  // namespace
}  // namespace arp

extern "C" int arp_group_predictive_check(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                                          int32_t kind, const int32_t* idx, const float* w, int32_t T, const float* y,
                                          const int32_t* scale_idx, const float* log_scale, int64_t n_obs,
                                          const int32_t* order, int64_t n_grouped, const int32_t* group_start, int64_t n_groups,
                                          int64_t g0, int64_t g1, uint64_t seed, int64_t draw_offset, double* group_stats,
                                          uint8_t* mask, int64_t* n_masked, void* stream) {
  using namespace arp;
  const char* name = "arp_group_predictive_check";
  const std::string who = name;
  if (!x || !idx || !w || !y || !scale_idx || !log_scale || !group_start || !group_stats || !mask || !n_masked) {
    set_error(who + ": x, the table (idx, w, y, scale_idx, log_scale), group_start, group_stats, mask and n_masked are required");
    return 1;
  }
  if (!group_call_ok(name, n_obs, n_grouped, order, n_groups, g0, g1)) return 1;
  if (!table_call_ok(name, n_samples, n_chains, D, row_stride, kind, T, 0, n_obs)) return 1;
  if (draw_offset < 0) { set_error(who + ": draw_offset >= 0 is required"); return 1; }
  const long long R = n_samples * n_chains;
  const long long ntiles = (R + kObsDraws - 1) / kObsDraws;
  const long long shares = shares_of(ntiles, g1 - g0);
  hipStream_t st = (hipStream_t)stream;
  ARP_HIP_OK(hipMemsetAsync(n_masked, 0, sizeof(int64_t), st));
  hipLaunchKernelGGL(ppc_group_kernel, dim3((unsigned)ntiles, (unsigned)shares), dim3(kObsThreads), tile_lds_bytes(D), st, x, R,
                     (unsigned)n_chains, (int)D, (long long)row_stride, (int)kind, (int)T, idx, w, y, scale_idx, log_scale, (int)n_obs,
                     order, (int)n_grouped, group_start, (long long)g0, (long long)g1, (unsigned)seed, (unsigned)(seed >> 32),
                     (unsigned long long)draw_offset, group_stats, (unsigned char*)mask, (unsigned long long*)n_masked);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
