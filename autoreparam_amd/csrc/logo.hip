// Group log-likelihood of recorded draws (include/autoreparam.h: arp_group_loglik): per GROUP of observations and draw, the
// joint log-likelihood of the group's observations at the recorded state (lc, the CONDITIONAL form) and, for Normal data,
// the same with the group's own latent element integrated against its conditional prior (lm, the MARGINAL form) -- what
// PSIS leave-one-group-out cross-validation is computed from (psis.hip reads either in the place of a pointwise
// log-likelihood; Merkle, Furr, Rabe-Hesketh 2019 for why the marginal form is the one to trust).  The groups, `order` /
// `group_start`, their clamps, the walk and which wave owns which group: group_table.h.  slope[j] runs parallel to order:
// the sum of the weights with which observation order[j] reads the group's element, elem[g] that element's index in the
// state.  Model-independent; the table, the tile of draws, eta_n and s_n: obs_table.h; the site chains: site_table.h.
//
// Build-specific: the reference evaluates joint densities only.
//
// Per (n, r), float32, contraction off -- loglik.hip's operations, restated (moving lines in that kernel cost 1 %:
// obs_table.h), so that the value is bit for bit what arp_pointwise_loglik writes:
//
//   Normal:     z = (y_n - eta_n) exp(-s_n),  ll = -0.5 z^2 - s_n - 0.5 log(2 pi);   b = slope exp(-s_n), b z, b b
//   Bernoulli:  ll = y_n eta_n - (max(eta_n, 0) + log1p(exp(-|eta_n|)))
//
// Per (group, draw), float64, in order's sequence:  S_ll += ll,  S_bz += b z,  S_bb += b b.   lc = (float) S_ll.
//
// The marginal form.  Let t = x[elem[g]] be the group's element, t0 its recorded value, and the rest of the row as
// recorded.  The group's observations read t linearly, eta_n(t0 + d) = eta_n + slope_n d, and -- the caller's rule
// (diagnostics.marginal_selection) -- no s_n and no other site reads it, so z_n(t0 + d) = z_n - b_n d and
//
//   sum_n ll_n(t0 + d) = S_ll + d S_bz - 0.5 d^2 S_bb.
//
// The element's conditional prior is N(loc, exp(sj)) with loc and sj its site chains over the row; with tau = exp(-2 sj)
// and m = t0 - loc,  log N(t0 + d | loc, exp(sj)) = -0.5 (m + d)^2 tau + 0.5 log tau - 0.5 log(2 pi).  The exponent of
// the integrand is therefore a quadratic in d,
//
//   S_ll - 0.5 m^2 tau + 0.5 log tau - 0.5 log(2 pi) + d q - 0.5 d^2 P,     P = S_bb + tau,  q = S_bz - m tau,
//
// and  int exp(d q - 0.5 d^2 P) dd = sqrt(2 pi / P) exp(q^2 / (2 P)),  so
//
//   lm = log int exp(sum_n ll_n(t0 + d)) N(t0 + d | loc, exp(sj)) dd
//      = S_ll - 0.5 (m^2 tau - q^2 / P) - 0.5 log1p(S_bb / tau)                  (0.5 log tau - 0.5 log P = -0.5 log(P / tau)).
//
// Centred at the recorded draw: t0 is a draw from the element's conditional posterior, whose mode is d = q / P, so q is
// a residual, not a difference of large terms -- expanding about loc instead would subtract two squares of the size of
// (loc / exp(sj))^2.  Everything behind the three sums is float64: tau = exp(-2 sj), m, P, q and the line above.
//
// Shape of the work: group_table.h's; slope, elem and the site rows are scalar loads like order (the table pointers are
// separate __restrict__ arguments).  A wave carries the three sums in registers; a lane stores one float per output and
// group, 256 adjacent bytes a wave.  A row depends neither on [g0, g1), nor on the tiling, nor on how the draws are spread
// over calls.  Without lm (the kernel's other instantiation) b, b z and b b are not computed and lc is bitwise the same.
//
// Cost.  Per (n, r) loglik.hip's (one expf, or expf and log1pf) and, with lm, two products more; per (group, r) two site
// chains, one exp, one log1p and one division in float64.  Against ppc_group.hip: no Philox, logf, sqrtf, cospif, erfcf,
// and 4 or 8 bytes stored where that stores 64.  Measured: DESIGN.md section 6.
//
// Arithmetic.  u = 2^-24.  Per observation, with A_n = sum_t |w_t x_t| and loglik.hip's Normal bound
//   e_n = u [ T A_n exp(-s) |z| + z^2 (5 + |s|) + 3 |s| + |ll| ]:
// exp(-s) is within relative u (2 + |s|) (expf: 2 u; s: one addition), so b within u (3 + |s|) |b|; z within
// u [ T A_n exp(-s) + |z| (4 + |s|) ]; the two products round once more:
//   |d (b z)| <= u [ T A_n exp(-s) |b| + |b z| (8 + 2 |s|) ],     |d (b b)| <= u b^2 (7 + 2 |s|).
// The float64 sums add (n_g + 4) 2^-53 of their terms' magnitudes: not first order.  With E_ll, E_bz, E_bb the sums of
// the three per-observation bounds over the group, site_table.h's |d loc| <= 3 u A_loc and |d sj| <= 3 u A_s (so
// |d m| <= 3 u A_loc, |d tau| <= 6 u A_s tau) and c = m + q / P = (m S_bb + S_bz) / P, the partial derivatives of lm are
//   d/dS_ll = 1,  d/dS_bz = q / P,  d/dS_bb = -0.5 (q^2 / P^2 + 1 / P),  d/dm = -tau c,  d/dtau = 0.5 (S_bb / (tau P) - c^2),
// hence, to first order against the exact value of the same float32 inputs,
//
//   |lm_dev - lm| <= E_ll + |q / P| E_bz + 0.5 (q^2 / P^2 + 1 / P) E_bb + 3 u A_loc tau |c| + 3 u A_s (S_bb / P + c^2 tau) + u |lm|
//
// (the last term: the rounding of the float64 result to float32).  lc is exact given the float32 ll: (float) of their
// float64 sum in order's sequence.
//
// Things that go wrong quietly here:
//  * A tau that is 0, infinite or NaN (sj beyond +-354, or a NaN chain) makes lm non-finite; it is written as it comes
//    and PSIS reports the group as not finite.
//  * An empty group writes lc = lm = 0, by select (the formula would give 0 - 0 only for a finite tau).
//  * A draw that is left out writes 0 in both, by select (0 * inf is NaN).
//  * Clamped order and group_start entries, a wave without a group: group_table.h.  elem[g] is clamped into [0, D)
//    before it addresses the tile or the site table: a wrong number, never a read past the end.
//  * Dead lanes of the last ragged tile compute on a zero row and store nothing.
//  * Bernoulli data has no closed form: lm with kind ARP_OBS_BERNOULLI is refused on the host, not approximated.
#include "arp_device.h"
#include "group_table.h"
#include "site_table.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr float kHalfLog2PiF = 0.9189385332046727f;

template <bool Marginal>
__global__ __launch_bounds__(kObsThreads) void logo_kernel(
    const float* __restrict__ x, long long R, unsigned n_chains, int D, long long stride, int kind, int T,
    const int* __restrict__ idx, const float* __restrict__ w, const float* __restrict__ y,
    const int* __restrict__ scale_idx, const float* __restrict__ log_scale, int n_obs, const int* __restrict__ order,
    const float* __restrict__ slope, int n_grouped, const int* __restrict__ group_start, const int* __restrict__ elem,
    long long g0, long long g1, const int* __restrict__ site_loc_idx, const float* __restrict__ site_loc_w,
    const float* __restrict__ site_loc0, const int* __restrict__ site_scale_idx, const float* __restrict__ site_scale_w,
    const float* __restrict__ site_log_scale0, float* __restrict__ lc, float* __restrict__ lm, long long out_stride,
    unsigned char* __restrict__ mask, unsigned long long* __restrict__ n_masked) {
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

  const float* row = tile + lane * (D | 1);
  const long long hop = (long long)gridDim.y * kObsWaves;
  for (long long grp = g0 + (long long)blockIdx.y * kObsWaves + wave; grp < g1; grp += hop) {
    const int jb = group_begin(group_start, grp, n_grouped);
    const int je = group_end(group_start, grp, jb, n_grouped);
    double s_ll = 0.0, s_bz = 0.0, s_bb = 0.0;
    int next = first_member(order, jb, je);
    for (int j = jb; j < je; ++j) {
      const long long n = member_obs(next, n_obs);
      next = next_member(order, j, je, next);
      const float eta = obs_eta(row, idx, w, n, T, D);
      const float yn = y[n];
      float v;
      if (kind == 0) {
        const float s = obs_log_scale(row, scale_idx, log_scale, n, D);
        const float ems = expf(-s);
        const float z = (yn - eta) * ems;
        v = -0.5f * (z * z) - s - kHalfLog2PiF;
        if (Marginal) {
          const float b = slope[j] * ems;
          const float bz = b * z, bb = b * b;
          s_bz += (double)bz;
          s_bb += (double)bb;
        }
      } else {
        v = yn * eta - (fmaxf(eta, 0.0f) + log1pf(expf(-fabsf(eta))));
      }
      s_ll += (double)v;
    }
    const long long at = (grp - g0) * out_stride + r0 + lane;
    if (lc && live) lc[at] = bad ? 0.0f : (float)s_ll;
    if (Marginal) {
      const int d = min(max(elem[grp], 0), D - 1);
      const float loc = site_chain(row, site_loc_idx, site_loc_w, site_loc0[d], d, D);
      const float sj = site_chain(row, site_scale_idx, site_scale_w, site_log_scale0[d], d, D);
      const double tau = exp(-2.0 * (double)sj);
      const double m = (double)row[d] - (double)loc;
      const double P = s_bb + tau;
      const double q = s_bz - m * tau;
      const double v = s_ll - 0.5 * (m * m * tau - q * q / P) - 0.5 * log1p(s_bb / tau);
      if (live) lm[at] = (bad || jb == je) ? 0.0f : (float)v;
    }
  }
}

}  // namespace
}  // namespace arp

extern "C" int arp_group_loglik(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride, int32_t kind,
                                const int32_t* idx, const float* w, int32_t T, const float* y, const int32_t* scale_idx,
                                const float* log_scale, int64_t n_obs, const int32_t* order, const float* slope,
                                int64_t n_grouped, const int32_t* group_start, const int32_t* elem, int64_t n_groups, int64_t g0,
                                int64_t g1, const int32_t* site_loc_idx, const float* site_loc_w, const float* site_loc0,
                                const int32_t* site_scale_idx, const float* site_scale_w, const float* site_log_scale0, float* lc,
                                float* lm, int64_t out_stride, uint8_t* mask, int64_t* n_masked, void* stream) {
  using namespace arp;
  const char* name = "arp_group_loglik";
  const std::string who = name;
  if (!x || !idx || !w || !y || !scale_idx || !log_scale || !group_start || !mask || !n_masked) {
    set_error(who + ": x, the table (idx, w, y, scale_idx, log_scale), group_start, mask and n_masked are required");
    return 1;
  }
  if (!slope || !elem) { set_error(who + ": slope and elem are required"); return 1; }
  if (!lc && !lm) { set_error(who + ": lc or lm is required (both outputs are NULL)"); return 1; }
  if (lm && (!site_loc_idx || !site_loc_w || !site_loc0 || !site_scale_idx || !site_scale_w || !site_log_scale0)) {
    set_error(who + ": the site table (site_loc_idx, site_loc_w, site_loc0, site_scale_idx, site_scale_w, site_log_scale0) is "
                    "required with lm");
    return 1;
  }
  if (!group_call_ok(name, n_obs, n_grouped, order, n_groups, g0, g1)) return 1;
  if (!table_call_ok(name, n_samples, n_chains, D, row_stride, kind, T, 0, n_obs)) return 1;
  if (lm && kind != 0) {
    set_error(who + ": lm is for kind ARP_OBS_NORMAL only (the Bernoulli marginal has no closed form)");
    return 1;
  }
  const long long R = n_samples * n_chains;
  if (out_stride < R) { set_error(who + ": out_stride >= n_samples * n_chains is required"); return 1; }
  const long long ntiles = (R + kObsDraws - 1) / kObsDraws;
  const long long shares = shares_of(ntiles, g1 - g0);
  hipStream_t st = (hipStream_t)stream;
  ARP_HIP_OK(hipMemsetAsync(n_masked, 0, sizeof(int64_t), st));
  auto kernel = lm ? logo_kernel<true> : logo_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)ntiles, (unsigned)shares), dim3(kObsThreads), tile_lds_bytes(D), st, x, R,
                     (unsigned)n_chains, (int)D, (long long)row_stride, (int)kind, (int)T, idx, w, y, scale_idx, log_scale, (int)n_obs,
                     order, slope, (int)n_grouped, group_start, elem, (long long)g0, (long long)g1, site_loc_idx, site_loc_w,
                     site_loc0, site_scale_idx, site_scale_w, site_log_scale0, lc, lm, (long long)out_stride,
                     (unsigned char*)mask, (unsigned long long*)n_masked);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
