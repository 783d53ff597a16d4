// Ancestral draws from the prior (include/autoreparam.h: arp_site_prior_draws): the model's latent site table
// (autoreparam_amd/models.py: ModelSpec.site_table) walked front to back, n_draws times -- the generating twin of
// arp_site_logprior (prior.hip), what a prior predictive check and the prior-to-posterior contraction are computed from.
// Model-independent; needs no model handle.  Build-specific: the reference never draws from a prior.  The draw of one
// element, as specified below, is site_draw.h's site_draw_element, which site_redraw.hip walks the same table with.
//
//   loc_d = loc0[d] + sum_t loc_w[d][t] x[loc_idx[d][t]],   s_d = log_scale0[d] + sum_t scale_w[d][t] x[scale_idx[d][t]]
//   form 0 (Normal, scale exp(s)):       x_d = loc_d + exp(s_d) z
//   form 1 (Normal, scale softplus(s)):  x_d = loc_d + sigma z,  sigma = max(s_d, 0) + log1p(exp(-|s_d|))
//   form 2 (log of a Gamma variable):    x_d = log g,  g ~ Gamma(shape k = loc0[d], rate exp(s_d))  (the loc terms are not read)
//
// over the elements of the same draw that were drawn before d (site_table.h's chain; the table is in ancestral order, so
// that is every element a term of non-zero weight points at).  An element that is not drawn yet reads as 0.
//
// Random numbers.  Counter based, as ppc.hip: philox4x32_10(counter (d, lo32 g, hi32 g, j), key (lo32 seed, hi32 seed)),
// g = draw_offset + r.  The Normal forms take j = 0 and words 0 and 1: z = sqrt(-2 log u') cospi(2 a) with ppc.hip's u' in
// (0, 1] and its angle a in [1, 2) revolutions, through the device library's logf, sqrtf and cospif.  The value of (d, g) is
// a function of (seed, d, g) and of the draw's earlier elements alone: no result depends on the launch shape, on where a
// call's first draw lies or on the other draws; no atomics.
//
// Form 2 is Marsaglia and Tsang's method (2000) carried out in log space -- at shape 0.5 a Gamma variable has mass far
// below float32's normal range, its logarithm has not.  With boost = k < 1, a = boost ? k + 1 : k, dd = a - 1 / 3,
// c = 1 / sqrt(9 dd), attempt j = 0 ... 31 takes the words of counter word 1 + j:
//   z from words (0, 1) as above;  t = 1 + c z, rejected if t <= 0;  U = fma((float)w2, 2^-32, 2^-33)
//   accepted iff  log U < m_rhs = ((0.5 z^2 + dd) - dd t^3) + (3 dd) log t            (t^3 = (t t) t)
//   x_d = ((log dd + 3 log t) + (boost ? log(U_b) / k : 0)) - s_d,  U_b formed as U from w3 of the accepting attempt
// (dd t^3 is Gamma(a, 1); U_b^(1 / k) takes it to shape k; the rate divides).  An attempt accepts with probability above
// 0.95 at every shape, so 32 rejections in a row (below 1e-41) are there for determinism, not for use: x_d = NaN and
// undrawn[r] = 1.  k <= 0 or a non-finite k gives NaN without an attempt (and without undrawn).
//
// Shape of the work.  One wave per workgroup owns a tile of 64 draws in LDS, a draw per lane, pitch D | 1 (obs_table.h's
// tile and its bank argument: lane l reads row l at one column, 32 different banks within a half-wave).  The element is
// uniform per wave, so the table columns -- separate __restrict__ arguments -- are scalar loads.  Each lane writes x_d into
// its own row and reads its parents from it; the tile goes to global memory at the end, adjacent lanes storing adjacent
// floats of a row.  A single wave, so the four of a workgroup do not wait for one another's rejections, and at D = 255 two
// tiles fit a CU's LDS.  The rejection loop runs until every lane of the wave has accepted.
//
// Arithmetic.  float32, contraction off; library functions at the OpenCL full-profile limits ppc.hip uses (log 3, exp 3,
// sqrt 3, cospi 4, log1p 2 ulp; one ulp <= 2 u relative, u = 2^-24).  To first order against the exact value of the same
// float32 parents, the same table and the same Philox words, with A_loc, A_s as prior.hip's (|loc_dev - loc| <= 3 u A_loc,
// |s_dev - s| <= 3 u A_s) and |z_dev - z| <= 18 u |z| (ppc.hip):
//
//   form 0:  |x_dev - x| <= u [ 3 A_loc + exp(s) |z| (25 + 3 A_s) + |x| ]
//   form 1:  |x_dev - x| <= u [ 3 A_loc + |z| (3 A_s + 6 + 20 sigma) + |x| ]
//   form 2:  |x_dev - x| <= u [ 5 + 6 |log dd| + 3 T + 21 |log t| + |L| + (1 + 7 |log U_b|) / k (boost only) + |L + B| + 3 A_s + |x| ]
//            T = 29 |t - 1| / t + 1,  L = log dd + 3 log t,  B = boost ? log(U_b) / k : 0
//   accept margin m = m_rhs - log U:
//            E_m = u [ 19 z^2 + 6 dd + 8 dd t^3 + 39 dd |log t| + |0.5 z^2 + dd - dd t^3| + |m_rhs| + 1 + 6 |log U|
//                      + 3 dd |1 - t^3| T ]
//
// (Form 0: exp(s) carries exp's 6 u and s's 3 u A_s relatively, the product with z 18 u more and its own rounding; the
// sum rounds by u |x| and carries loc's 3 u A_loc.
// Form 1: softplus has slope at most 1; exp(-|s|) <= 1 carries 6 u, of which log1p passes on at most half; log1p <= log 2
// adds 4 u log 2 and the sum u sigma: dsigma <= u (3 A_s + 6 + sigma); then as form 0 with 18 + 1 on sigma |z|.
// Form 2: k + 1 rounds by u a, the constant 1 / 3 is off by at most u / 3 and the difference rounds by u dd; with
// a <= 1.5 dd that is 5 u dd.  c: half of dd's 5 u, half of the product 9 dd's u, sqrt's 6 u and the division: 10 u.
// t: the product c z carries 10 + 18 + 1 and the sum rounds by u t: dt <= u (29 |t - 1| + t) = u t T.  log t is within
// dt / t + 6 u |log t|, three times that and the product's 3 u |log t| make 3 u T + 21 u |log t|; log dd is within
// 5 u + 6 u |log dd|; L rounds once.  log U_b: U_b is one rounding off, u, and log's 6 u |log U_b|; the division rounds
// once more.  The last two sums round by u |L + B| and u |x|; s carries 3 u A_s.
// E_m: 0.5 z^2 is within 37 u of itself, i.e. 18.5 u z^2; its sum with dd rounds (u (0.5 z^2 + dd)) and carries dd's 5 u dd;
// dd t^3 carries dd's 5 u, the two products of t^3 and its own: 8 u dd t^3 beside t's error; 3 dd rounds once more than
// dd (6 u), log t's 6 u and the product make 13 u (3 dd |log t|) beside t's error; t's error reaches m through
// d/dt (-dd t^3 + 3 dd log t) = 3 dd (1 - t^3) / t; the two outer sums round by u |0.5 z^2 + dd - dd t^3| and u |m_rhs|;
// log U is within u + 6 u |log U|.)
// An attempt with |m| <= E_m is UNDECIDED: float32 and float64 may disagree about accepting it, and from there on the two
// draw different values for this element and for what descends from it.  Per attempt that has probability about
// 2 E_m (the density of -log U is at most 1), 1e-5 or so at the shapes served.
//
// Things that go wrong quietly here:
//  * Rows of x past the draws, columns d >= D: never stored.  Dead lanes of the last ragged tile draw like the others (their
//    g is past the call's range) and store nothing.
//  * The table's indices are clamped into [0, D) (the caller's checks, diagnostics.upload_site_table, keep them there and
//    in ancestral order); a form other than 1 or 2 is read as 0.
//  * A term of weight 0 multiplies what it points at: 0 times an infinite parent is NaN, as in arp_site_logprior.
#include "arp_device.h"
#include "obs_table.h"
#include "site_draw.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

__global__ __launch_bounds__(kObsDraws) void prior_draw_kernel(int D, const int* __restrict__ form, const int* __restrict__ loc_idx,
                                                               const float* __restrict__ loc_w, const float* __restrict__ loc0,
                                                               const int* __restrict__ scale_idx,
                                                               const float* __restrict__ scale_w,
                                                               const float* __restrict__ log_scale0, long long R, unsigned key0,
                                                               unsigned key1, unsigned long long draw_offset,
                                                               float* __restrict__ x, long long stride,
                                                               unsigned char* __restrict__ undrawn) {
  extern __shared__ float tile[];                // [64][D | 1]
  const int lane = threadIdx.x;
  const int Dp = D | 1;
  const long long r0 = (long long)blockIdx.x * kObsDraws;
  const int nrows = (int)min((long long)kObsDraws, R - r0);
  const unsigned long long g = draw_offset + (unsigned long long)(r0 + lane);
  const unsigned g_lo = (unsigned)g, g_hi = (unsigned)(g >> 32);
  float* row = tile + lane * Dp;
  for (int d = 0; d < D; ++d) row[d] = 0.0f;     // an element that is not drawn yet reads as 0
  bool failed = false;
  for (int d = 0; d < D; ++d) {
    row[d] = site_draw_element(row, d, D, form, loc_idx, loc_w, loc0, scale_idx, scale_w, log_scale0, g_lo, g_hi, key0, key1, failed);
  }
  if (undrawn && lane < nrows) undrawn[r0 + lane] = failed ? 1 : 0;
  __syncthreads();
  // element e = lane + 64 a of the tile is (row e / D, column e % D): adjacent lanes, adjacent floats
  const int nelem = nrows * D;
  for (int e = lane; e < nelem; e += kObsDraws) {
    const int lr = (int)((unsigned)e / (unsigned)D), d = e - lr * D;
    x[(r0 + lr) * stride + d] = tile[lr * Dp + d];
  }
}

}  // namespace
}  // namespace arp

extern "C" int arp_site_prior_draws(int32_t D, const int32_t* form, const int32_t* loc_idx, const float* loc_w, const float* loc0,
                                    const int32_t* scale_idx, const float* scale_w, const float* log_scale0, int64_t n_draws,
                                    uint64_t seed, int64_t draw_offset, float* x, int64_t row_stride, uint8_t* undrawn,
                                    void* stream) {
  using namespace arp;
  const std::string who = "arp_site_prior_draws";
  if (!form || !loc_idx || !loc_w || !loc0 || !scale_idx || !scale_w || !log_scale0 || !x) {
    set_error(who + ": the table (form, loc_idx, loc_w, loc0, scale_idx, scale_w, log_scale0) and x are required");
    return 1;
  }
  if (D < 1 || D > kObsMaxD) { set_error(who + ": 1 <= D <= 255 is required"); return 1; }
  if (n_draws < 1 || n_draws > kPdMaxR) { set_error(who + ": 1 <= n_draws <= 2^24 is required"); return 1; }
  if (row_stride < D) { set_error(who + ": row_stride >= D is required"); return 1; }
  if (draw_offset < 0) { set_error(who + ": draw_offset >= 0 is required"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(prior_draw_kernel, dim3(blocks_for(n_draws, kObsDraws)), dim3(kObsDraws), tile_lds_bytes(D), st, (int)D, form,
                     loc_idx, loc_w, loc0, scale_idx, scale_w, log_scale0, (long long)n_draws, (unsigned)seed,
                     (unsigned)(seed >> 32), (unsigned long long)draw_offset, x, (long long)row_stride, (unsigned char*)undrawn);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
