// Posterior predictive check (include/autoreparam.h: arp_predictive_check): replicated observations y_rep[n][r] of
// observation n at draw r of a centred trace, drawn from the model's observation table (autoreparam_amd/models.py:
// ModelSpec.observation_table) and folded on the spot into per-draw test statistics and per-observation predictive
// moments -- does data simulated from the fitted model look like the data?  Model-independent; the table, the tile of
// draws, eta_n and s_n, and the predictive terms mu, var, z_obs, e, p and pit of the two kinds of data: obs_table.h.  The
// per-(n, r) body -- the Philox call, y_rep, the two deviances -- is ppc_terms.h's, which ppc_group.hip (the same replicated
// values folded by group) calls too: the random numbers, the arithmetic and the bounds below hold for both.
//
//   Normal:     y_rep = eta + exp(s) z;  dev(v) = ((v - eta) exp(-s))^2 + 2 s + log 2 pi
//   Bernoulli:  y_rep = (u < p);  dev(v) = -2 (v eta - (max(eta, 0) + log1p(e)))
//
// Build-specific: the reference has no predictive checks.
//
// Random numbers.  Counter based, so that no result depends on the tiling, the observation range of a call or the rank
// that holds a draw: one philox4x32_10(counter (n, lo32 g, hi32 g, 0), key (lo32 seed, hi32 seed)) per (n, r), g =
// draw_offset + r, n the observation's index in the whole table; words 0 and 1 are used.  u = (w0 >> 8) 2^-24 in [0, 1) is
// exact in float32.  The normal is the sampler's Box-Muller (arp_device.h: normal_pair) on the same u' in (0, 1] and the
// same angle a in [1, 2) revolutions, z = sqrt(-2 log u') cospi(2 a), but through the device library's logf, sqrtf and
// cospif: not the hardware approximations, whose error is not stated anywhere -- this is not the sampler's hot path, and a
// per-element test needs a bound.
//
// Shape of the work: obs_table.h's, and the fold, in two directions, all of it in float64 over the float32 per-(n, r)
// values and in a fixed order:
//  * along the observations, per draw: every lane carries its draw's eight statistics in registers over its wave's
//    observations (ascending n); the four waves are added through LDS in wave order; the workgroup's row goes to the
//    workspace [group][R][8], and a second launch combines the groups in ascending order (+, +, min, max, +, +, +, +).
//  * along the draws, per observation: an xor butterfly over the 64 lanes (__shfl_xor on doubles, 32 16 8 4 2 1; every
//    lane ends with the same bits) gives the tile's four sums, lane 0 stores them to the workspace [tile][n][4], and a
//    third launch adds the tiles in ascending order.  The count #{y_rep <= y} is a ballot.
// No float atomics anywhere: two calls give bitwise equal outputs.  A split observation range changes the association of
// the per-draw sums only (to float64 rounding), never min, max, y_rep or obs_sums.
//
// Cost.  Per (n, r): T multiply-adds and LDS reads as loglik, then Philox -- 10 rounds of two 32 x 32 -> 64 multiplies,
// i.e. 40 v_mul_lo / v_mul_hi at quarter rate -- and logf, sqrtf, cospif, two expf and erfcf (Normal) or expf, log1pf
// and a division (Bernoulli).  Measured next to arp_pointwise_loglik: DESIGN.md section 6.
//
// Arithmetic.  float32, contraction off; eta, s and the predictive terms are obs_table.h's functions, which loopred.hip
// calls too: the bounds on mu, m2 and pit below are derived here once and hold for both.  Library functions at the OpenCL
// full-profile limits (OpenCL C specification, "Relative error as ULPs": log 3, exp 3, sqrt 3, sinpi / cospi 4, erfc 16,
// log1p 2 ulp; no sharper statement for the ROCm device library was at hand, so these are what the tests use).  With
// u = 2^-24 (one ulp <= 2 u relative), A = sum_t |w_t x_t|, z_obs = (y - eta) exp(-s), phi the standard normal density, to
// first order against the exact value of the same float32 inputs:
//
//   |eta_dev - eta| <= T u A                              (obs_table.h)
//   Normal
//     |z_dev - z|         <= 18 u |z|                      (log 6 u halved by the root, sqrt 6 u, cospi 8 u, the product 1)
//     |y_rep_dev - y_rep| <= u [ T A + exp(s) |z| (26 + |s|) + |y_rep| ]
//     |pit_dev - pit|     <= u [ phi(z_obs) (T A exp(-s) + |z_obs| (10 + |s|)) + 32 pit ] + 2^-126
//     |dev_dev(v) - dev(v)| <= u [ 2 T A exp(-s) |zv| + zv^2 (18 + 2 |s|) + 4 |s| + |dev| + 2 ] + 2 exp(-s) |zv| |v_dev - v|,
//                            zv = (v - eta) exp(-s)        (v = y: the last term is 0; v = y_rep: the bound above)
//     mu = eta;  |m2_dev - m2| <= u [ 2 |eta| T A + eta^2 + exp(2 s) (14 + 2 |s|) + m2 ],  m2 = mu^2 + var
//   Bernoulli
//     |p_dev - p|     <= u [ p (1 - p) (T A + 6) + 2 p ] =: bp      (exp 6 u; 1 + e and the division one each)
//     |var_dev - var| <= bp + 2 u,  |m2_dev - m2| <= 3 bp + 4 u,  |pit_dev - pit| <= bp / 2 + u
//     |dev_dev(v) - dev(v)| <= 2 u [ T A (|v| + 1) + |v eta| + 8 + softplus(eta) + |v eta - softplus(eta)| ]
//     y_rep_dev = y_rep wherever |u - p| > bp
//
// (exp(s): the rounding of s = log_scale + x, u |s|, and exp's 6 u; y_rep: the product exp(s) z carries 18 + 6 + |s|,
// its own rounding and one to spare, the sum one of |y_rep|.  pit: the error of z_obs -- eta's through exp(-s), the subtraction, exp,
// the product, the constant -1 / sqrt 2 and its product -- times d pit / d z = phi(z), then erfc's 16 ulp; 2^-126 where
// erfc underflows.  dev: the square doubles z's 8 + |s| and adds one; the two sums; log 2 pi rounded to float32.)
// Second-order terms are left out; the tests allow twice these figures, as they do for loglik.hip.
//
// Things that go wrong quietly here:
//  * A draw that is left out (a non-finite element among its D): its draw_stats row and its y_rep entries are WRITTEN, as
//    0 by select -- never a product with a 0 / 1 mask, 0 * inf is NaN -- and it enters no obs_sums, again by select.
//  * Reads past the end, the table's indices: obs_table.h.
//  * Dead lanes of the last ragged tile take part in every shuffle and ballot (the butterfly needs all 64) with 0 by
//    select; they store nothing.
#include "arp_device.h"
#include "obs_table.h"
#include "ppc_terms.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kPcObsCols = 4;                    // columns of obs_sums

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(kObsThreads) void ppc_kernel(
    const float* __restrict__ x, long long R, unsigned n_chains, int D, long long stride, int kind, int T,
    const int* __restrict__ idx, const float* __restrict__ w, const float* __restrict__ y,
    const int* __restrict__ scale_idx, const float* __restrict__ log_scale, long long n0, long long n1, long long per_group,
    unsigned key0, unsigned key1, unsigned long long draw_offset, double* __restrict__ part_draw,
    double* __restrict__ part_obs, float* __restrict__ y_rep, long long y_rep_stride, unsigned char* __restrict__ mask,
    unsigned long long* __restrict__ n_masked) {
  extern __shared__ float tile[];                // [64][D | 1]
  __shared__ int sh_bad[kObsDraws];
  __shared__ double sh_part[kObsWaves - 1][kPcCols][kObsDraws];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long r0 = (long long)blockIdx.x * kObsDraws;
  const int nrows = (int)min((long long)kObsDraws, R - r0);
  stage_tile<true>(x, r0, nrows, n_chains, D, stride, tile, sh_bad);
  const bool live = lane < nrows;
  const bool bad = sh_bad[lane] != 0;
  const bool used = live && !bad;
  if (blockIdx.y == 0 && wave == 0) write_mask(live, bad, lane, r0, mask, n_masked);

  const unsigned long long g = draw_offset + (unsigned long long)(r0 + lane);
  const unsigned g_lo = (unsigned)g, g_hi = (unsigned)(g >> 32);
  const float* row = tile + lane * (D | 1);
  const long long nb = n0 + (long long)blockIdx.y * per_group, ne = min(n1, nb + per_group);
  double a_y = 0.0, a_yy = 0.0, a_dr = 0.0, a_do = 0.0, a_mu = 0.0, a_n = 0.0;
  float a_min = __builtin_inff(), a_max = -__builtin_inff();
  for (long long n = nb + wave; n < ne; n += kObsWaves) {
    const PpcTerms pc = ppc_terms(row, kind, T, D, idx, w, y, scale_idx, log_scale, n, g_lo, g_hi, key0, key1);
    const float yn = y[n];
    const float yr = pc.yr, dev_r = pc.dev_r, dev_o = pc.dev_o;
    const float mu = pc.pt.mu, m2 = pc.pt.m2, pit = pc.pt.pit;
    // along the observations (this lane's draw)
    a_y += (double)yr;
    a_yy += (double)yr * (double)yr;
    a_dr += (double)dev_r;
    a_do += (double)dev_o;
    a_mu += (double)mu;
    a_n += 1.0;
    a_min = fminf(a_min, yr);
    a_max = fmaxf(a_max, yr);
    if (y_rep && live) y_rep[(n - n0) * y_rep_stride + r0 + lane] = bad ? 0.0f : yr;
    // along the draws (this wave's observation): every lane takes part, one that does not count with 0 by select
    const double s_mu = wave_sum(used ? (double)mu : 0.0);
    const double s_m2 = wave_sum(used ? (double)m2 : 0.0);
    const double s_pit = wave_sum(used ? (double)pit : 0.0);
    const unsigned long long le = __ballot(used && yr <= yn);
    if (lane == 0) {
      double* po = part_obs + ((long long)blockIdx.x * (n1 - n0) + (n - n0)) * kPcObsCols;
      po[0] = s_mu; po[1] = s_m2; po[2] = s_pit; po[3] = (double)__popcll(le);
    }
  }

  // the four waves' rows of this tile, added in wave order
  if (wave > 0) {
    double (*sp)[kObsDraws] = sh_part[wave - 1];
    sp[0][lane] = a_y; sp[1][lane] = a_yy; sp[2][lane] = (double)a_min; sp[3][lane] = (double)a_max;
    sp[4][lane] = a_dr; sp[5][lane] = a_do; sp[6][lane] = a_mu; sp[7][lane] = a_n;
  }
  __syncthreads();
  if (wave == 0 && live) {
    double lo = (double)a_min, hi = (double)a_max;
#pragma unroll
    for (int v = 0; v < kObsWaves - 1; ++v) {
      a_y += sh_part[v][0][lane]; a_yy += sh_part[v][1][lane];
      lo = fmin(lo, sh_part[v][2][lane]); hi = fmax(hi, sh_part[v][3][lane]);
      a_dr += sh_part[v][4][lane]; a_do += sh_part[v][5][lane]; a_mu += sh_part[v][6][lane]; a_n += sh_part[v][7][lane];
    }
    double* pd = part_draw + ((long long)blockIdx.y * R + r0 + lane) * kPcCols;
    pd[0] = bad ? 0.0 : a_y; pd[1] = bad ? 0.0 : a_yy; pd[2] = bad ? 0.0 : lo; pd[3] = bad ? 0.0 : hi;
    pd[4] = bad ? 0.0 : a_dr; pd[5] = bad ? 0.0 : a_do; pd[6] = bad ? 0.0 : a_mu; pd[7] = bad ? 0.0 : a_n;
  }
}

// draw_stats[r][c] over the groups in ascending order; one thread per (r, c)
__global__ __launch_bounds__(kObsThreads) void ppc_fold_draws(const double* __restrict__ part_draw, long long R, long long groups,
                                                             double* __restrict__ draw_stats) {
  const long long i = (long long)blockIdx.x * kObsThreads + threadIdx.x;
  if (i >= R * kPcCols) return;
  const int c = (int)(i & (kPcCols - 1));
  double v = part_draw[i];
  for (long long gi = 1; gi < groups; ++gi) {
    const double p = part_draw[gi * R * kPcCols + i];
    v = c == 2 ? fmin(v, p) : c == 3 ? fmax(v, p) : v + p;
  }
  draw_stats[i] = v;
}

// obs_sums[n][c] over the tiles in ascending order; one thread per (n, c)
__global__ __launch_bounds__(kObsThreads) void ppc_fold_obs(const double* __restrict__ part_obs, long long nobs, long long ntiles,
                                                           double* __restrict__ obs_sums) {
  const long long i = (long long)blockIdx.x * kObsThreads + threadIdx.x;
  if (i >= nobs * kPcObsCols) return;
  double v = part_obs[i];
  for (long long ti = 1; ti < ntiles; ++ti) v += part_obs[ti * nobs * kPcObsCols + i];
  obs_sums[i] = v;
}

}  // namespace
}  // namespace arp

extern "C" int64_t arp_predictive_workspace_bytes(int64_t n_obs, int64_t n_draws) {
  using namespace arp;
  if (!obs_shape_ok(n_obs, n_draws)) return 0;
  const Split sp = split_of(n_obs, n_draws);
  Carve c;
  c.take(sp.ntiles * n_obs * kPcObsCols * (int64_t)sizeof(double));
  c.take(sp.groups * n_draws * kPcCols * (int64_t)sizeof(double));
  return c.bytes();
}

extern "C" int arp_predictive_check(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                                    int32_t kind, const int32_t* idx, const float* w, int32_t T, const float* y,
                                    const int32_t* scale_idx, const float* log_scale, int64_t n0, int64_t n1, uint64_t seed,
                                    int64_t draw_offset, double* draw_stats, double* obs_sums, float* y_rep,
                                    int64_t y_rep_stride, uint8_t* mask, int64_t* n_masked, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  using namespace arp;
  const char* name = "arp_predictive_check";
  const std::string who = name;
  if (!x || !idx || !w || !y || !scale_idx || !log_scale || !draw_stats || !obs_sums || !mask || !n_masked) {
    set_error(who + ": x, the table (idx, w, y, scale_idx, log_scale), draw_stats, obs_sums, mask and n_masked are required");
    return 1;
  }
  if (!table_call_ok(name, n_samples, n_chains, D, row_stride, kind, T, n0, n1)) return 1;
  if (draw_offset < 0) { set_error(who + ": draw_offset >= 0 is required"); return 1; }
  const long long R = n_samples * n_chains;
  if (y_rep && y_rep_stride < R) { set_error(who + ": y_rep_stride >= n_samples * n_chains is required"); return 1; }
  const long long nobs = n1 - n0;
  const int64_t need = arp_predictive_workspace_bytes(nobs, R);
  if (!workspace_size_ok(need > 0 && workspace && workspace_bytes >= need, name, "see arp_predictive_workspace_bytes")) return 1;
  if (!workspace_aligned(workspace, name)) return 1;
  const Split sp = split_of(nobs, R);
  Carve c;
  double* part_obs = (double*)((char*)workspace + c.take(sp.ntiles * nobs * kPcObsCols * (int64_t)sizeof(double)));
  double* part_draw = (double*)((char*)workspace + c.take(sp.groups * R * kPcCols * (int64_t)sizeof(double)));
  hipStream_t st = (hipStream_t)stream;
  ARP_HIP_OK(hipMemsetAsync(n_masked, 0, sizeof(int64_t), st));
  hipLaunchKernelGGL(ppc_kernel, dim3((unsigned)sp.ntiles, (unsigned)sp.groups), dim3(kObsThreads), tile_lds_bytes(D), st, x, R,
                     (unsigned)n_chains, (int)D, (long long)row_stride, (int)kind, (int)T, idx, w, y, scale_idx, log_scale, (long long)n0, (long long)n1,
                     sp.per_group, (unsigned)seed, (unsigned)(seed >> 32), (unsigned long long)draw_offset, part_draw, part_obs,
                     y_rep, (long long)y_rep_stride, (unsigned char*)mask, (unsigned long long*)n_masked);
  ARP_HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(ppc_fold_draws, dim3(blocks_for(R * kPcCols, kObsThreads)), dim3(kObsThreads), 0, st, (const double*)part_draw, R,
                     sp.groups, draw_stats);
  ARP_HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(ppc_fold_obs, dim3(blocks_for(nobs * kPcObsCols, kObsThreads)), dim3(kObsThreads), 0, st, (const double*)part_obs,
                     nobs, sp.ntiles, obs_sums);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
