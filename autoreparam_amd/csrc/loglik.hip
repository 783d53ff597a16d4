// Pointwise log-likelihood of recorded draws (include/autoreparam.h: arp_pointwise_loglik): ll[n][r] for observation n
// and draw r of a centred trace, from the model's observation table -- what PSIS-LOO and WAIC (psis.hip) are computed
// from.  Model-independent; the table, the tile of draws, eta_n and s_n, the shape of the work and what goes wrong
// quietly with the tile and the table: obs_table.h.
//
//   Normal:     ll = -0.5 ((y_n - eta_n) exp(-s_n))^2 - s_n - 0.5 log(2 pi)
//   Bernoulli:  ll = y_n eta_n - softplus(eta_n),   softplus(e) = max(e, 0) + log1p(exp(-|e|))
//
// Build-specific: the reference evaluates joint densities only.  Stores of ll are coalesced along r.
//
// No matrix cores: German credit at 65 536 draws is 1 000 x 65 536 x 62 = 4 10^9 multiply-adds, far under a millisecond
// of vector arithmetic; what the kernel takes beyond that is LDS reads, the likelihood's expf / log1pf and the store of
// ll (measured: DESIGN.md section 6).
//
// Arithmetic.  float32, contraction off.  With u = 2^-24, A = sum_t |w_t x_t|, obs_table.h's |eta_dev - eta| <= T u A and
// z = (y - eta) exp(-s), to first order against the exact value of the same float32 inputs (expf and log1pf good to one
// ulp = 2 u):
//
//   Normal:     |ll_dev - ll| <= u [ T A exp(-s) |z| + z^2 (5 + |s|) + 3 |s| + |ll| ]
//   Bernoulli:  |ll_dev - ll| <= u [ T A (|y| + 1) + |y eta| + 3 + softplus(eta) + |ll| ]
//
// (Normal: the error of eta scaled by |d ll / d eta| = exp(-s) |z|; the roundings of y - eta, exp(-s), their product,
// its square and of s itself -- a table entry rounded to float32, one addition -- inside z^2, the two subtractions.
// Bernoulli: softplus has slope at most 1; log1p(exp(.)) <= log 2 carries four roundings of its own.)
//
// A draw that is left out: a draw with a non-finite element among its D is masked: its ll entries are WRITTEN, as 0 by
// select -- never a product with a 0 / 1 mask, 0 * inf is NaN -- and nothing downstream reads them.
#include "obs_table.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr float kHalfLog2PiF = 0.9189385332046727f;

__global__ __launch_bounds__(kObsThreads) void loglik_kernel(const float* __restrict__ x, long long R, unsigned n_chains, int D,
                                                             long long stride, int kind, int T, const int* __restrict__ idx,
                                                             const float* __restrict__ w, const float* __restrict__ y,
                                                             const int* __restrict__ scale_idx,
                                                             const float* __restrict__ log_scale, long long n0, long long n1,
                                                             long long per_group, float* __restrict__ ll, long long ll_stride,
                                                             unsigned char* __restrict__ mask,
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

  const float* row = tile + lane * (D | 1);
  const long long nb = n0 + (long long)blockIdx.y * per_group, ne = min(n1, nb + per_group);
  for (long long n = nb + wave; n < ne; n += kObsWaves) {
    const float eta = obs_eta(row, idx, w, n, T, D);
    const float yn = y[n];
    float v;
    if (kind == 0) {
      const float s = obs_log_scale(row, scale_idx, log_scale, n, D);
      const float z = (yn - eta) * expf(-s);
      v = -0.5f * (z * z) - s - kHalfLog2PiF;
    } else {
      v = yn * eta - (fmaxf(eta, 0.0f) + log1pf(expf(-fabsf(eta))));
    }
    if (live) ll[(n - n0) * ll_stride + r0 + lane] = bad ? 0.0f : v;
  }
}

}  // namespace
}  // namespace arp

extern "C" int arp_pointwise_loglik(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                                    int32_t kind, const int32_t* idx, const float* w, int32_t T, const float* y,
                                    const int32_t* scale_idx, const float* log_scale, int64_t n0, int64_t n1, float* ll,
                                    int64_t ll_stride, uint8_t* mask, int64_t* n_masked, void* stream) {
  using namespace arp;
  const char* name = "arp_pointwise_loglik";
  const std::string who = name;
  if (!x || !idx || !w || !y || !scale_idx || !log_scale || !ll || !mask || !n_masked) {
    set_error(who + ": x, the table (idx, w, y, scale_idx, log_scale), ll, mask and n_masked are required");
    return 1;
  }
  if (!table_call_ok(name, n_samples, n_chains, D, row_stride, kind, T, n0, n1)) return 1;
  const long long R = n_samples * n_chains;
  if (ll_stride < R) { set_error(who + ": ll_stride >= n_samples * n_chains is required"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  ARP_HIP_OK(hipMemsetAsync(n_masked, 0, sizeof(int64_t), st));
  const Split sp = split_of(n1 - n0, R);
  hipLaunchKernelGGL(loglik_kernel, dim3((unsigned)sp.ntiles, (unsigned)sp.groups), dim3(kObsThreads), tile_lds_bytes(D), st, x, R,
                     (unsigned)n_chains, (int)D, (long long)row_stride, (int)kind, (int)T, idx, w, y, scale_idx, log_scale,
                     (long long)n0, (long long)n1, sp.per_group, ll, (long long)ll_stride, (unsigned char*)mask,
                     (unsigned long long*)n_masked);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
