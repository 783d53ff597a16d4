// Pointwise log-likelihood of recorded draws (include/autoreparam.h: arp_pointwise_loglik): ll[n][r] for observation n
// and draw r of a centred trace, from the model's observation table (autoreparam_amd/models.py:
// ModelSpec.observation_table) -- what PSIS-LOO and WAIC (psis.hip) are computed from.  Model-independent: every model
// with data here is Normal or Bernoulli-logit over a linear predictor of the centred latents,
//
//   eta_n = sum_t w[n][t] x[idx[n][t]],   s_n = log_scale[n] + (scale_idx[n] >= 0 ? x[scale_idx[n]] : 0)
//   Normal:     ll = -0.5 ((y_n - eta_n) exp(-s_n))^2 - s_n - 0.5 log(2 pi)
//   Bernoulli:  ll = y_n eta_n - softplus(eta_n),   softplus(e) = max(e, 0) + log1p(exp(-|e|))
//
// Build-specific: the reference evaluates joint densities only.
//
// Shape of the work.  Draws lie across the lanes of a wave and the observation is uniform per wave, so idx, w, y and the
// scale entries are wave-uniform (scalar) loads.  A workgroup of four waves stages ONE tile of 64 draws -- all D elements
// of each, read coalesced from the trace in place -- in LDS with an odd row pitch (lane l reads x[l][idx]: 64 different
// banks whatever idx is), finds which of its draws are left out, and its waves then walk the observations of the
// workgroup's share (blockIdx.y), wave v taking every fourth.  Stores of ll are coalesced along r.
//
// No matrix cores: German credit at 65 536 draws is 1 000 x 65 536 x 62 = 4 10^9 multiply-adds, far under a millisecond
// of vector arithmetic; what the kernel takes beyond that is LDS reads, the likelihood's expf / log1pf and the store of
// ll (measured: DESIGN.md section 6).  The table pointers are __restrict__ kernel arguments: that is what lets the
// compiler load idx and w through the scalar unit (handed over in a struct they became per-lane vector loads).
//
// Arithmetic.  float32 throughout, contraction off: eta is the chain eta <- eta + w_t x_t over t = 0 ... T - 1 in that
// order, every product and every sum rounded once.  With u = 2^-24, A = sum_t |w_t x_t| and z = (y - eta) exp(-s), to
// first order against the exact value of the same float32 inputs (expf and log1pf good to one ulp = 2 u):
//
//   |eta_dev - eta| <= T u A
//   Normal:     |ll_dev - ll| <= u [ T A exp(-s) |z| + z^2 (5 + |s|) + 3 |s| + |ll| ]
//   Bernoulli:  |ll_dev - ll| <= u [ T A (|y| + 1) + |y eta| + 3 + softplus(eta) + |ll| ]
//
// (Normal: the error of eta scaled by |d ll / d eta| = exp(-s) |z|; the roundings of y - eta, exp(-s), their product,
// its square and of s itself -- a table entry rounded to float32, one addition -- inside z^2, the two subtractions.
// Bernoulli: softplus has slope at most 1; log1p(exp(.)) <= log 2 carries four roundings of its own.)
//
// Things that go wrong quietly here:
//  * A draw that is left out.  A draw with a non-finite element among its D is masked: its ll entries are WRITTEN, as 0
//    by select -- never a product with a 0 / 1 mask, 0 * inf is NaN -- and nothing downstream reads them.
//  * Reads past the end.  A load is issued for (r < n_samples * n_chains, d < D) only; nothing is read past
//    x[(n_samples - 1) * row_stride + n_chains * D - 1].  Dead rows of the tile hold 0 and are never stored.
//  * The table.  idx and scale_idx are clamped into [0, D) before they address the tile; the caller's checks (
//    diagnostics.pointwise_loglik) keep them there in the first place.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "diag_host.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kLlThreads = 256;
constexpr int kLlWaves = kLlThreads / 64;
constexpr int kLlDraws = 64;                     // draws per tile: one per lane
constexpr int kLlMaxD = 255;                     // 64 rows of pitch 255 floats: 65 280 bytes of LDS
constexpr int kLlMaxT = 4096;
constexpr long long kLlTargetWorkgroups = 2048;
constexpr float kHalfLog2PiF = 0.9189385332046727f;

__global__ __launch_bounds__(kLlThreads) void loglik_kernel(const float* __restrict__ x, long long R, unsigned n_chains, int D,
                                                            long long stride, int kind, int T, const int* __restrict__ idx,
                                                            const float* __restrict__ w, const float* __restrict__ y,
                                                            const int* __restrict__ scale_idx,
                                                            const float* __restrict__ log_scale, long long n0, long long n1,
                                                            long long per_group, float* __restrict__ ll, long long ll_stride,
                                                            unsigned char* __restrict__ mask,
                                                            unsigned long long* __restrict__ n_masked) {
  extern __shared__ float tile[];                // [64][Dp]
  __shared__ int sh_bad[kLlDraws];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int Dp = D | 1;
  const long long r0 = (long long)blockIdx.x * kLlDraws;
  const int nrows = (int)min((long long)kLlDraws, R - r0);

  if (t < kLlDraws) sh_bad[t] = 0;
  __syncthreads();
  // element e = t + 256 a of the tile is (row e / D, column e % D); a dead row takes 0 without a load
  const int nelem = kLlDraws * D;
  for (int e = t; e < nelem; e += kLlThreads) {
    const int lr = (int)((unsigned)e / (unsigned)D), d = e - lr * D;
    float v = 0.0f;
    if (lr < nrows) {
      const unsigned r = (unsigned)(r0 + lr);
      const unsigned step = r / n_chains, chain = r - step * n_chains;
      v = x[(long long)step * stride + (long long)chain * D + d];
      if (!(v - v == 0.0f)) sh_bad[lr] = 1;
    }
    tile[lr * Dp + d] = v;
  }
  __syncthreads();
  const bool live = lane < nrows;
  const bool bad = sh_bad[lane] != 0;
  if (blockIdx.y == 0 && wave == 0) {
    if (live) mask[r0 + lane] = bad ? 1 : 0;
    const unsigned long long b = __ballot(live && bad);
    if (lane == 0 && b != 0) atomicAdd(n_masked, (unsigned long long)__popcll(b));      // (an integer count: order-free)
  }

  const float* row = tile + lane * Dp;
  const long long nb = n0 + (long long)blockIdx.y * per_group, ne = min(n1, nb + per_group);
  for (long long n = nb + wave; n < ne; n += kLlWaves) {
    const int* ip = idx + n * T;
    const float* wp = w + n * T;
    float eta = 0.0f;
#pragma unroll 4
    for (int k = 0; k < T; ++k) {
      const int i = min(max(ip[k], 0), D - 1);
      eta = eta + wp[k] * row[i];
    }
    const float yn = y[n];
    float v;
    if (kind == 0) {
      const int si = scale_idx[n];
      float s = log_scale[n];
      if (si >= 0) s = s + row[min(si, D - 1)];
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
  const std::string who = "arp_pointwise_loglik";
  if (!x || !idx || !w || !y || !scale_idx || !log_scale || !ll || !mask || !n_masked) {
    set_error(who + ": x, the table (idx, w, y, scale_idx, log_scale), ll, mask and n_masked are required");
    return 1;
  }
  if (D < 1 || D > kLlMaxD) { set_error(who + ": 1 <= D <= 255 is required"); return 1; }
  if (!trace_shape_ok(n_samples, n_chains, D, "arp_pointwise_loglik")) return 1;
  if (row_stride < n_chains * D) { set_error(who + ": row_stride >= n_chains * D is required"); return 1; }
  if (kind != 0 && kind != 1) { set_error(who + ": kind must be ARP_OBS_NORMAL or ARP_OBS_BERNOULLI"); return 1; }
  if (T < 1 || T > kLlMaxT) { set_error(who + ": 1 <= T <= 4096 is required"); return 1; }
  if (n0 < 0 || n1 <= n0 || n1 >= (1ll << 31)) { set_error(who + ": 0 <= n0 < n1 < 2^31 is required"); return 1; }
  const long long R = n_samples * n_chains;
  if (ll_stride < R) { set_error(who + ": ll_stride >= n_samples * n_chains is required"); return 1; }
  hipStream_t st = (hipStream_t)stream;
  ARP_HIP_OK(hipMemsetAsync(n_masked, 0, sizeof(int64_t), st));
  const long long ntiles = (R + kLlDraws - 1) / kLlDraws;
  const long long nobs = n1 - n0;
  long long groups = std::max<long long>(1, (kLlTargetWorkgroups + ntiles - 1) / ntiles);
  groups = std::min<long long>(std::min<long long>(groups, (nobs + kLlWaves - 1) / kLlWaves), 65535);
  const long long per_group = (nobs + groups - 1) / groups;
  groups = (nobs + per_group - 1) / per_group;
  const size_t lds = (size_t)kLlDraws * (D | 1) * sizeof(float);
  hipLaunchKernelGGL(loglik_kernel, dim3((unsigned)ntiles, (unsigned)groups), dim3(kLlThreads), lds, st, x, R, (unsigned)n_chains,
                     (int)D, (long long)row_stride, (int)kind, (int)T, idx, w, y, scale_idx, log_scale, (long long)n0, (long long)n1, per_group, ll, (long long)ll_stride,
                     (unsigned char*)mask, (unsigned long long*)n_masked);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
