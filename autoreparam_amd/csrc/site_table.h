// What the kernels over a model's latent site table share (prior.hip, prior_draw.hip; the table: autoreparam_amd/models.py:
// ModelSpec.site_table): the float32 chain of a site's loc and of its log-scale over a lane's row of the tile.
//
//   loc_d = loc0[d] + sum_t loc_w[d][t] x[loc_idx[d][t]],   s_d = log_scale0[d] + sum_t scale_w[d][t] x[scale_idx[d][t]]
//
// float32, contraction off: c <- c + w_t x_t over t = 0, 1 in that order from c = loc0 / log_scale0, every product and
// every sum rounded once; the indices are clamped into [0, D).  The bound 3 u A: prior.hip.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace arp {

constexpr int kSiteTerms = 2;                    // ARP_SITE_TERMS

// c + sum_t w[d][t] row[idx[d][t]], in term order
__device__ __forceinline__ float site_chain(const float* row, const int* idx, const float* w, float c, int d, int D) {
  const int* ip = idx + d * kSiteTerms;
  const float* wp = w + d * kSiteTerms;
#pragma unroll
  for (int k = 0; k < kSiteTerms; ++k) {
    const int i = min(max(ip[k], 0), D - 1);
    c = c + wp[k] * row[i];
  }
  return c;
}

}  // namespace arp
