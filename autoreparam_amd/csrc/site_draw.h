// The draw of ONE element of a latent site table given the elements of the same draw it hangs on -- what prior_draw.hip
// (every element, front to back) and site_redraw.hip (the flagged ones, the others recorded) both walk the table with.
// The three forms, the Philox counter (d, lo32 g, hi32 g, j) and key, the 32-attempt log-space Marsaglia-Tsang loop, the
// float32 operation order and the error bounds: prior_draw.hip's header, which derives them once for both kernels.
#pragma once
#include "arp_device.h"
#include "site_table.h"

#pragma clang fp contract(off)

namespace arp {

constexpr int kPdAttempts = 32;
constexpr long long kPdMaxR = 1ll << 24;
constexpr float kTwoPowM32 = 2.3283064365386963e-10f, kTwoPowM33 = 1.1641532182693481e-10f;

// ppc.hip's z from words 0 and 1
__device__ __forceinline__ float draw_z(uint32_t w0, uint32_t w1) {
  const float up = fmaf((float)w0, kTwoPowM32, kTwoPowM33);
  return sqrtf(-2.0f * logf(up)) * cospif(2.0f * angle_rev(w1));
}

// x_d of draw g from this lane's row of the tile (its parents: whatever the row holds at their columns); d is uniform per
// wave, and so is every branch but the accept test.  Every lane of the wave must call it: the rejection loop runs until
// __all lanes have accepted.  failed: set where the 32 attempts ran out, left alone otherwise.  The table columns are
// separate pointers, as the kernels take them: that keeps their loads scalar (obs_table.h).
__device__ __forceinline__ float site_draw_element(const float* row, int d, int D, const int* form, const int* loc_idx,
                                                   const float* loc_w, const float* loc0, const int* scale_idx,
                                                   const float* scale_w, const float* log_scale0, unsigned g_lo, unsigned g_hi,
                                                   unsigned key0, unsigned key1, bool& failed) {
  const int f = form[d];
  const float s = site_chain(row, scale_idx, scale_w, log_scale0[d], d, D);
  float v;
  uint32_t rnd[4];
  if (f == 2) {
    const float k = loc0[d];
    v = __builtin_nanf("");
    if (k > 0.0f && k < __builtin_inff()) {    // (wave-uniform)
      const bool boost = k < 1.0f;
      const float a = boost ? k + 1.0f : k;
      const float dd = a - (1.0f / 3.0f);
      const float c = 1.0f / sqrtf(9.0f * dd);
      const float dd3 = 3.0f * dd;
      bool done = false;
      for (int j = 0; j < kPdAttempts && !__all(done); ++j) {
        philox4x32_10((uint32_t)d, g_lo, g_hi, 1u + (uint32_t)j, key0, key1, rnd);
        const float z = draw_z(rnd[0], rnd[1]);
        const float t = 1.0f + c * z;
        const float U = fmaf((float)rnd[2], kTwoPowM32, kTwoPowM33);
        const float lt = logf(t);              // NaN for t < 0: the comparison below is then false as well
        const float rhs = ((0.5f * (z * z) + dd) - dd * ((t * t) * t)) + dd3 * lt;
        if (!done && t > 0.0f && logf(U) < rhs) {
          const float Ub = fmaf((float)rnd[3], kTwoPowM32, kTwoPowM33);
          const float b = boost ? logf(Ub) / k : 0.0f;
          v = ((logf(dd) + 3.0f * lt) + b) - s;
          done = true;
        }
      }
      failed = failed || !done;
    }
  } else {
    philox4x32_10((uint32_t)d, g_lo, g_hi, 0u, key0, key1, rnd);
    const float z = draw_z(rnd[0], rnd[1]);
    const float loc = site_chain(row, loc_idx, loc_w, loc0[d], d, D);
    const float sigma = f == 1 ? fmaxf(s, 0.0f) + log1pf(expf(-fabsf(s))) : expf(s);
    v = loc + sigma * z;
  }
  return v;
}

}  // namespace arp
