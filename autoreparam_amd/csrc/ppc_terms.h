// The replicated value of ONE (observation, draw) and what is folded of it -- what ppc.hip (every observation of a range,
// folded per draw and per observation) and ppc_group.hip (the observations of a group, folded per group and draw) both
// walk the observation table with.  The Philox counter (n, lo32 g, hi32 g, 0) and key, u and the Box-Muller z, the float32
// operation order of y_rep and the two deviances, and the error bounds: ppc.hip's header, which derives them once for
// both kernels; eta, s and the predictive terms: obs_table.h.
#pragma once
#include "arp_device.h"
#include "obs_table.h"

#pragma clang fp contract(off)

namespace arp {

constexpr int kPcCols = 8;                       // columns of draw_stats and of group_stats
constexpr float kLog2PiF = 1.8378770664093453f;

// y_rep, dev(y_rep), dev(y) and the predictive terms of (n, this lane's draw)
struct PpcTerms { float yr, dev_r, dev_o; PredTerms pt; };

// n is uniform per wave -- its index in the WHOLE table, which is what the counter takes -- and so is kind.  The table
// columns are separate pointers, as the kernels take them: that keeps their loads scalar (obs_table.h).
__device__ __forceinline__ PpcTerms ppc_terms(const float* row, int kind, int T, int D, const int* idx, const float* w,
                                              const float* y, const int* scale_idx, const float* log_scale, long long n,
                                              unsigned g_lo, unsigned g_hi, unsigned key0, unsigned key1) {
  PpcTerms o;
  const float eta = obs_eta(row, idx, w, n, T, D);
  const float yn = y[n];
  uint32_t rnd[4];
  philox4x32_10((uint32_t)n, g_lo, g_hi, 0u, key0, key1, rnd);
  if (kind == 0) {
    const float s = obs_log_scale(row, scale_idx, log_scale, n, D);
    const float es = expf(s), ems = expf(-s);
    const float up = fmaf((float)rnd[0], 2.3283064365386963e-10f, 1.1641532182693481e-10f);
    const float z = sqrtf(-2.0f * logf(up)) * cospif(2.0f * angle_rev(rnd[1]));
    o.yr = eta + es * z;
    o.pt = normal_terms(eta, yn, es, ems);
    const float zo = o.pt.aux, zr = (o.yr - eta) * ems;
    const float two_s = 2.0f * s;
    o.dev_r = (zr * zr + two_s) + kLog2PiF;
    o.dev_o = (zo * zo + two_s) + kLog2PiF;
  } else {
    o.pt = bernoulli_terms(eta, yn);
    const float e = o.pt.aux, p = o.pt.mu;
    const float u01 = (float)(rnd[0] >> 8) * 5.9604644775390625e-08f;
    o.yr = u01 < p ? 1.0f : 0.0f;
    const float sp = fmaxf(eta, 0.0f) + log1pf(e);
    o.dev_r = -2.0f * (o.yr * eta - sp);
    o.dev_o = -2.0f * (yn * eta - sp);
  }
  return o;
}

}  // namespace arp
