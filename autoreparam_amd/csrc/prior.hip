// Per-site log prior of recorded draws (include/autoreparam.h: arp_site_logprior): the log density of every latent
// element d at draw r of a centred trace, from the model's latent site table (autoreparam_amd/models.py:
// ModelSpec.site_table), and the sums of those densities over caller-chosen groups of elements -- the prior-side twin
// of arp_pointwise_loglik, what power-scaling a CHOSEN prior is computed from.  Model-independent.  Build-specific: the
// reference evaluates joint densities only.
//
//   loc_d = loc0[d] + sum_t loc_w[d][t] x[loc_idx[d][t]],   s_d = log_scale0[d] + sum_t scale_w[d][t] x[scale_idx[d][t]]
//   form 0 (Normal, scale exp(s)):       z = (x_d - loc_d) exp(-s_d),  lp = -0.5 z^2 - s_d + norm[d]
//   form 1 (Normal, scale softplus(s)):  sigma = max(s_d, 0) + log1p(exp(-|s_d|)),  z = (x_d - loc_d) / sigma,
//                                        lp = -0.5 z^2 - log(sigma) + norm[d]
//   form 2 (log of a Gamma variable):    lp = loc0[d] x_d - exp(s_d + x_d) + norm[d]       (the loc terms are not read)
//
// Shape of the work: obs_table.h's, with the elements where the observations were.  A workgroup stages one tile of 64
// draws in LDS (stage_tile<true>, pitch D | 1), a draw per lane; the element is uniform per wave, so the table columns
// -- separate __restrict__ arguments -- are scalar loads.  The elements are walked in the order (group, d): thread d finds
// its element's place by counting (D <= 255: one pass over group_of in LDS), and the four waves take the four quarters
// [v D / 4, (v + 1) D / 4) of that order.  Within a quarter a group is a run of adjacent places; a wave adds the float32
// values of a run to a float64 accumulator in ascending d.  A run in the middle of a quarter is a whole group and is
// stored at once; the first and the last run of a quarter may go on in the neighbour's, so those partials meet through
// LDS (2 slots a wave) and wave 0 adds the slots of one group in wave order.  The order of every addition is a function
// of (D, group_of) alone; no float atomics.  A group without elements is written as 0.
// (Per-wave partials of EVERY group would take 2 KiB of LDS a group: that is why only the runs at the quarters' edges
// go through LDS.)
//
// Arithmetic.  float32, contraction off; loc and s are the chains c <- c + w_t x_t over t = 0, 1 in that order from
// c = loc0 / log_scale0, every product and every sum rounded once (a term of weight 0 adds an exact 0).  With u = 2^-24,
// A_loc = |loc0| + sum_t |w_t x_t| and A_s = |log_scale0| + sum_t |w_t x_t|: two products and two sums of partial
// sums within A give
//
//   |loc_dev - loc| <= 3 u A_loc,   |s_dev - s| <= 3 u A_s
//
// and, to first order against the exact value of the same float32 inputs (expf, logf, log1pf good to one ulp = 2 u, the
// division correctly rounded),
//
//   form 0:  |lp_dev - lp| <= u [ 3 A_loc exp(-s) |z| + z^2 (5 + 3 A_s) + 4 A_s + |lp| ]
//   form 1:  |lp_dev - lp| <= u [ 3 A_loc |z| / sigma + z^2 (4 + B) + B + 3 |log sigma| + |lp| ],
//            B = (3 A_s + 3) / sigma + 1
//   form 2:  |lp_dev - lp| <= u [ 2 |loc0 x| + E (3 + 3 A_s + |s + x|) + |lp| ],   E = exp(s + x)
//
// (Form 0: z carries the error of loc scaled by exp(-s), the roundings of x - loc, of exp(-s) (2 u) and of the product,
// and the error of s, relatively: dz <= 3 u A_loc exp(-s) + |z| (4 u + 3 u A_s); z^2 doubles that and rounds once, the
// factor 0.5 is exact: 0.5 z^2 is within u [3 A_loc exp(-s) |z| + z^2 (4.5 + 3 A_s)]; the subtraction of s rounds by
// u (0.5 z^2 + |s|) and carries s's own 3 u A_s, |s| <= A_s; the addition of norm rounds by u |lp|.
// Form 1: softplus has slope at most 1 and log1p(exp(.)) <= log 2 carries four roundings of its own, the sum one:
// dsigma <= u (3 A_s + 3 + sigma) = u sigma B; z carries 3 u A_loc / sigma + |z| (3 u + u B), 0.5 z^2 is within
// u [3 A_loc |z| / sigma + z^2 (3.5 + B)]; log(sigma) is within u (B + 2 |log sigma|); the two last operations round by
// u (0.5 z^2 + |log sigma|) and u |lp|.
// Form 2: the product rounds by u |loc0 x|; s + x by u |s + x| on top of s's 3 u A_s, and exp turns that absolute error
// into a relative one next to its own 2 u; the subtraction rounds by u (|loc0 x| + E), the addition of norm by u |lp|.)
//
// group_lp is the float64 sum of the float32 values: n_g - 1 additions in whatever tree, so
//   |group_lp - sum_d lp_d| <= sum of the elements' bounds + (n_g + 4) 2^-53 sum |elem_lp|.
//
// A draw that is left out: a draw with a non-finite element among its D is masked; its elem_lp and group_lp entries are
// WRITTEN, as 0 by select.  NaN and +-inf of a finite draw are results.  What goes wrong quietly with the tile and the
// table's indices: obs_table.h; group_of is clamped into [0, G) as the indices are into [0, D), and a form other than 1
// or 2 is read as 0.
#include "obs_table.h"
#include "site_table.h"

#pragma clang fp contract(off)

namespace arp {
namespace {

constexpr int kSiteSlots = 2 * kObsWaves;        // the first and the last run of every wave's quarter

__global__ __launch_bounds__(kObsThreads) void site_kernel(const float* __restrict__ x, long long R, unsigned n_chains, int D,
                                                           long long stride, const int* __restrict__ form,
                                                           const int* __restrict__ loc_idx, const float* __restrict__ loc_w,
                                                           const float* __restrict__ loc0, const int* __restrict__ scale_idx,
                                                           const float* __restrict__ scale_w,
                                                           const float* __restrict__ log_scale0, const float* __restrict__ norm,
                                                           const int* __restrict__ group_of, int G,
                                                           double* __restrict__ group_lp, float* __restrict__ elem_lp,
                                                           unsigned char* __restrict__ mask,
                                                           unsigned long long* __restrict__ n_masked) {
  extern __shared__ float tile[];                // [64][D | 1]
  __shared__ int sh_bad[kObsDraws];
  __shared__ int sh_group[kObsMaxD + 1];         // the group of element d
  __shared__ int sh_perm[kObsMaxD + 1];          // the elements in the order (group, d)
  __shared__ int sh_members[kObsMaxD + 1];       // how many elements group g has
  __shared__ double sh_part[kSiteSlots][kObsDraws];
  __shared__ int sh_slot_group[kSiteSlots];      // the group a slot holds a partial sum of; -1: none
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const long long r0 = (long long)blockIdx.x * kObsDraws;
  const int nrows = (int)min((long long)kObsDraws, R - r0);
  if (t < D) sh_group[t] = min(max(group_of[t], 0), G - 1);
  if (t < kSiteSlots) sh_slot_group[t] = -1;
  stage_tile<true>(x, r0, nrows, n_chains, D, stride, tile, sh_bad);       // (its barriers publish sh_group as well)
  if (t < D) {
    // element t's place in the order (group, d); and, G <= D, the size of group t
    const int g = sh_group[t];
    int place = 0, members = 0;
    for (int e = 0; e < D; ++e) {
      const int ge = sh_group[e];
      place += (ge < g || (ge == g && e < t)) ? 1 : 0;
      members += ge == t ? 1 : 0;
    }
    sh_perm[place] = t;
    sh_members[t] = members;
  }
  __syncthreads();
  const bool live = lane < nrows;
  const bool bad = sh_bad[lane] != 0;
  if (wave == 0) write_mask(live, bad, lane, r0, mask, n_masked);

  const float* row = tile + lane * (D | 1);
  double* out = group_lp + (r0 + lane) * (long long)G;
  const int i0 = wave * D / kObsWaves, i1 = (wave + 1) * D / kObsWaves;
  double acc = 0.0;
  int cur = -1;                                  // the group of the run being added; wave-uniform, as `first` is
  bool first = true;
  for (int i = i0; i < i1; ++i) {
    const int d = __builtin_amdgcn_readfirstlane(sh_perm[i]);
    const int g = __builtin_amdgcn_readfirstlane(sh_group[d]);
    if (g != cur) {
      if (cur >= 0) {                            // a run has ended and another follows: the quarter's first, or a whole group
        if (first) {
          sh_part[2 * wave][lane] = acc;
          if (lane == 0) sh_slot_group[2 * wave] = cur;
          first = false;
        } else if (live) {
          out[cur] = acc;
        }
      }
      cur = g;
      acc = 0.0;
    }
    const int f = form[d];
    const float xd = row[d];
    const float s = site_chain(row, scale_idx, scale_w, log_scale0[d], d, D);
    float v;
    if (f == 2) {
      v = loc0[d] * xd - expf(s + xd);
    } else {
      const float loc = site_chain(row, loc_idx, loc_w, loc0[d], d, D);
      if (f == 1) {
        const float sigma = fmaxf(s, 0.0f) + log1pf(expf(-fabsf(s)));
        const float z = (xd - loc) / sigma;
        v = -0.5f * (z * z) - logf(sigma);
      } else {
        const float z = (xd - loc) * expf(-s);
        v = -0.5f * (z * z) - s;
      }
    }
    v = v + norm[d];
    v = bad ? 0.0f : v;
    if (elem_lp && live) elem_lp[(r0 + lane) * (long long)D + d] = v;
    acc += (double)v;
  }
  if (cur >= 0) {                                // the quarter's last run (its first as well, if it has only one)
    const int slot = 2 * wave + (first ? 0 : 1);
    sh_part[slot][lane] = acc;
    if (lane == 0) sh_slot_group[slot] = cur;
  }
  __syncthreads();
  if (wave == 0) {
    // the slots in wave order: those of one group are adjacent, since the quarters are adjacent in the order (group, d)
    cur = -1;
    for (int k = 0; k < kSiteSlots; ++k) {
      const int g = __builtin_amdgcn_readfirstlane(sh_slot_group[k]);
      if (g < 0) continue;
      if (g != cur) {
        if (cur >= 0 && live) out[cur] = acc;
        cur = g;
        acc = sh_part[k][lane];
      } else {
        acc += sh_part[k][lane];
      }
    }
    if (cur >= 0 && live) out[cur] = acc;
  }
  for (int g = wave; g < G; g += kObsWaves)
    if (__builtin_amdgcn_readfirstlane(sh_members[g]) == 0 && live) out[g] = 0.0;
}

}  // namespace
}  // namespace arp

extern "C" int arp_site_logprior(const float* x, int64_t n_samples, int64_t n_chains, int32_t D, int64_t row_stride,
                                 const int32_t* form, const int32_t* loc_idx, const float* loc_w, const float* loc0,
                                 const int32_t* scale_idx, const float* scale_w, const float* log_scale0, const float* norm,
                                 const int32_t* group_of, int32_t G, double* group_lp, float* elem_lp, uint8_t* mask,
                                 int64_t* n_masked, void* stream) {
  using namespace arp;
  const char* name = "arp_site_logprior";
  const std::string who = name;
  if (!x || !form || !loc_idx || !loc_w || !loc0 || !scale_idx || !scale_w || !log_scale0 || !norm || !group_of || !group_lp ||
      !mask || !n_masked) {
    set_error(who + ": x, the table (form, loc_idx, loc_w, loc0, scale_idx, scale_w, log_scale0, norm), group_of, group_lp, "
                    "mask and n_masked are required");
    return 1;
  }
  if (D < 1 || D > kObsMaxD) { set_error(who + ": 1 <= D <= 255 is required"); return 1; }
  if (!trace_shape_ok(n_samples, n_chains, D, name)) return 1;
  if (row_stride < n_chains * D) { set_error(who + ": row_stride >= n_chains * D is required"); return 1; }
  if (G < 1 || G > D) { set_error(who + ": 1 <= G <= D groups are required"); return 1; }
  const long long R = n_samples * n_chains;
  hipStream_t st = (hipStream_t)stream;
  ARP_HIP_OK(hipMemsetAsync(n_masked, 0, sizeof(int64_t), st));
  hipLaunchKernelGGL(site_kernel, dim3((unsigned)((R + kObsDraws - 1) / kObsDraws)), dim3(kObsThreads), tile_lds_bytes(D), st, x, R,
                     (unsigned)n_chains, (int)D, (long long)row_stride, form, loc_idx, loc_w, loc0, scale_idx, scale_w, log_scale0,
                     norm, group_of, (int)G, group_lp, elem_lp, (unsigned char*)mask, (unsigned long long*)n_masked);
  ARP_HIP_OK(hipGetLastError());
  return 0;
}
