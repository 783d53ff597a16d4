// What the kernels over GROUPS of a model's observations share (ppc_group.hip, logo.hip): the layout of the groups, the walk
// over a group's members, which wave owns which group, and on the host the refusals both entry points make.  The table,
// the tile of draws and the launch rule (shares_of): obs_table.h.
//
// Layout.  A group is a list of observation indices (diagnostics.group_selection: the observations that read one element
// of a latent part), not contiguous in the table: `order` [n_grouped] holds the grouped observations sorted by group,
// ascending observation index within a group, and group_start[g] ... group_start[g + 1] is group g's stretch of it.
//
// Ownership.  Every wave owns WHOLE groups -- wave v of workgroup (tile, b) takes the groups g0 + 4 b + v, then every
// (4 gridDim.y)-th: round robin, not by size, so the longest group bounds a wave's time -- and carries a group's sums in
// registers over its members in order's sequence.  Hence no LDS fold, no barrier behind the tile's, no workspace, no second
// launch and no float atomics: the sums of a (group, draw) are one fixed chain of additions, whatever the tiling, the
// range [g0, g1) of the call and the way groups are shared among waves and workgroups.  A wave without a group (more waves
// than groups in the call) still takes part in the staging and its barriers, and stores nothing.  The observation is
// uniform per wave, so group_start and order are scalar loads; the next entry of order is asked for before the current
// member's body, which hides the first of the two dependent scalar loads.
//
// Clamps.  order and group_start come from the caller: an order entry is clamped into [0, n_obs) and a group_start entry
// into [0, n_grouped], the end of a group not before its start, before they address anything; the uploaders
// (diagnostics.upload_groups, upload_logo_groups) keep them there in the first place.  A clamped entry gives a wrong
// number, never a read past the end.
#pragma once
#include "obs_table.h"

namespace arp {

// group g's stretch [jb, je) of order;  then  next = first_member;  for (j = jb; j < je; ++j) { n = member_obs(next, n_obs);
// next = next_member(order, j, je, next);  the body of (j, n) }.  (Small value-returning pieces on purpose: a walk that takes
// the body as a callable, or a prefetch that writes `next` through a reference, moved instructions of the kernels.)
__device__ __forceinline__ int group_begin(const int* start, long long g, int n_grouped) { return min(max(start[g], 0), n_grouped); }
__device__ __forceinline__ int group_end(const int* start, long long g, int jb, int n_grouped) { return min(max(start[g + 1], jb), n_grouped); }
__device__ __forceinline__ int first_member(const int* order, int jb, int je) { return jb < je ? order[jb] : 0; }
__device__ __forceinline__ long long member_obs(int next, int n_obs) { return min(max(next, 0), n_obs - 1); }
__device__ __forceinline__ int next_member(const int* order, int j, int je, int next) { return j + 1 < je ? order[j + 1] : next; }

// ---- host ----
// The refusals both entry points make of the groups, behind their own test for null pointers
inline bool group_call_ok(const char* name, int64_t n_obs, int64_t n_grouped, const int32_t* order, int64_t n_groups, int64_t g0,
                          int64_t g1) {
  const char* rule = nullptr;
  if (n_obs < 1 || n_obs >= (1ll << 31)) rule = ": 1 <= n_obs < 2^31 is required";
  else if (n_grouped < 0 || n_grouped >= (1ll << 31)) rule = ": 0 <= n_grouped < 2^31 is required";
  else if (n_grouped > 0 && !order) rule = ": order is required (n_grouped > 0)";
  else if (n_groups < 1 || n_groups >= (1ll << 31)) rule = ": 1 <= n_groups < 2^31 is required";
  else if (g0 < 0 || g1 <= g0 || g1 > n_groups) rule = ": 0 <= g0 < g1 <= n_groups is required";
  if (rule) set_error(std::string(name) + rule);
  return !rule;
}

}  // namespace arp
