// Host plumbing the diagnostics share (diag.hip, rank.hip, mcess.hip, ess.hip): how a caller-owned workspace is carved and
// checked, the shape rules of the [S, C, D] entry points, grid sizes.  Host code only.
#pragma once
#include <stdint.h>
#include <string>
#include "host_error.h"

namespace arp {

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// A workspace handed out front to back, every array 256-byte aligned: take() gives the array's offset, bytes() the total.
struct Carve {
  int64_t at = 0;
  int64_t take(int64_t bytes) { const int64_t off = at; at += align256(bytes); return off; }
  int64_t bytes() const { return at; }
};

// workgroups of `threads` that cover n items
inline unsigned blocks_for(long long n, long long threads) { return (unsigned)((n + threads - 1) / threads); }

// What a [S, C, D] trace must satisfy whichever diagnostic reads it: 32-bit draw indices within an element, and grids that
// stay below 2^31 workgroups (2^35 values per call).  `who` is the entry point, for the message.
inline bool trace_shape_ok(int64_t n_samples, int64_t n_chains, int32_t D, const char* who) {
  const char* rule = nullptr;
  if (n_samples <= 0 || n_chains <= 0 || D <= 0) rule = ": n_samples > 0, n_chains > 0 and D > 0 are required";
  else if (n_samples >= (1ll << 31) || n_chains >= (1ll << 31) || n_samples * n_chains >= (1ll << 31))
    rule = ": at most 2^31 - 1 draws per element (n_samples * n_chains)";
  else if (n_samples * n_chains * D > (1ll << 35)) rule = ": at most 2^35 values per call";
  if (rule) set_error(std::string(who) + rule);
  return !rule;
}

// The two refusals of a workspace, apart (the entry points ask in different orders, and some only one): `enough` is the
// caller's own test of the size, `see` where the size comes from
inline bool workspace_size_ok(bool enough, const char* who, const char* see) {
  if (!enough) set_error(std::string(who) + ": workspace too small (" + see + ")");
  return enough;
}
inline bool workspace_aligned(const void* workspace, const char* who) {
  const bool ok = ((uintptr_t)workspace & 255) == 0;
  if (!ok) set_error(std::string(who) + ": the workspace must be 256-byte aligned");
  return ok;
}

}  // namespace arp
