// Chain-kernel instantiations for german_credit_lognormalcentered: the padded
// 64-column design matrix is split over K lanes x 64/K consecutive features (host_common.h: german_lane_ops).
#include "host_common.h"

namespace arp {
const LaneOps& german_bf3_ops() {
  static const LaneOps o = german_lane4_ops<kGermanLogNormal, true>();
  return o;
}
const std::vector<LaneOps>& german_ops() {
  static const std::vector<LaneOps> t = german_lane_ops<kGermanLogNormal>();
  return t;
}
}  // namespace arp
