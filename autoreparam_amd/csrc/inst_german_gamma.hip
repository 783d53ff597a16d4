// Chain-kernel instantiations for german_credit_gammascale: the lanes of inst_german.hip with Gamma-prior scales
// (model_german.h, PRIOR_ = kGermanGamma), selected by arp_model_set_option(h, "german_prior", "gamma").
#include "host_common.h"

namespace arp {
const LaneOps& german_gamma_bf3_ops() {
  static const LaneOps o = german_lane4_ops<kGermanGamma, true>();
  return o;
}
const std::vector<LaneOps>& german_gamma_ops() {
  static const std::vector<LaneOps> t = german_lane_ops<kGermanGamma>();
  return t;
}
}  // namespace arp
