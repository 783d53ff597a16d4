// Chain-kernel instantiations for german_credit_gammascale: the lanes of inst_german.hip with Gamma-prior scales
// (model_german.h, PRIOR_ = kGermanGamma), selected by arp_model_set_option(h, "german_prior", "gamma").
#include "host_common.h"

namespace arp {
// chain kernels from the lanes sized for 4 waves per workgroup, the VI kernel from the 4-lane (matrix-core)
// instantiation in its row-part form, sized for the VI workgroup (as inst_german.hip)
static LaneOps with_vi(LaneOps o, const LaneOps& vi) {
  o.vi = vi.vi; o.vi_block = vi.vi_block; o.vi_parts = vi.vi_parts; o.vi_occ = vi.vi_occ; o.vi_dmax = vi.vi_dmax;
  return o;
}
const LaneOps& german_gamma_bf3_ops() {
  static const LaneOps o = with_vi(Launch<GermanLane<4, 16, kBlock / 64, false, true, kGermanGamma>>::ops(),
                                   Launch<GermanLane<4, 16, kGermanViBlock / 64, true, true, kGermanGamma>>::vi_only());
  return o;
}
const std::vector<LaneOps>& german_gamma_ops() {
  static const std::vector<LaneOps> t = {
      with_vi(Launch<GermanLane<4, 16, kBlock / 64, false, false, kGermanGamma>>::ops(),
              Launch<GermanLane<4, 16, kGermanViBlock / 64, true, false, kGermanGamma>>::vi_only()),
      Launch<GermanLane<8, 8, kBlock / 64, false, false, kGermanGamma>>::ops(),
      Launch<GermanLane<16, 4, kBlock / 64, false, false, kGermanGamma>>::ops(),
  };
  return t;
}
}  // namespace arp
