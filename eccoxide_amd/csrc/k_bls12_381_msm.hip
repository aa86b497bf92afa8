// Kernel instantiations for the multi-scalar multiplication on BLS12-381 G1 (kernels_msm.hpp): a translation unit of its
// own beside k_bls12_381.hip, which takes these slots into its CurveOps, so that the two compile side by side.
#include "kernels_msm.hpp"
#include "launch.hpp"

namespace eccx {
namespace {
using G = MsmWeierstrassA0<BLS12_381U>;

size_t msm_bytes_(size_t n, int c) { return msm_layout<G>(n, c).bytes; }
hipError_t msm_(hipStream_t s, int cus, size_t n, int c, const uint8_t* scalars, const uint8_t* points, const uint8_t* inf, uint8_t* ws,
                uint32_t** row, uint8_t* flag, uint32_t opts) {
  return msm_launch<G>(s, cus, n, c, scalars, points, inf, ws, row, flag, (opts & OPT_VALIDATE) != 0);
}
}  // namespace

void msm_ops_BLS12_381(CurveOps& t) {
  t.msm_bytes = msm_bytes_;
  t.msm = msm_;
}
}  // namespace eccx
