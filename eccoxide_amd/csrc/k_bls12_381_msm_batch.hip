// Kernel instantiations for the batched multi-scalar multiplication over shared points on BLS12-381 G1
// (kernels_msm_batch.hpp): a translation unit of its own beside k_bls12_381_msm.hip, which k_bls12_381.hip takes into its
// CurveOps, so that the units compile side by side.
#define ECCX_MSM_UNIT batch_g1
#include "kernels_msm_batch.hpp"
#include "launch.hpp"

namespace eccx {
namespace {
using G = MsmWeierstrassA0<BLS12_381U>;

size_t msm_batch_bytes_(size_t n, size_t m, int c) { return msmb_layout<G>(n, m, c).bytes; }
hipError_t msm_batch_(hipStream_t s, int cus, size_t n, size_t m, int c, const uint8_t* scalars, const uint8_t* points, const uint8_t* inf,
                      uint8_t* ws, uint32_t** rows, uint8_t* flags, uint32_t opts) {
  return msmb_launch<G>(s, cus, n, m, c, scalars, points, inf, ws, rows, flags, (opts & OPT_VALIDATE) != 0);
}
}  // namespace

void msm_batch_ops_BLS12_381(CurveOps& t) {
  t.msm_batch_bytes = msm_batch_bytes_;
  t.msm_batch = msm_batch_;
}
}  // namespace eccx
