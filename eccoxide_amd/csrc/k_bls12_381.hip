// Kernel instantiations for BLS12_381 (see k_weierstrass.inc) + the a = 0 / endomorphism kernels (kernels_bls.hpp).
#define ECCX_CURVE BLS12_381
#define ECCX_CURVE_U BLS12_381U
#define ECCX_OPS_NAME ops_BLS12_381
#define ECCX_CODEC_FORMAT FORMAT_ZCASH
#define ECCX_GLV_PARAMS BLS12_381_GLV
#include "kernels_bls.hpp"
#include "kernels_h2c.hpp"
#include "launch.hpp"

namespace eccx {
namespace {
hipError_t subgroup_check_(int grid, hipStream_t s, size_t n, uint8_t* xy, uint8_t* flags) {
  hipLaunchKernelGGL((k_bls_subgroup_check<BLS12_381U, BLS12_381_GLV>), dim3(grid), dim3(WG), 0, s, n, xy, flags);
  return hipGetLastError();
}
// hashing to G1 (kernels_h2c.hpp): count = 1 encode_to_curve, 2 hash_to_curve
hipError_t h2c_hash_to_field_(int grid, hipStream_t s, size_t n, const uint8_t* msgs, const uint64_t* offsets, const H2cTag& tag,
                              int count, uint32_t* rows, uint8_t* flags) {
  if (count == 2)
    hipLaunchKernelGGL((k_h2c_hash_to_field<BLS12_381U, BLS12_381_H2C, 2>), dim3(grid), dim3(WG), 0, s, n, msgs, offsets, tag, rows, flags);
  else
    hipLaunchKernelGGL((k_h2c_hash_to_field<BLS12_381U, BLS12_381_H2C, 1>), dim3(grid), dim3(WG), 0, s, n, msgs, offsets, tag, rows, flags);
  return hipGetLastError();
}
hipError_t h2c_map_finish_(int grid, hipStream_t s, size_t n, int count, uint32_t* rows) {
  if (count == 2)
    hipLaunchKernelGGL((k_h2c_map_finish<BLS12_381U, BLS12_381_H2C, BLS12_381_GLV, 2>), dim3(grid), dim3(WG), 0, s, n, rows);
  else
    hipLaunchKernelGGL((k_h2c_map_finish<BLS12_381U, BLS12_381_H2C, BLS12_381_GLV, 1>), dim3(grid), dim3(WG), 0, s, n, rows);
  return hipGetLastError();
}
int h2c_map_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_h2c_map_finish<BLS12_381U, BLS12_381_H2C, BLS12_381_GLV, 2>);
  return persistent_grid(occ, cus, n);
}
}  // namespace
}  // namespace eccx
#define ECCX_EXTRA_OPS(t)                                   \
  do {                                                      \
    (t).subgroup_check = subgroup_check_;                   \
    (t).h2c_hash_to_field = h2c_hash_to_field_;             \
    (t).h2c_map_finish = h2c_map_finish_;                   \
    (t).h2c_map_grid = h2c_map_grid_;                       \
    msm_ops_BLS12_381(t);                                   \
    msm_batch_ops_BLS12_381(t);                             \
    point_sum_ops_BLS12_381(t);                             \
  } while (0)
#include "k_weierstrass.inc"
