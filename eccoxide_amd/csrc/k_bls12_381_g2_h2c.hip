// Kernel instantiations for hashing to BLS12-381 G2 (kernels_h2c_g2.hpp): a translation unit of its own beside
// k_bls12_381_g2.hip, which takes these slots into its CurveOps, so that the two compile side by side.
#include "kernels_h2c_g2.hpp"
#include "launch.hpp"

namespace eccx {
namespace {
using CU = BLS12_381U;
using G = BLS12_381_G2;
using HC = BLS12_381_G2_H2C;
using S = BLS12_381_GLV;

// count = 1 encode_to_curve, 2 hash_to_curve
hipError_t hash_to_field_(int grid, hipStream_t s, size_t n, const uint8_t* msgs, const uint64_t* offsets, const H2cTag& tag, int count,
                          uint32_t* rows, uint8_t* flags) {
  if (count == 2)
    hipLaunchKernelGGL((k_h2c_g2_hash_to_field<CU, HC, 2>), dim3(grid), dim3(WG), 0, s, n, msgs, offsets, tag, rows, flags);
  else
    hipLaunchKernelGGL((k_h2c_g2_hash_to_field<CU, HC, 1>), dim3(grid), dim3(WG), 0, s, n, msgs, offsets, tag, rows, flags);
  return hipGetLastError();
}
hipError_t map_(int grid, hipStream_t s, size_t n, int count, uint32_t* rows) {
  if (count == 2)
    hipLaunchKernelGGL((k_h2c_g2_map<CU, HC, 2>), dim3(grid), dim3(WG), 0, s, n, rows);
  else
    hipLaunchKernelGGL((k_h2c_g2_map<CU, HC, 1>), dim3(grid), dim3(WG), 0, s, n, rows);
  return hipGetLastError();
}
int map_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_h2c_g2_map<CU, HC, 2>);
  return persistent_grid(occ, cus, n);
}
hipError_t clear_(int grid, hipStream_t s, size_t n, uint32_t* rows) {
  hipLaunchKernelGGL((k_h2c_g2_clear<CU, G, S>), dim3(grid), dim3(WG), 0, s, n, rows);
  return hipGetLastError();
}
int clear_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_h2c_g2_clear<CU, G, S>);
  return persistent_grid(occ, cus, n);
}
}  // namespace

void h2c_ops_BLS12_381_G2(CurveOps& t) {
  t.h2c_hash_to_field = hash_to_field_;
  t.h2c_map_finish = map_;
  t.h2c_map_grid = map_grid_;
  t.h2c_clear = clear_;
  t.h2c_clear_grid = clear_grid_;
}
}  // namespace eccx
