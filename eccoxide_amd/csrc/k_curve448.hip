// Kernel instantiations for curve448: the X448 ladder and its normalisation (kernels_x448.hpp).
#include "kernels_x448.hpp"
#include "launch.hpp"

namespace eccx {
hipError_t launch_x448_ladder(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* u, uint32_t* rows,
                              uint8_t* flags, uint32_t opts) {
  hipLaunchKernelGGL(k_x448_ladder_unsat<CURVE448U>, dim3(grid), dim3(WG), 0, s, n, scalars, u, rows, flags, opts);
  return hipGetLastError();
}
hipError_t launch_x448_to_u(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags) {
  hipLaunchKernelGGL((k_batch_to_affine_unsat<CURVE448U, NORM_MONTGOMERY_U, X448_NORM_U>), dim3(grid), dim3(WG), 0, s, n, rows, out,
                     flags);
  return hipGetLastError();
}
int x448_ladder_grid(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_x448_ladder_unsat<CURVE448U>);
  return persistent_grid(occ, cus, n);
}
int x448_row_words() { return urow3_words<CURVE448U>(); }
int x448_norm_units() { return X448_NORM_U; }
}  // namespace eccx
