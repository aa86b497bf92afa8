// Kernel instantiations for the BLS12-381 pairing (kernels_pairing.hpp): a translation unit of its own beside
// k_bls12_381_g2.hip, which takes these slots into its CurveOps, so that the three compile side by side.
#include "kernels_pairing.hpp"
#include "launch.hpp"

#include <algorithm>

namespace eccx {
namespace {
using CU = BLS12_381U;
using G = BLS12_381_G2;
using PC = BLS12_381_PAIRING;
using S = BLS12_381_GLV;

hipError_t miller_(int grid, hipStream_t s, size_t n, uint32_t pairs, const uint8_t* g1, const uint8_t* g1_inf, const uint8_t* g2,
                   const uint8_t* g2_inf, uint32_t* terms, uint32_t* fbuf, uint8_t* status, uint32_t* slab, uint32_t opts) {
  const int pgrid = (int)std::min<size_t>((n + WG - 1) / WG, 4096);
  hipLaunchKernelGGL((k_pairing_prepare<CU, G>), dim3(pgrid), dim3(WG), 0, s, n, pairs, g1, g1_inf, g2, g2_inf, terms, status, opts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_pairing_miller<CU, S>), dim3(grid), dim3(WG), 0, s, n, pairs, g1_inf, g2_inf, terms, fbuf, slab);
  return hipGetLastError();
}
hipError_t finalexp_(int grid, hipStream_t s, size_t n, uint32_t* fbuf, uint8_t* out, uint8_t* status, uint32_t* slab) {
  hipLaunchKernelGGL((k_pairing_finalexp<CU, PC, S>), dim3(grid), dim3(WG), 0, s, n, fbuf, out, status, slab);
  return hipGetLastError();
}
int miller_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_pairing_miller<CU, S>);
  return persistent_grid(occ, cus, n);
}
int finalexp_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_pairing_finalexp<CU, PC, S>);
  return persistent_grid(occ, cus, n);
}
}  // namespace

void pairing_ops_BLS12_381_G2(CurveOps& t) {
  t.pairing_miller = miller_;
  t.pairing_finalexp = finalexp_;
  t.pairing_miller_grid = miller_grid_;
  t.pairing_finalexp_grid = finalexp_grid_;
  t.pairing_row_words = PAIRING_ROW_WORDS;
  t.pairing_slab_words = PAIRING_SLAB_WORDS;
}
}  // namespace eccx
