// Kernel instantiations for the BLS12-381 pairing (kernels_pairing.hpp): a translation unit of its own beside
// k_bls12_381_g2.hip, which takes these slots into its CurveOps, so that the three compile side by side.
#include "kernels_pairing.hpp"
#include "kernels_pairing_groups.hpp"
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

// ---- ragged groups (kernels_pairing_groups.hpp) ----
int groups_grid_(int cus, size_t slots) {
  static const int occ_m = occupancy_per_cu(k_pgroups_miller<CU, S>);
  static const int occ_p = occupancy_per_cu(k_pgroups_product<CU>);
  return std::max(persistent_grid(occ_m, cus, slots), persistent_grid(occ_p, cus, slots));
}
hipError_t groups_(hipStream_t s, int cus, size_t n, size_t terms, const uint64_t* offsets, const uint8_t* g1, const uint8_t* g1_inf,
                   const uint8_t* g2, const uint8_t* g2_inf, uint32_t* tbuf, uint32_t* cbuf, uint32_t* fbuf, uint32_t* cstart,
                   uint8_t* tflag, uint8_t* status, uint32_t* slab, uint32_t opts) {
  static const int occ_m = occupancy_per_cu(k_pgroups_miller<CU, S>);
  static const int occ_p = occupancy_per_cu(k_pgroups_product<CU>);
  const size_t slots = n + terms / PGROUPS_CHUNK;
  hipLaunchKernelGGL(k_pgroups_scan, dim3(1), dim3(PGROUPS_SCAN_WG), 0, s, n, terms, offsets, cstart, status);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (terms) {
    const int pgrid = (int)std::min<size_t>((terms + WG - 1) / WG, 4096);
    hipLaunchKernelGGL((k_pgroups_prepare<CU, G>), dim3(pgrid), dim3(WG), 0, s, terms, g1, g1_inf, g2, g2_inf, tbuf, tflag, opts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((k_pgroups_miller<CU, S>), dim3(persistent_grid(occ_m, cus, slots)), dim3(WG), 0, s, n, terms, offsets, cstart,
                       tflag, tbuf, cbuf, status, slab);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the longest group (n, terms) allow has ceil(terms / K) chunks: passes until one value is left of it
    const uint64_t longest = (terms + PGROUPS_CHUNK - 1) / PGROUPS_CHUNK;
    for (uint64_t stride = 1; stride < longest; stride *= PGROUPS_FANIN) {
      hipLaunchKernelGGL((k_pgroups_product<CU>), dim3(persistent_grid(occ_p, cus, slots)), dim3(WG), 0, s, n, cstart, cbuf, stride, slab);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  const int ggrid = (int)std::min<size_t>((n + WG - 1) / WG, 4096);
  hipLaunchKernelGGL((k_pgroups_gather<CU>), dim3(ggrid), dim3(WG), 0, s, n, cstart, cbuf, fbuf);
  return hipGetLastError();
}
}  // namespace

void pairing_ops_BLS12_381_G2(CurveOps& t) {
  t.pairing_miller = miller_;
  t.pairing_finalexp = finalexp_;
  t.pairing_miller_grid = miller_grid_;
  t.pairing_finalexp_grid = finalexp_grid_;
  t.pairing_row_words = PAIRING_ROW_WORDS;
  t.pairing_slab_words = PAIRING_SLAB_WORDS;
  t.pairing_groups = groups_;
  t.pairing_groups_grid = groups_grid_;
  t.pairing_group_chunk = PGROUPS_CHUNK;
  t.pairing_group_fanin = PGROUPS_FANIN;
}
}  // namespace eccx
