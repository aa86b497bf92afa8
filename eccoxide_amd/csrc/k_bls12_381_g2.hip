// Kernel instantiations for BLS12-381 G2 (kernels_g2.hpp): a CurveOps of its own.  The slots of the reference-mirroring
// kernels (var, base, to_affine_hom, point_add), of the endomorphism ladders, of the wide and LDS combs, of the lane
// gather and of ECDSA stay null: the C ABI answers those requests with ECCX_ERR_ARG.
#include "kernels_g2.hpp"
#include "launch.hpp"

namespace eccx {
namespace {
using CU = BLS12_381U;
using CS = BLS12_381;
using G = BLS12_381_G2;

hipError_t var_fast_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint32_t* rows,
                     uint8_t* flags, uint32_t* scratch, uint32_t opts) {
  hipLaunchKernelGGL((k_g2_scalarmul_var<CU, G, false>), dim3(grid), dim3(WG), 0, s, n, scalars, points, rows, flags, scratch, opts);
  return hipGetLastError();
}
hipError_t var_ct_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint32_t* rows,
                   uint8_t* flags, uint32_t* scratch, uint32_t opts) {
  hipLaunchKernelGGL((k_g2_scalarmul_var<CU, G, true>), dim3(grid), dim3(WG), 0, s, n, scalars, points, rows, flags, scratch, opts);
  return hipGetLastError();
}
int var_fast_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_g2_scalarmul_var<CU, G, false>);
  return persistent_grid(occ, cus, n);
}
int var_ct_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_g2_scalarmul_var<CU, G, true>);
  return persistent_grid(occ, cus, n);
}
hipError_t to_affine_(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags) {
  hipLaunchKernelGGL(k_g2_to_affine<CU>, dim3(grid), dim3(WG), 0, s, n, rows, out, flags);
  return hipGetLastError();
}
hipError_t table_convert_(hipStream_t s, size_t entries, const uint8_t* affine, uint32_t* table) {
  hipLaunchKernelGGL(k_g2_affine_to_table<CU>, dim3((unsigned)((entries + WG - 1) / WG)), dim3(WG), 0, s, entries, affine, table);
  return hipGetLastError();
}
hipError_t base_index_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* table, uint32_t* rows,
                       uint8_t* flags) {
  hipLaunchKernelGGL((k_g2_scalarmul_base<CU, false>), dim3(grid), dim3(WG), 0, s, n, scalars, table, rows, flags);
  return hipGetLastError();
}
hipError_t base_ct_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* table, uint32_t* rows,
                    uint8_t* flags) {
  hipLaunchKernelGGL((k_g2_scalarmul_base<CU, true>), dim3(grid), dim3(WG), 0, s, n, scalars, table, rows, flags);
  return hipGetLastError();
}
hipError_t point_add_(int grid, hipStream_t s, size_t n, const uint8_t* a, const uint8_t* a_inf, const uint8_t* b,
                      const uint8_t* b_inf, uint32_t* rows, uint8_t* flags, uint32_t opts) {
  hipLaunchKernelGGL(k_g2_point_add<CU>, dim3(grid), dim3(WG), 0, s, n, a, a_inf, b, b_inf, rows, flags, opts);
  return hipGetLastError();
}
hipError_t decompress_(int grid, hipStream_t s, size_t n, const uint8_t* enc, uint8_t* out, uint8_t* flags) {
  hipLaunchKernelGGL((k_g2_decompress<CU, G>), dim3(grid), dim3(WG), 0, s, n, enc, out, flags);
  return hipGetLastError();
}
hipError_t decompress_raw_(int grid, hipStream_t s, size_t n, const uint8_t* enc, uint8_t* out, uint8_t* flags) {
  hipLaunchKernelGGL((k_g2_from_uncompressed<CU, G>), dim3(grid), dim3(WG), 0, s, n, enc, out, flags);
  return hipGetLastError();
}
hipError_t compress_(int grid, hipStream_t s, size_t n, const uint8_t* xy, const uint8_t* inf, uint8_t* out) {
  hipLaunchKernelGGL((k_g2_compress<CS, false>), dim3(grid), dim3(WG), 0, s, n, xy, inf, out);
  return hipGetLastError();
}
hipError_t compress_raw_(int grid, hipStream_t s, size_t n, const uint8_t* xy, const uint8_t* inf, uint8_t* out) {
  hipLaunchKernelGGL((k_g2_compress<CS, true>), dim3(grid), dim3(WG), 0, s, n, xy, inf, out);
  return hipGetLastError();
}
hipError_t subgroup_check_(int grid, hipStream_t s, size_t n, uint8_t* xy, uint8_t* flags) {
  hipLaunchKernelGGL((k_g2_subgroup_check<CU, G, BLS12_381_GLV>), dim3(grid), dim3(WG), 0, s, n, xy, flags);
  return hipGetLastError();
}
}  // namespace

const CurveOps& ops_BLS12_381_G2() {
  static const CurveOps o = [] {
    CurveOps t = {};
    // a coordinate is an Fp2 element: 96 bytes, c1 || c0; the lane's window table takes the 17 slab rows the host sizes
    t.info = {2 * CS::FB, CS::SB, 2 * CS::L, G2_AFF_WORDS, 0, 0, G2_SLAB_ROW_WORDS, G2_PT_WORDS};
    t.var_fast = var_fast_;
    t.var_fast_grid = var_fast_grid_;
    t.to_affine_var = to_affine_;
    t.point_add_u = point_add_;
    t.to_affine_add_u = to_affine_;
    t.enc_bytes = 2 * CS::FB;
    t.decompress = decompress_;
    t.compress = compress_;
    t.decompress_raw = decompress_raw_;
    t.compress_raw = compress_raw_;
    t.subgroup_check = subgroup_check_;
    t.coz_row_words = G2_SLAB_ROW_WORDS;
    t.var_ct = var_ct_;
    t.var_ct_grid = var_ct_grid_;
    // one table for both fixed-base forms: the reference's 4-bit comb, 64 windows x 15 entries (j + 1) 16^i G
    t.ct_bits = 4;
    t.ct_windows = G2_COMB_WINDOWS;
    t.ct_entries = G2_COMB_ENTRIES;
    t.ct_entry_words = G2_AFF_WORDS;
    t.ct_convert = table_convert_;
    t.base_ct = base_ct_;
    t.base_unsat = base_index_;
    h2c_ops_BLS12_381_G2(t);  // hashing to G2
    pairing_ops_BLS12_381_G2(t);  // the pairing
    point_sum_ops_BLS12_381_G2(t);  // sums of ragged groups
    msm_batch_ops_BLS12_381_G2(t);  // the batched multi-scalar multiplication (m = 1: the MSM on G2)
    return t;
  }();
  return o;
}
}  // namespace eccx
