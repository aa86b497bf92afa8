// Kernel instantiations for Jubjub, the a = -1 twisted Edwards curve over the BLS12-381 scalar field Fr
// (src/curve/jubjub/mod.rs): the Edwards templates of edwards25519 on the curve classes JUBJUBU (general Montgomery,
// 9 x 29 bits) and JUBJUB (saturated twin, big-endian bytes), and the decoder of kernels_jubjub.hpp.
#include "kernels_ct.hpp"
#include "kernels_jubjub.hpp"
#include "launch.hpp"

namespace eccx {
namespace {
hipError_t var_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint8_t* out,
                uint8_t* flags, uint8_t* proj, uint32_t* /*scratch*/, uint32_t opts) {
  hipLaunchKernelGGL(k_ed_scalarmul_var<JUBJUB>, dim3(grid), dim3(WG), 0, s, n, scalars, points, out, flags, proj, opts);
  return hipGetLastError();
}
hipError_t base_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* table, uint8_t* out,
                 uint8_t* flags, uint8_t* proj, uint32_t opts) {
  hipLaunchKernelGGL(k_ed_scalarmul_base<JUBJUB>, dim3(grid), dim3(WG), 0, s, n, scalars, table, out, flags, proj, opts);
  return hipGetLastError();
}
hipError_t to_affine_var_(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags) {
  hipLaunchKernelGGL((k_batch_to_affine_unsat<JUBJUBU, NORM_EDWARDS, to_affine_u(JUBJUB::L)>), dim3(grid), dim3(WG), 0, s, n, rows, out,
                     flags);
  return hipGetLastError();
}
hipError_t to_affine_hom_(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags) {
  hipLaunchKernelGGL((k_batch_to_affine<JUBJUB, NORM_EDWARDS, to_affine_u(JUBJUB::L)>), dim3(grid), dim3(WG), 0, s, n, rows, out, flags);
  return hipGetLastError();
}
hipError_t comb_convert_(hipStream_t s, size_t entries, const uint8_t* affine, uint32_t* table) {
  hipLaunchKernelGGL(k_ed_affine_to_niels_unsat<JUBJUBU>, dim3((unsigned)((entries + 127) / 128)), dim3(128), 0, s, entries, affine, table, ED_U_ENTRY_WORDS);
  return hipGetLastError();
}
hipError_t base_w8_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* table, uint32_t* rows,
                    uint8_t* flags) {
  hipLaunchKernelGGL(k_ed_scalarmul_base_unsat<JUBJUBU>, dim3(grid), dim3(WG), 0, s, n, scalars, table, rows, flags);
  return hipGetLastError();
}
hipError_t var_fast_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint32_t* rows,
                     uint8_t* flags, uint32_t* scratch, uint32_t opts) {
  hipLaunchKernelGGL((k_ed_scalarmul_var_unsat<JUBJUBU, false>), dim3(grid), dim3(WG), 0, s, n, scalars, points, rows, flags, scratch,
                     opts, nullptr, nullptr);
  return hipGetLastError();
}
hipError_t var_fused_(int grid, hipStream_t s, size_t n, const uint8_t* u2, const uint8_t* q, uint32_t* rows, uint8_t* flags,
                      uint32_t* scratch, uint32_t opts, const uint8_t* u1, const uint32_t* utable) {
  hipLaunchKernelGGL((k_ed_scalarmul_var_unsat<JUBJUBU, true>), dim3(grid), dim3(WG), 0, s, n, u2, q, rows, flags, scratch, opts,
                     u1, utable);
  return hipGetLastError();
}
int var_fast_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_ed_scalarmul_var_unsat<JUBJUBU, false>);
  return persistent_grid(occ, cus, n);
}
int var_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_ed_scalarmul_var<JUBJUB>);
  return persistent_grid(occ, cus, n);
}
hipError_t point_add_(int grid, hipStream_t s, size_t n, const uint8_t* a, const uint8_t* a_fl, const uint8_t* b,
                      const uint8_t* b_fl, uint32_t* rows, uint8_t* flags, uint32_t opts) {
  hipLaunchKernelGGL(k_ed_point_add<JUBJUB>, dim3(grid), dim3(WG), 0, s, n, a, a_fl, b, b_fl, rows, flags, opts);
  return hipGetLastError();
}
hipError_t to_affine_add_u_(int grid, hipStream_t s, size_t n, const uint32_t* rows, uint8_t* out, uint8_t* flags) {
  hipLaunchKernelGGL((k_batch_to_affine_unsat<JUBJUBU, NORM_EDWARDS, to_affine_add_u(JUBJUB::L)>), dim3(grid), dim3(WG), 0, s, n, rows,
                     out, flags);
  return hipGetLastError();
}
hipError_t point_add_u_(int grid, hipStream_t s, size_t n, const uint8_t* a, const uint8_t* a_fl, const uint8_t* b,
                        const uint8_t* b_fl, uint32_t* rows, uint8_t* flags, uint32_t opts) {
  hipLaunchKernelGGL(k_ed_point_add_unsat<JUBJUBU>, dim3(grid), dim3(WG), 0, s, n, a, a_fl, b, b_fl, rows, flags, opts);
  return hipGetLastError();
}
hipError_t decompress_(int grid, hipStream_t s, size_t n, const uint8_t* enc, uint8_t* out, uint8_t* flags) {
  hipLaunchKernelGGL(k_jubjub_point_decompress<JUBJUBU>, dim3(grid), dim3(WG), 0, s, n, enc, out, flags);
  return hipGetLastError();
}
hipError_t compress_(int grid, hipStream_t s, size_t n, const uint8_t* xy, const uint8_t* /*inf: the identity is (0, 1)*/, uint8_t* out) {
  hipLaunchKernelGGL((k_point_compress<JUBJUB, FORMAT_JUBJUB>), dim3(grid), dim3(WG), 0, s, n, xy, nullptr, out);
  return hipGetLastError();
}
// secret scalars (ECCX_CT_SCAN), variable base: the windowed ladder with every table row read at every lookup
hipError_t var_ct_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint8_t* points, uint32_t* rows,
                   uint8_t* flags, uint32_t* scratch, uint32_t opts) {
  hipLaunchKernelGGL((k_ed_scalarmul_var_unsat<JUBJUBU, false, ECCX_CT_ED_VAR_BITS, true>), dim3(grid), dim3(WG), 0, s, n, scalars, points,
                     rows, flags, scratch, opts, nullptr, nullptr);
  return hipGetLastError();
}
int var_ct_grid_(int cus, size_t n) {
  static const int occ = occupancy_per_cu(k_ed_scalarmul_var_unsat<JUBJUBU, false, ECCX_CT_ED_VAR_BITS, true>);
  return persistent_grid(occ, cus, n);
}
// secret scalars (ECCX_CT_SCAN): signed windows, every entry of the window read (kernels_ct.hpp)
hipError_t ct_convert_(hipStream_t s, size_t entries, const uint8_t* affine, uint32_t* table) {
  hipLaunchKernelGGL(k_ed_affine_to_niels_unsat<JUBJUBU>, dim3((unsigned)((entries + 127) / 128)), dim3(128), 0, s, entries, affine,
                     table, ct_entry_words<JUBJUBU>());
  return hipGetLastError();
}
hipError_t base_ct_(int grid, hipStream_t s, size_t n, const uint8_t* scalars, const uint32_t* table, uint32_t* rows,
                    uint8_t* flags) {
  hipLaunchKernelGGL((k_ed_scalarmul_base_ct<JUBJUBU, false>), dim3(grid), dim3(WG), 0, s, n, scalars, table, rows, flags);
  return hipGetLastError();
}
}  // namespace
const CurveOps& ops_JUBJUB() {
  static const CurveOps o = [] {
    // no LDS-resident comb, no lane-gather comb, no protocol slots: the C ABI refuses what is null here (strict_opts)
    CurveOps t = {{JUBJUB::FB, JUBJUB::SB, JUBJUB::L, 4 * JUBJUB::L, 0, 1, ED_VAR_ROW_WORDS,
                   (urow3_words<JUBJUBU>() > row_words<JUBJUB::L>() ? urow3_words<JUBJUBU>() : row_words<JUBJUB::L>())}, var_, base_, var_fast_, nullptr, to_affine_hom_, var_grid_, var_fast_grid_, to_affine_var_, point_add_, ED_U_ENTRY_WORDS, comb_bits<JUBJUBU>(), comb_convert_, base_w8_, 0, 0, 0, 0, nullptr, var_fused_, 32, decompress_, compress_, nullptr, nullptr,
                   point_add_u_, to_affine_add_u_};
    t.ct_bits = ct_base_bits<JUBJUBU>();
    t.ct_windows = ct_base_windows<JUBJUBU>();
    t.ct_entries = ct_base_entries<JUBJUBU>();
    t.ct_entry_words = ct_entry_words<JUBJUBU>();
    t.ct_convert = ct_convert_;
    t.base_ct = base_ct_;
    t.var_ct = var_ct_;
    t.var_ct_grid = var_ct_grid_;
    t.strict_opts = 1;
    return t;
  }();
  return o;
}
}  // namespace eccx
