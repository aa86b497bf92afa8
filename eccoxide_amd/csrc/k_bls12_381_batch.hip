// Kernel instantiations for the short public-scalar multiplication on BLS12-381 G1 and G2 and for the byte-moving kernels of
// BLS batch verification (kernels_bls_batch.hpp): a translation unit of its own, so that it compiles beside the others and
// theirs stay as they were.
#include "kernels_bls_batch.hpp"
#include "launch.hpp"

namespace eccx {
namespace {
using G1 = MsmWeierstrassA0<BLS12_381U>;
using G2 = MsmG2<BLS12_381U, BLS12_381_G2>;
unsigned byte_grid(size_t n) { return (unsigned)((n + WG - 1) / WG); }
}  // namespace

hipError_t launch_scalarmul_u64(hipStream_t s, int cus, int g2, size_t n, const uint8_t* coeffs, const uint8_t* points, const uint8_t* inf,
                                uint32_t* rows, uint8_t* flags, uint32_t opts) {
  const bool validate = (opts & OPT_VALIDATE) != 0;
  return g2 ? scalarmul_u64_launch<G2>(s, cus, n, coeffs, points, inf, rows, flags, validate)
            : scalarmul_u64_launch<G1>(s, cus, n, coeffs, points, inf, rows, flags, validate);
}
hipError_t launch_bls_batch_flags(hipStream_t s, size_t n, size_t batches, const uint64_t* batch_offsets, const uint8_t* coeffs,
                                  const uint8_t* key_fl, const uint8_t* sig_fl, const uint8_t* h_fl, uint32_t* pre, uint8_t* member_status) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_bls_batch_flags, dim3(byte_grid(n)), dim3(WG), 0, s, n, batches, batch_offsets, coeffs, key_fl, sig_fl, h_fl, pre,
                     member_status);
  return hipGetLastError();
}
size_t bls_batch_pieces(size_t n, size_t batches) { return n / BATCH_PIECE + batches + 1; }
hipError_t launch_bls_batch_pieces(hipStream_t s, size_t n, size_t batches, const uint64_t* batch_offsets, uint64_t* slots,
                                   uint64_t* batch_pieces) {
  const size_t pieces = bls_batch_pieces(n, batches);
  hipError_t e = hipMemsetAsync(slots, 0xFF, (pieces + 2) * sizeof(uint64_t), s);  // PIECE_UNSET
  if (e == hipSuccess) e = hipMemsetAsync(slots, 0, sizeof(uint64_t), s);
  if (e != hipSuccess) return e;
  const size_t grid = batches < 65536 ? batches : 65536;
  hipLaunchKernelGGL(k_bls_batch_pieces, dim3((unsigned)grid), dim3(WG), 0, s, n, batches, batch_offsets, slots, batch_pieces);
  return hipGetLastError();
}
hipError_t launch_bls_batch_assemble(hipStream_t s, size_t n, size_t batches, int min_sig, const uint64_t* batch_offsets,
                                     const uint8_t* scaled, const uint8_t* scaled_fl, const uint8_t* other, const uint8_t* other_fl,
                                     const uint8_t* agg, const uint8_t* agg_fl, const uint32_t* pre, uint8_t* g1, uint8_t* g1_inf,
                                     uint8_t* g2, uint8_t* g2_inf, uint64_t* term_offsets, uint8_t* verdicts) {
  hipLaunchKernelGGL(k_bls_batch_assemble, dim3(byte_grid(n + batches)), dim3(WG), 0, s, n, batches, min_sig, batch_offsets, scaled,
                     scaled_fl, other, other_fl, agg, agg_fl, pre, g1, g1_inf, g2, g2_inf, term_offsets, verdicts);
  return hipGetLastError();
}
}  // namespace eccx
