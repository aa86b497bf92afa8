// Kernel instantiations for the sums of ragged groups of points on BLS12-381 G1 and G2 (kernels_bls_sig.hpp): a translation
// unit of its own beside k_bls12_381.hip and k_bls12_381_g2.hip, which take these slots into their CurveOps, so that the
// three compile side by side.
#include "kernels_bls_sig.hpp"
#include "launch.hpp"

namespace eccx {
namespace {
using G1 = MsmWeierstrassA0<BLS12_381U>;
using G2 = MsmG2<BLS12_381U, BLS12_381_G2>;

template <class G>
hipError_t point_sum_(hipStream_t s, int cus, size_t n, size_t members, const uint64_t* offsets, const uint8_t* points, const uint8_t* inf,
                      uint32_t* rows, uint8_t* flags, uint32_t opts) {
  return point_sum_launch<G>(s, cus, n, members, offsets, points, inf, rows, flags, (opts & OPT_VALIDATE) != 0);
}
}  // namespace

namespace {
unsigned byte_grid(size_t n) { return (unsigned)((n + WG - 1) / WG); }
}  // namespace
hipError_t launch_bls_secret_prepare(hipStream_t s, size_t n, const uint8_t* secrets, uint8_t* sk, uint8_t* status) {
  hipLaunchKernelGGL(k_bls_secret_prepare, dim3(byte_grid(n)), dim3(WG), 0, s, n, secrets, sk, status);
  return hipGetLastError();
}
hipError_t launch_bls_secret_finish(hipStream_t s, size_t n, const uint8_t* hflags, uint8_t* status, uint8_t* out, int width, uint8_t* sk) {
  hipLaunchKernelGGL(k_bls_secret_finish, dim3(byte_grid(n)), dim3(WG), 0, s, n, hflags, status, out, width, sk);
  return hipGetLastError();
}
hipError_t launch_bls_key_flags(hipStream_t s, size_t n, uint8_t* flags) {
  hipLaunchKernelGGL(k_bls_key_flags, dim3(byte_grid(n)), dim3(WG), 0, s, n, flags);
  return hipGetLastError();
}
hipError_t launch_bls_assemble(hipStream_t s, size_t n, int min_sig, const uint8_t* key_xy, const uint8_t* key_fl, const uint8_t* sig_xy,
                               const uint8_t* sig_fl, const uint8_t* h_xy, const uint8_t* h_fl, const uint64_t* key_offsets, size_t keys,
                               uint8_t* g1, uint8_t* g1_inf, uint8_t* g2, uint8_t* g2_inf, uint8_t* verdicts) {
  hipLaunchKernelGGL(k_bls_assemble, dim3(byte_grid(n)), dim3(WG), 0, s, n, min_sig, key_xy, key_fl, sig_xy, sig_fl, h_xy, h_fl, key_offsets,
                     keys, g1, g1_inf, g2, g2_inf, verdicts);
  return hipGetLastError();
}
hipError_t launch_bls_fold(hipStream_t s, size_t n, const uint8_t* pairing_verdicts, uint8_t* verdicts) {
  hipLaunchKernelGGL(k_bls_fold, dim3(byte_grid(n)), dim3(WG), 0, s, n, pairing_verdicts, verdicts);
  return hipGetLastError();
}
hipError_t launch_bls_group_flags(hipStream_t s, size_t n, size_t terms, const uint64_t* group_offsets, const uint8_t* key_fl,
                                  const uint8_t* h_fl, uint32_t* pre) {
  if (terms == 0) return hipSuccess;
  hipLaunchKernelGGL(k_bls_group_flags, dim3(byte_grid(terms)), dim3(WG), 0, s, n, terms, group_offsets, key_fl, h_fl, pre);
  return hipGetLastError();
}
hipError_t launch_bls_assemble_groups(hipStream_t s, size_t n, size_t terms, int min_sig, const uint8_t* key_xy, const uint8_t* key_fl,
                                      const uint8_t* sig_xy, const uint8_t* sig_fl, const uint8_t* h_xy, const uint8_t* h_fl,
                                      const uint64_t* group_offsets, const uint32_t* pre, uint8_t* g1, uint8_t* g1_inf, uint8_t* g2,
                                      uint8_t* g2_inf, uint64_t* term_offsets, uint8_t* verdicts) {
  hipLaunchKernelGGL(k_bls_assemble_groups, dim3(byte_grid(terms + n)), dim3(WG), 0, s, n, terms, min_sig, key_xy, key_fl, sig_xy, sig_fl,
                     h_xy, h_fl, group_offsets, pre, g1, g1_inf, g2, g2_inf, term_offsets, verdicts);
  return hipGetLastError();
}

void point_sum_ops_BLS12_381(CurveOps& t) { t.point_sum = point_sum_<G1>; }
void point_sum_ops_BLS12_381_G2(CurveOps& t) { t.point_sum = point_sum_<G2>; }
}  // namespace eccx
