// Kernel instantiations for KZG commitments on BLS12-381 (kernels_kzg.hpp): the vector kernels in the scalar field Fr, on
// Jubjub's field classes, and the byte-moving kernels of eccx_kzg_verify.  A translation unit of its own, so that it compiles
// beside the others.
#include "kernels_kzg.hpp"
#include "launch.hpp"

namespace eccx {
namespace {
unsigned lane_grid(size_t n) { return (unsigned)((n + KZG_WG - 1) / KZG_WG); }
}  // namespace

size_t kzg_workspace_bytes(size_t N, size_t m) { return kzg_ws_words(N, m) * sizeof(uint32_t); }

hipError_t launch_kzg_eval_quotient(hipStream_t s, size_t N, size_t m, const uint8_t* polys, const uint8_t* zs, const uint8_t* domain,
                                    const uint8_t* ninv_be, uint32_t* ws, uint8_t* ys, uint8_t* quot, uint8_t* flags) {
  int lg = 0;
  while (((size_t)1 << lg) < N) ++lg;
  KzgFr ninv;
  for (int k = 0; k < 8; ++k)
    ninv.w[k] = (uint32_t)ninv_be[31 - 4 * k] | (uint32_t)ninv_be[30 - 4 * k] << 8 | (uint32_t)ninv_be[29 - 4 * k] << 16 |
                (uint32_t)ninv_be[28 - 4 * k] << 24;
  hipLaunchKernelGGL(k_kzg_eval_quotient<JUBJUBU>, dim3((unsigned)m), dim3(KZG_WG), 0, s, N, lg, polys, zs, domain, ninv, ws, ys, quot, flags);
  return hipGetLastError();
}
hipError_t launch_kzg_range(hipStream_t s, size_t N, size_t m, const uint8_t* polys, uint8_t* flags) {
  hipLaunchKernelGGL(k_kzg_range<JUBJUBU>, dim3((unsigned)m), dim3(KZG_WG), 0, s, N, polys, flags);
  return hipGetLastError();
}
hipError_t launch_kzg_finish(hipStream_t s, size_t m, const uint8_t* pre, const uint8_t* sum_fl, uint8_t* out, int width, uint8_t* flags) {
  hipLaunchKernelGGL(k_kzg_finish, dim3(lane_grid(m)), dim3(KZG_WG), 0, s, m, pre, sum_fl, out, width, flags);
  return hipGetLastError();
}
hipError_t launch_kzg_verify_prepare(hipStream_t s, size_t n, const uint8_t* zs, const uint8_t* ys, const uint8_t* c_fl, const uint8_t* p_fl,
                                     uint8_t* proof_xy, uint8_t* u1, uint8_t* u2, uint8_t* verdicts) {
  hipLaunchKernelGGL(k_kzg_verify_prepare<JUBJUB>, dim3(lane_grid(n)), dim3(KZG_WG), 0, s, n, zs, ys, c_fl, p_fl, proof_xy, u1, u2, verdicts);
  return hipGetLastError();
}
hipError_t launch_kzg_verify_assemble(hipStream_t s, size_t n, const uint8_t* a_xy, const uint8_t* a_fl, const uint8_t* proof_xy,
                                      const uint8_t* p_fl, const uint8_t* tau_g2, uint8_t* g1, uint8_t* g1_inf, uint8_t* g2,
                                      uint8_t* g2_inf, uint8_t* verdicts) {
  KzgG2 tau;
  for (int k = 0; k < 192; ++k) tau.b[k] = tau_g2[k];
  hipLaunchKernelGGL(k_kzg_verify_assemble, dim3(lane_grid(n)), dim3(KZG_WG), 0, s, n, a_xy, a_fl, proof_xy, p_fl, tau, g1, g1_inf, g2, g2_inf,
                     verdicts);
  return hipGetLastError();
}
}  // namespace eccx
