// Test-only library: KZG's vector kernel in the scalar field Fr (eccoxide_amd/csrc/kernels_kzg.hpp) run ALONE, on host
// buffers, for tests/test_kzg_stages_gpu.py to compare the values, the quotient evaluations and the flags with the Python
// model byte for byte -- the product's eccx_kzg_open never hands the quotients out.
//   kzgcheck_eval_quotient   m polynomials of N evaluations (N a power of two): ys, quot (or null: the evaluation alone) and
//                            flags; ninv_be is N^-1 mod r as the CALLER computed it, 32 big-endian bytes.  The outputs are
//                            filled with 0xAA first, so that zero bytes of a rejected polynomial are bytes the kernel wrote.
// Returns a hipError_t, or -1 for a bad argument.  Not part of the product; built by __graft_entry__.build().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_kzg.hpp"

extern "C" int kzgcheck_eval_quotient(size_t N, size_t m, const uint8_t* polys, const uint8_t* zs, const uint8_t* domain,
                                      const uint8_t* ninv_be, uint8_t* ys, uint8_t* quot, uint8_t* flags) {
  using namespace eccx;
  if (N == 0 || (N & (N - 1)) != 0 || m == 0 || !polys || !zs || !domain || !ninv_be || !ys || !flags) return -1;
  int lg = 0;
  while (((size_t)1 << lg) < N) ++lg;
  KzgFr ninv;
  for (int k = 0; k < 8; ++k)
    ninv.w[k] = (uint32_t)ninv_be[31 - 4 * k] | (uint32_t)ninv_be[30 - 4 * k] << 8 | (uint32_t)ninv_be[29 - 4 * k] << 16 |
                (uint32_t)ninv_be[28 - 4 * k] << 24;
  const size_t pb = m * N * 32, wb = kzg_ws_words(N, m) * sizeof(uint32_t);
  uint8_t *d_p = nullptr, *d_z = nullptr, *d_d = nullptr, *d_y = nullptr, *d_q = nullptr, *d_f = nullptr;
  uint32_t* d_ws = nullptr;
  hipError_t e = hipMalloc(&d_p, pb);
  if (e == hipSuccess) e = hipMalloc(&d_z, m * 32);
  if (e == hipSuccess) e = hipMalloc(&d_d, N * 32);
  if (e == hipSuccess) e = hipMalloc(&d_y, m * 32);
  if (e == hipSuccess && quot) e = hipMalloc(&d_q, pb);
  if (e == hipSuccess) e = hipMalloc(&d_f, m);
  if (e == hipSuccess) e = hipMalloc(&d_ws, wb);
  if (e == hipSuccess) e = hipMemcpy(d_p, polys, pb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_z, zs, m * 32, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_d, domain, N * 32, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_y, 0xAA, m * 32);
  if (e == hipSuccess && quot) e = hipMemset(d_q, 0xAA, pb);
  if (e == hipSuccess) e = hipMemset(d_f, 0xAA, m);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_kzg_eval_quotient<JUBJUBU>, dim3((unsigned)m), dim3(KZG_WG), 0, 0, N, lg, d_p, d_z, d_d, ninv, d_ws, d_y, d_q, d_f);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(ys, d_y, m * 32, hipMemcpyDeviceToHost);
  if (e == hipSuccess && quot) e = hipMemcpy(quot, d_q, pb, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(flags, d_f, m, hipMemcpyDeviceToHost);
  (void)hipFree(d_p); (void)hipFree(d_z); (void)hipFree(d_d); (void)hipFree(d_y); (void)hipFree(d_q); (void)hipFree(d_f); (void)hipFree(d_ws);
  return (int)e;
}
