// Test-only library: P-256's merged products on signed columns (ufe.hpp u_mul_sub_core_pp1) and the public
// ladder's doubling built on them (kernels_unsat.hpp ujac_dbl_merged), run on raw limb arrays so that
// tests/test_p256_merged.py can feed them the worst operands their types admit and compare with Python
// integers.  Not part of the product; built by __graft_entry__.build() into tests/hip_merged/libmergedcheck.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_unsat.hpp"

namespace eccx {

enum : int { MOP_MUL_SUB = 0,       // a*b - c*d (+ p), all four tight and below 3p
             MOP_MUL_SUB_2SQR = 1,  // a*b - 2*c^2 (+ p), tight and below 3p
             MOP_DBL = 2 };         // (x, y, z) -> ujac_dbl_merged and ujac_dbl side by side: out = x3, y3, z3, x3', y3', z3'

template <class C, int K, int V>
__device__ U<C, K, V> load_m(const uint32_t* p) {
  U<C, K, V> r;
#pragma unroll
  for (int i = 0; i < C::N; ++i) r.v[i] = p[i];
  return r;
}
template <class C, int K, int V>
__device__ void store_m(uint32_t* p, const U<C, K, V>& a) {
#pragma unroll
  for (int i = 0; i < C::N; ++i) p[i] = a.v[i];
}

// a, b, c, d: n rows of N limbs each; out: n rows of N limbs (MOP_DBL: 6 N)
__global__ void k_merged_check(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                               const uint32_t* __restrict__ c, const uint32_t* __restrict__ d, uint32_t* __restrict__ out,
                               size_t n) {
  using C = P256U;
  constexpr int N = C::N;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* pa = a + i * N;
  const uint32_t* pb = b + i * N;
  const uint32_t* pc = c + i * N;
  const uint32_t* pd = d + i * N;
  switch (op) {
    case MOP_MUL_SUB:
      store_m(out + i * N, u_mul_sub(load_m<C, 1, 3>(pa), load_m<C, 1, 3>(pb), load_m<C, 1, 3>(pc), load_m<C, 1, 3>(pd)));
      break;
    case MOP_MUL_SUB_2SQR:
      store_m(out + i * N, u_mul_sub_2sqr(load_m<C, 1, 3>(pa), load_m<C, 1, 3>(pb), load_m<C, 1, 3>(pc)));
      break;
    case MOP_DBL: {  // x = a, y = b (tight, below 3p), z = c (limbs below 2 * 2^B, value below 4p)
      UJac<C> p, r, s;
      p.x = load_m<C, 1, 3>(pa);
      p.y = load_m<C, 1, 3>(pb);
      p.z = load_m<C, UJac<C>::ZK, UJac<C>::ZV>(pc);
      ujac_dbl_merged<C>(r, p);
      ujac_dbl<C>(s, p);
      uint32_t* po = out + i * 6 * N;
      store_m(po, r.x);
      store_m(po + N, r.y);
      store_m(po + 2 * N, r.z);
      store_m(po + 3 * N, s.x);
      store_m(po + 4 * N, s.y);
      store_m(po + 5 * N, s.z);
      break;
    }
    default: break;
  }
}

}  // namespace eccx

extern "C" {

// N, B of the field the checks run on
int mergedcheck_info(int* info) {
  info[0] = eccx::P256U::N;
  info[1] = eccx::P256U::B;
  return 0;
}

// runs one operation over n rows (host pointers); returns 0 or a hipError_t
int mergedcheck_run(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, size_t n) {
  constexpr int N = eccx::P256U::N;
  if (op < 0 || op > 2) return -1;
  const size_t in_bytes = n * N * sizeof(uint32_t);
  const size_t out_bytes = (op == 2 ? 6 : 1) * in_bytes;
  uint32_t* dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const uint32_t* host[4] = {a, b, c, d};
  hipError_t e = hipSuccess;
  for (int k = 0; k < 5 && e == hipSuccess; ++k) e = hipMalloc(&dev[k], k < 4 ? in_bytes : out_bytes);
  for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemcpy(dev[k], host[k], in_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dev[4], 0, out_bytes);
  if (e == hipSuccess) {
    const int wg = 64;
    hipLaunchKernelGGL(eccx::k_merged_check, dim3((unsigned)((n + wg - 1) / wg)), dim3(wg), 0, 0, op, dev[0], dev[1], dev[2], dev[3],
                       dev[4], n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dev[4], out_bytes, hipMemcpyDeviceToHost);
  for (int k = 0; k < 5; ++k)
    if (dev[k]) (void)hipFree(dev[k]);
  return (int)e;
}
}
