// Test-only library: single operations of secp256k1's unsaturated field (P256K1U: 9 x 29 bits, general Montgomery
// reduction) on raw limb arrays, so that tests/test_p256k1_field.py can feed them the worst limbs their type bounds
// admit and compare with Python integers.  Not part of the product; built by __graft_entry__.build() into
// tests/hip_p256k1/libfieldcheck_k1.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "curve.hpp"
#include "inv_gcd.hpp"
#include "ufe.hpp"

namespace eccx {

using C = P256K1U;

// operand bounds of the checks: the laziest the multiplier admits without reducing (K1 K2 <= KKMAX = 6)
constexpr int KA = 3, KB = 2, KS = UB<C>::ksq_ok(2) ? 2 : 1;
static_assert(UB<C>::kk_ok(KA, KB), "check bounds");

enum : int { OP_MUL_TIGHT = 0, OP_MUL_LAZY = 1, OP_SQR_LAZY = 2, OP_SUB_CHAIN = 3, OP_REDUCE_MAX = 4,
             OP_CANONICAL = 5, OP_MUL_AUTO = 6, OP_ADD_AUTO = 7, OP_INVERT = 8,
             OP_MUL_ADD = 9,   // a (b - c) + (4p - c) d in one reduction: the Y3 of the mixed addition (kernels_coz.hpp)
             OP_MUL_BETA = 10,  // a * beta (the endomorphism's x), a at the widest bound the constant product takes
             OP_DBL_Y = 11 };   // the doubling's Y3 shape E (D - X3) - 8 C with C = B^2 (kernels_unsat.hpp ujac_dbl, a = 0)

template <int K, int V>
__device__ U<C, K, V> load_u(const uint32_t* p) {
  U<C, K, V> r;
#pragma unroll
  for (int i = 0; i < C::N; ++i) r.v[i] = p[i];
  return r;
}
template <int K, int V>
__device__ void store_u(uint32_t* p, const U<C, K, V>& a) {
#pragma unroll
  for (int i = 0; i < C::N; ++i) p[i] = a.v[i];
}

__global__ void k_field_check_k1(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                 const uint32_t* __restrict__ c, const uint32_t* __restrict__ d, uint32_t* __restrict__ out,
                                 size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int N = C::N;
  constexpr int KM = UB<C>::KMAX;
  const uint32_t* pa = a + i * N;
  const uint32_t* pb = b + i * N;
  const uint32_t* pc = c + i * N;
  const uint32_t* pd = d + i * N;
  uint32_t* po = out + i * N;
  switch (op) {
    case OP_MUL_TIGHT: store_u(po, u_mul(load_u<1, 3>(pa), load_u<1, 3>(pb))); break;
    case OP_MUL_LAZY: store_u(po, u_mul(load_u<KA, 7>(pa), load_u<KB, 4>(pb))); break;
    case OP_SQR_LAZY: store_u(po, u_sqr(load_u<KS, 5>(pa))); break;
    case OP_SUB_CHAIN: {
      auto x = load_u<1, 3>(pa);
      auto y = load_u<1, 3>(pb);
      store_u(po, u_reduce(u_sub(u_sub(u_sub(x, y), y), y)));
      break;
    }
    case OP_REDUCE_MAX: store_u(po, u_reduce(load_u<KM, 64>(pa))); break;
    case OP_CANONICAL: {
      Fe<C::Sat::L> s;
      u_to_canonical<C>(s, load_u<KM, 64>(pa));
#pragma unroll
      for (int k = 0; k < N; ++k) po[k] = k < C::Sat::L ? s.v[k] : 0u;
      break;
    }
    case OP_MUL_AUTO: store_u(po, u_mul(load_u<KM, 64>(pa), load_u<KM, 64>(pb))); break;
    case OP_ADD_AUTO: {
      auto x = load_u<KM, 64>(pa);
      auto y = load_u<KM, 64>(pb);
      store_u(po, u_reduce(u_add(u_add(x, y), u_add(x, y))));
      break;
    }
    case OP_INVERT: {
      Fe<C::Sat::L> x, y;
#pragma unroll
      for (int k = 0; k < C::Sat::L; ++k) x.v[k] = pa[k];
      fe_inv_gcd<typename C::Sat>(y, x);
#pragma unroll
      for (int k = 0; k < N; ++k) po[k] = k < C::Sat::L ? y.v[k] : 0u;
      break;
    }
    case OP_MUL_ADD: {
      const auto cc = load_u<1, 3>(pc);
      store_u(po, u_mul_add(load_u<1, 3>(pa), u_sub(load_u<1, 3>(pb), cc), u_neg(cc), load_u<1, 3>(pd)));
      break;
    }
    case OP_MUL_BETA: store_u(po, u_mul_k<C>(load_u<KM, 64>(pa), C::BETA)); break;
    case OP_DBL_Y: {  // E (D - X3) - 8 C with E = a, D = b, X3 = c, C = d^2 (the a = 0 ladder doubling's tail)
      const auto e = load_u<1, 3>(pa);
      const auto cs = u_sqr(load_u<1, 3>(pd));
      const auto c2 = u_add(cs, cs);
      const auto c4 = u_add(c2, c2);
      const auto c8 = u_reduce(u_add(c4, c4));
      store_u(po, u_reduce(u_sub(u_mul(e, u_sub(load_u<1, 3>(pb), load_u<1, 3>(pc))), c8)));
      break;
    }
    default: break;
  }
}

}  // namespace eccx

extern "C" {

// info[0..7] = N, B, KMAX, KKMAX, KA, KB, KS, L
int fieldcheck_k1_info(int* info) {
  using namespace eccx;
  info[0] = C::N; info[1] = C::B; info[2] = UB<C>::KMAX; info[3] = UB<C>::KKMAX;
  info[4] = KA; info[5] = KB; info[6] = KS; info[7] = C::Sat::L;
  return 0;
}

// one operation over n rows of N limbs (host pointers, four operand arrays); returns 0 or a hipError_t
int fieldcheck_k1_run4(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out,
                       size_t n) {
  using namespace eccx;
  const size_t bytes = n * (size_t)C::N * sizeof(uint32_t);
  uint32_t* dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipError_t e = hipSuccess;
  for (int k = 0; k < 5 && e == hipSuccess; ++k) e = hipMalloc(&dev[k], bytes);
  const uint32_t* src[4] = {a, b, c, d};
  for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemcpy(dev[k], src[k], bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dev[4], 0, bytes);
  if (e == hipSuccess) {
    const int wg = 128;
    const int grid = (int)((n + wg - 1) / wg);
    hipLaunchKernelGGL(k_field_check_k1, dim3(grid), dim3(wg), 0, 0, op, dev[0], dev[1], dev[2], dev[3], dev[4], n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dev[4], bytes, hipMemcpyDeviceToHost);
  for (int k = 0; k < 5; ++k)
    if (dev[k]) (void)hipFree(dev[k]);
  return (int)e;
}
}
