// Test-only library: P-256's doubled square (ufe.hpp u_sqr2), its merged products with a signed second factor
// (US, u_sdiff, u_mul_sub / u_mul_sub_2sqr on u_mul_sub_core_pp1) and the public ladder's doubling and mixed
// addition built on them (kernels_unsat.hpp ujac_dbl_merged, kernels_coz.hpp ujac_madd_signed), run on raw limb
// arrays so that tests/test_p256_signed_operands.py can feed them the worst operands their types admit and compare
// with Python integers.  The mixed addition as it was before the signed operands is kept here, and only here, as a
// second opinion.  Not part of the product; built by __graft_entry__.build() into tests/hip_signed/libsignedcheck.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_coz.hpp"

namespace eccx {

enum : int { SOP_SQR2 = 0,            // in0 -> 2 in0^2
             SOP_MUL_SUB_S = 1,       // in0 * (in1 - in2) - in3 * in4 (+ p)
             SOP_MUL_SUB_2SQR_S = 2,  // in0 * (in1 - in2) - 2 in3^2 (+ p)
             SOP_DBL = 3,             // (x, y, z) = in0..2 -> ujac_dbl_merged, then ujac_dbl: x3, y3, z3, x3', y3', z3'
             SOP_MADD_POS = 4,        // (x, y, z) = in0..2 + (in3, in4): ujac_madd_signed, then the former addition:
             SOP_MADD_NEG = 5,        //   x3, y3, z3, x3', y3', z3', then one row of flags (h_zero, r_zero, h_zero', r_zero')
             SOP_COUNT = 6 };

template <class C, int K, int V>
__device__ U<C, K, V> load_s(const uint32_t* p) {
  U<C, K, V> r;
#pragma unroll
  for (int i = 0; i < C::N; ++i) r.v[i] = p[i];
  return r;
}
template <class C, int K, int V>
__device__ void store_s(uint32_t* p, const U<C, K, V>& a) {
#pragma unroll
  for (int i = 0; i < C::N; ++i) p[i] = a.v[i];
}

// r = p + (x2, +-y2, 1) as the ladder computed it before the signed operands: v - x3 biased and reduced in front of
// the merged product
template <class CU>
__device__ void madd_signed_former(UJac<CU>& r, bool& h_zero, bool& r_zero, const UJac<CU>& p, const U<CU, 1, 3>& x2,
                                   const U<CU, 1, 3>& y2, bool neg) {
  auto z1z1 = u_sqr(p.z);
  auto u2 = u_mul(x2, z1z1);
  auto t = u_mul(p.z, z1z1);
  U<CU, 2, 4> sy;
  u_select(sy, neg, u_neg(y2), u_as<2, 4>(y2));
  auto s2 = u_mul(u_reduce(sy), t);
  auto h = u_reduce(u_sub(u2, p.x));
  auto rr = u_reduce(u_sub(s2, p.y));
  h_zero = u_is_zero_mod_p(h);
  r_zero = u_is_zero_mod_p(rr);
  auto hh = u_sqr(h);
  auto hhh = u_mul(h, hh);
  auto v = u_mul(p.x, hh);
  auto r2 = u_sqr(rr);
  auto x3 = u_reduce(u_sub(u_sub(u_sub(r2, hhh), v), v));
  r.x = x3;
  r.y = u_mul_sub(rr, u_reduce(u_sub(v, x3)), p.y, hhh);
  r.z = u_fit<UJac<CU>::ZK, UJac<CU>::ZV>(u_mul(p.z, h));
}

__host__ __device__ constexpr int sop_out_rows(int op) { return op >= SOP_MADD_POS ? 7 : (op == SOP_DBL ? 6 : 1); }

// in: 5 arrays of n rows of N limbs each; out: n rows of sop_out_rows(op) * N limbs
__global__ void k_signed_check(int op, const uint32_t* __restrict__ in0, const uint32_t* __restrict__ in1,
                               const uint32_t* __restrict__ in2, const uint32_t* __restrict__ in3,
                               const uint32_t* __restrict__ in4, uint32_t* __restrict__ out, size_t n) {
  using C = P256U;
  constexpr int N = C::N;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* p0 = in0 + i * N;
  const uint32_t* p1 = in1 + i * N;
  const uint32_t* p2 = in2 + i * N;
  const uint32_t* p3 = in3 + i * N;
  const uint32_t* p4 = in4 + i * N;
  uint32_t* po = out + i * (size_t)sop_out_rows(op) * N;
  switch (op) {
    case SOP_SQR2:
      store_s(po, u_sqr2(load_s<C, 1, 3>(p0)));
      break;
    case SOP_MUL_SUB_S:
      store_s(po, u_mul_sub(load_s<C, 1, 3>(p0), u_sdiff(load_s<C, 1, 3>(p1), load_s<C, 1, 3>(p2)), load_s<C, 1, 3>(p3),
                            load_s<C, 1, 3>(p4)));
      break;
    case SOP_MUL_SUB_2SQR_S:
      store_s(po, u_mul_sub_2sqr(load_s<C, 1, 3>(p0), u_sdiff(load_s<C, 1, 3>(p1), load_s<C, 1, 3>(p2)), load_s<C, 1, 3>(p3)));
      break;
    case SOP_DBL: {  // x, y tight and below 3p, z with limbs below 2 * 2^B and value below 4p
      UJac<C> p, r, s;
      p.x = load_s<C, 1, 3>(p0);
      p.y = load_s<C, 1, 3>(p1);
      p.z = load_s<C, UJac<C>::ZK, UJac<C>::ZV>(p2);
      ujac_dbl_merged<C>(r, p);
      ujac_dbl<C>(s, p);
      store_s(po, r.x);
      store_s(po + N, r.y);
      store_s(po + 2 * N, r.z);
      store_s(po + 3 * N, s.x);
      store_s(po + 4 * N, s.y);
      store_s(po + 5 * N, s.z);
      break;
    }
    case SOP_MADD_POS:
    case SOP_MADD_NEG: {
      UJac<C> p, r, s;
      p.x = load_s<C, 1, 3>(p0);
      p.y = load_s<C, 1, 3>(p1);
      p.z = load_s<C, UJac<C>::ZK, UJac<C>::ZV>(p2);
      const auto x2 = load_s<C, 1, 3>(p3);
      const auto y2 = load_s<C, 1, 3>(p4);
      bool hz, rz, hz2, rz2;
      ujac_madd_signed<C>(r, hz, rz, p, x2, y2, op == SOP_MADD_NEG);
      madd_signed_former<C>(s, hz2, rz2, p, x2, y2, op == SOP_MADD_NEG);
      store_s(po, r.x);
      store_s(po + N, r.y);
      store_s(po + 2 * N, r.z);
      store_s(po + 3 * N, s.x);
      store_s(po + 4 * N, s.y);
      store_s(po + 5 * N, s.z);
#pragma unroll
      for (int k = 0; k < N; ++k) po[6 * N + k] = 0;
      po[6 * N] = hz;
      po[6 * N + 1] = rz;
      po[6 * N + 2] = hz2;
      po[6 * N + 3] = rz2;
      break;
    }
    default: break;
  }
}

}  // namespace eccx

extern "C" {

// N, B of the field the checks run on, and the number of operations
int signedcheck_info(int* info) {
  info[0] = eccx::P256U::N;
  info[1] = eccx::P256U::B;
  info[2] = eccx::SOP_COUNT;
  return 0;
}

// runs one operation over n rows (host pointers; in: 5 arrays of n * N words, out: n * rows(op) * N words); returns 0
// or a hipError_t
int signedcheck_run(int op, const uint32_t* const* in, uint32_t* out, size_t n) {
  constexpr int N = eccx::P256U::N;
  if (op < 0 || op >= eccx::SOP_COUNT || n == 0) return -1;
  const size_t in_bytes = n * N * sizeof(uint32_t);
  const size_t out_bytes = (size_t)eccx::sop_out_rows(op) * in_bytes;
  uint32_t* dev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipError_t e = hipSuccess;
  for (int k = 0; k < 6 && e == hipSuccess; ++k) e = hipMalloc(&dev[k], k < 5 ? in_bytes : out_bytes);
  for (int k = 0; k < 5 && e == hipSuccess; ++k) e = hipMemcpy(dev[k], in[k], in_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dev[5], 0, out_bytes);
  if (e == hipSuccess) {
    const int wg = 64;
    hipLaunchKernelGGL(eccx::k_signed_check, dim3((unsigned)((n + wg - 1) / wg)), dim3(wg), 0, 0, op, dev[0], dev[1], dev[2],
                       dev[3], dev[4], dev[5], n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dev[5], out_bytes, hipMemcpyDeviceToHost);
  for (int k = 0; k < 6; ++k)
    if (dev[k]) (void)hipFree(dev[k]);
  return (int)e;
}
}
