// Test-only library: P-256's Montgomery product and square (ufe.hpp u_mul_core_mont, whose columns 0..N-2 take
// the whole low word as the Montgomery digit, UB::LO32) at the largest limb and value bounds their types admit,
// run on raw limb arrays so that tests/test_p256_lo32.py can compare with Python integers and check the value
// bound the result's type claims.  Not part of the product; built by __graft_entry__.build() into
// tests/hip_lo32/liblo32check.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "curve.hpp"
#include "ufe.hpp"

namespace eccx {

using C = P256U;
constexpr int KK = UB<C>::KKMAX;  // 6 for 9 x 29 bits
constexpr int KS = UB<C>::KLAZY;  // largest limb bound a square takes: 2

// operand types of each operation, (K1, V1) x (K2, V2) (a square: K2 = V2 = 0).  The value bounds are the largest
// whose vout() is 3 (V1 V2 = 63 < 2 RP); op 4 sits where RP divides V1 V2 (the one case the 32-bit digits move vout())
struct LOp {
  int k1, v1, k2, v2;
};
constexpr LOp OPS[] = {
    {KK, 7, 1, 9},  // columns at KKMAX: one operand as lazy as the budget allows
    {2, 7, 3, 9},   // KKMAX split 2 x 3
    {KS, 7, 0, 0},  // the laziest square
    {1, 3, 1, 3},   // the ladder's common case
    {1, 4, 1, 8},   // V1 V2 = RP
};
constexpr int LOP_COUNT = sizeof(OPS) / sizeof(OPS[0]);

template <int K, int V>
__device__ U<C, K, V> load_l(const uint32_t* p) {
  U<C, K, V> r;
#pragma unroll
  for (int i = 0; i < C::N; ++i) r.v[i] = p[i];
  return r;
}
template <int K, int V>
__device__ void store_l(uint32_t* p, const U<C, K, V>& a) {
#pragma unroll
  for (int i = 0; i < C::N; ++i) p[i] = a.v[i];
}
// the value bound of the result's type (its K is 1)
template <int K, int V>
constexpr int vbound(const U<C, K, V>&) {
  static_assert(K == 1, "products are tight");
  return V;
}

// the product of operation OP, with no reduction of an operand: the types must admit it as it is
template <int OP>
__device__ auto lop_result(const uint32_t* pa, const uint32_t* pb) {
  constexpr LOp o = OPS[OP];
  if constexpr (o.k2 == 0) return u_sqr(load_l<o.k1, o.v1>(pa));
  else return u_mul(load_l<o.k1, o.v1>(pa), load_l<o.k2, o.v2>(pb));
}
static_assert(UB<C>::kk_ok(OPS[0].k1, OPS[0].k2) && UB<C>::kk_ok(OPS[1].k1, OPS[1].k2) && UB<C>::ksq_ok(OPS[2].k1) &&
                  OPS[0].k1 * OPS[0].k2 == UB<C>::KKMAX && OPS[1].k1 * OPS[1].k2 == UB<C>::KKMAX,
              "operands at the column budget");

// out: n rows of N limbs; vb: the value bound of the result's type
__global__ void k_lo32_check(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out,
                             int* __restrict__ vb, size_t n) {
  constexpr int N = C::N;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* pa = a + i * N;
  const uint32_t* pb = b + i * N;
  switch (op) {
#define ECCX_LOP_CASE(OP)                        \
  case OP: {                                     \
    const auto r = lop_result<OP>(pa, pb);       \
    store_l(out + i * N, r);                     \
    if (i == 0) *vb = vbound(r);                 \
    break;                                       \
  }
    ECCX_LOP_CASE(0)
    ECCX_LOP_CASE(1)
    ECCX_LOP_CASE(2)
    ECCX_LOP_CASE(3)
    ECCX_LOP_CASE(4)
#undef ECCX_LOP_CASE
    default: break;
  }
}

}  // namespace eccx

extern "C" {

// info = N, B, KKMAX, KLAZY, RP, number of operations
int lo32check_info(int* info) {
  info[0] = eccx::C::N;
  info[1] = eccx::C::B;
  info[2] = eccx::KK;
  info[3] = eccx::KS;
  info[4] = (int)eccx::C::RP;
  info[5] = eccx::LOP_COUNT;
  return 0;
}

// ops[5 op .. 5 op + 4] = K1, V1, K2, V2 (0, 0: a square), vout(V1, V2) of operation op
int lo32check_ops(int* ops) {
  using namespace eccx;
  for (int i = 0; i < LOP_COUNT; ++i) {
    const LOp o = OPS[i];
    ops[5 * i] = o.k1;
    ops[5 * i + 1] = o.v1;
    ops[5 * i + 2] = o.k2;
    ops[5 * i + 3] = o.v2;
    ops[5 * i + 4] = UB<C>::vout(o.v1, o.k2 == 0 ? o.v1 : o.v2);
  }
  return 0;
}

// runs one operation over n >= 1 rows (host pointers); *vbound = the value bound V of the result's type (result < V p);
// returns 0 or a hipError_t
int lo32check_run(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int* vbound, size_t n) {
  constexpr int N = eccx::C::N;
  if (op < 0 || op >= eccx::LOP_COUNT || n == 0) return -1;
  static_assert(eccx::LOP_COUNT == 5, "k_lo32_check has one case per operation");
  const size_t bytes = n * N * sizeof(uint32_t);
  uint32_t* dev[3] = {nullptr, nullptr, nullptr};
  int* dvb = nullptr;
  const uint32_t* host[2] = {a, b};
  hipError_t e = hipSuccess;
  for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipMalloc(&dev[k], bytes);
  for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipMemcpy(dev[k], host[k], bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&dvb, sizeof(int));
  if (e == hipSuccess) e = hipMemset(dev[2], 0, bytes);
  if (e == hipSuccess) e = hipMemset(dvb, 0, sizeof(int));
  if (e == hipSuccess) {
    const int wg = 64;
    hipLaunchKernelGGL(eccx::k_lo32_check, dim3((unsigned)((n + wg - 1) / wg)), dim3(wg), 0, 0, op, dev[0], dev[1], dev[2], dvb, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dev[2], bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(vbound, dvb, sizeof(int), hipMemcpyDeviceToHost);
  for (int k = 0; k < 3; ++k)
    if (dev[k]) (void)hipFree(dev[k]);
  if (dvb) (void)hipFree(dvb);
  return (int)e;
}
}
