// Test-only library: the Goldilocks field layer (ufe.hpp, kind 4: p = 2^448 - 2^224 - 1 as 16 limbs of 28 bits) and one
// X448 ladder step (kernels_x448.hpp), run on raw limb arrays at the largest limb bounds their types admit so that
// tests/test_x448_field_gpu.py can compare with Python integers and check the bounds each result's type claims.  Not
// part of the product; built by __graft_entry__.build() into tests/hip_x448/libx448check.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "curve.hpp"
#include "inv_gcd.hpp"
#include "kernels_x448.hpp"

namespace eccx {

using C = CURVE448U;
using CS = CURVE448;
constexpr int N = C::N;
constexpr int KK = UB<C>::KKMAX;  // 15: 16 products of limbs below 2^28 per column
constexpr int KS = 3;             // the laziest square: K^2 <= KKMAX and the doubled operand below 2^32
static_assert(UB<C>::ksq_ok(KS) && !UB<C>::ksq_ok(KS + 1), "laziest square");
static_assert(KK == 15 && UB<C>::kk_ok(5, 3) && UB<C>::kk_ok(15, 1) && !UB<C>::kk_ok(4, 4), "operands at the column budget");

// what an operation does and the formats of its rows: L limbs (16 words), W the 14 words of the saturated twin (in a
// row of 16), Y 56 bytes (in a row of 16 words), S3 three elements (48 words), S4 four elements (64 words)
enum { OP_MUL, OP_SQR, OP_ADD_MUL, OP_SUB_REDUCE, OP_MUL_SMALL, OP_CANONICAL, OP_LOAD, OP_STORE, OP_INVERT, OP_STEP };
struct XOp {
  int what, k1, v1, k2, v2;  // operand types (K, V); k2 = 0: no second operand
  int aw, bw, ow;            // words per row of a, b, out
};
constexpr XOp OPS[] = {
    {OP_MUL, 5, 5, 3, 3, 16, 16, 16},          // 0  KKMAX split 5 x 3
    {OP_MUL, 3, 3, 5, 5, 16, 16, 16},          // 1  ... and 3 x 5
    {OP_MUL, 15, 15, 1, 2, 16, 16, 16},        // 2  one operand as lazy as a register allows
    {OP_SQR, KS, 3, 0, 0, 16, 16, 16},         // 3  the laziest square
    {OP_SQR, 1, 2, 0, 0, 16, 16, 16},          // 4
    {OP_MUL, 1, 2, 1, 2, 16, 16, 16},          // 5  the common case
    {OP_ADD_MUL, 1, 2, 1, 2, 16, 16, 16},      // 6  (a + b) * b
    {OP_SUB_REDUCE, 2, 2, 1, 2, 16, 16, 16},   // 7  u_reduce(a - b)
    {OP_MUL_SMALL, 3, 3, 0, 0, 16, 16, 16},    // 8  a * 39082
    {OP_CANONICAL, 15, 15, 0, 0, 16, 16, 16},  // 9  the residue below p, saturated words
    {OP_LOAD, 1, 2, 0, 0, 16, 16, 16},         // 10 56 bytes -> limbs
    {OP_STORE, 1, 2, 0, 0, 16, 16, 16},        // 11 limbs -> 56 canonical little-endian bytes
    {OP_INVERT, 1, 2, 0, 0, 16, 16, 16},       // 12 1 / a with 0 -> 0, as the normalisation does it
    {OP_STEP, 1, 2, 1, 2, 48, 48, 64},         // 13 (x1, x2, z2), (x3, z3, bit) -> (x2, z2, x3, z3)
};
constexpr int XOP_COUNT = sizeof(OPS) / sizeof(OPS[0]);

template <int K, int V>
__device__ U<C, K, V> load_l(const uint32_t* p) {
  U<C, K, V> r;
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = p[i];
  return r;
}
template <int K, int V>
__device__ void store_l(uint32_t* p, const U<C, K, V>& a) {
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = a.v[i];
}
template <int K, int V>
constexpr int kbound(const U<C, K, V>&) { return K; }
template <int K, int V>
constexpr int vbound(const U<C, K, V>&) { return V; }

// kv[0], kv[1]: the limb and value bounds of the result's type (0, 0 where the result is no U<>)
template <int OP>
__device__ void xop_run(const uint32_t* pa, const uint32_t* pb, uint32_t* po, int* kv) {
  constexpr XOp o = OPS[OP];
  using T = U<C, 1, 3>;
  if constexpr (o.what == OP_MUL || o.what == OP_SQR || o.what == OP_ADD_MUL || o.what == OP_SUB_REDUCE || o.what == OP_MUL_SMALL) {
    const auto a = load_l<o.k1, o.v1>(pa);
    auto fin = [&](const auto& r) {
      store_l(po, r);
      kv[0] = kbound(r);
      kv[1] = vbound(r);
    };
    // no operand may be reduced on the way in: the types must admit each operation as it is
    if constexpr (o.what == OP_MUL) {
      static_assert(UB<C>::kk_ok(o.k1, o.k2), "within the column budget");
      fin(u_mul(a, load_l<o.k2, o.v2>(pb)));
    } else if constexpr (o.what == OP_SQR) {
      static_assert(UB<C>::ksq_ok(o.k1), "within the column budget");
      fin(u_sqr(a));
    } else if constexpr (o.what == OP_ADD_MUL) {
      const auto b = load_l<o.k2, o.v2>(pb);
      fin(u_mul(u_add(a, b), b));
    } else if constexpr (o.what == OP_SUB_REDUCE) {
      fin(u_reduce(u_sub(a, load_l<o.k2, o.v2>(pb))));
    } else {
      fin(u_mul_small(a, C::A24));
    }
  } else if constexpr (o.what == OP_CANONICAL || o.what == OP_STORE) {
    Fe<CS::L> s;
    u_to_canonical<C>(s, load_l<o.k1, o.v1>(pa));
    if constexpr (o.what == OP_CANONICAL) {
#pragma unroll
      for (int i = 0; i < N; ++i) po[i] = i < CS::L ? s.v[i] : 0u;
    } else {
      po[14] = po[15] = 0;
      fe_store_le<CS>(reinterpret_cast<uint8_t*>(po), s);
    }
    kv[0] = kv[1] = 0;
  } else if constexpr (o.what == OP_LOAD) {
    const auto r = u_load_le_bytes<C>(reinterpret_cast<const uint8_t*>(pa));
    store_l(po, r);
    kv[0] = kbound(r);
    kv[1] = vbound(r);
  } else if constexpr (o.what == OP_INVERT) {
    // k_batch_to_affine_unsat's path for one unit: Z = 0 (mod p) is replaced by 1 before the inversion and the
    // output zeroed afterwards, both by selects
    T one, z = u_as<1, 3>(load_l<o.k1, o.v1>(pa));
#pragma unroll
    for (int i = 0; i < N; ++i) one.v[i] = C::ONE[i];
    const bool present = !u_is_zero_mod_p_ct(u_reduce(z));
    u_select(z, present, z, one);
    Fe<CS::L> c;
    u_to_canonical<C>(c, z);
    fe_inv_gcd<CS>(c, c);
    T inv = u_as<1, 3>(u_to_mont<C>(c)), zero;
    u_set_zero(zero);
    u_select(inv, present, inv, zero);
    store_l(po, inv);
    kv[0] = kbound(inv);
    kv[1] = vbound(inv);
  } else {
    T x1 = u_as<1, 3>(load_l<1, 2>(pa)), x2 = u_as<1, 3>(load_l<1, 2>(pa + N)), z2 = u_as<1, 3>(load_l<1, 2>(pa + 2 * N));
    T x3 = u_as<1, 3>(load_l<1, 2>(pb)), z3 = u_as<1, 3>(load_l<1, 2>(pb + N));
    const bool sw = (pb[2 * N] & 1u) != 0;
    {
      T a = x2, b = x3;
      u_select(x2, sw, b, a);
      u_select(x3, sw, a, b);
      a = z2; b = z3;
      u_select(z2, sw, b, a);
      u_select(z3, sw, a, b);
    }
    x448_step<C>(x1, x2, z2, x3, z3);
    store_l(po, x2);
    store_l(po + N, z2);
    store_l(po + 2 * N, x3);
    store_l(po + 3 * N, z3);
    kv[0] = kbound(x2);
    kv[1] = vbound(x2);
  }
}

__global__ void k_x448_check(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out,
                             int* __restrict__ kv, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int mine[2] = {0, 0};
  switch (op) {
#define ECCX_XOP_CASE(OP)                                                                                     \
  case OP:                                                                                                    \
    xop_run<OP>(a + i * OPS[OP].aw, b + i * OPS[OP].bw, out + i * OPS[OP].ow, mine);                          \
    break;
    ECCX_XOP_CASE(0) ECCX_XOP_CASE(1) ECCX_XOP_CASE(2) ECCX_XOP_CASE(3) ECCX_XOP_CASE(4) ECCX_XOP_CASE(5) ECCX_XOP_CASE(6)
    ECCX_XOP_CASE(7) ECCX_XOP_CASE(8) ECCX_XOP_CASE(9) ECCX_XOP_CASE(10) ECCX_XOP_CASE(11) ECCX_XOP_CASE(12) ECCX_XOP_CASE(13)
#undef ECCX_XOP_CASE
    default: break;
  }
  if (i == 0) {
    kv[0] = mine[0];
    kv[1] = mine[1];
  }
}

}  // namespace eccx

extern "C" {

// info = N, B, KKMAX, KLAZY (UB's: what a lazy coordinate may carry), number of operations, the small multiple, the
// laziest limb bound the squarer takes
int x448check_info(int* info) {
  info[0] = eccx::N;
  info[1] = eccx::C::B;
  info[2] = eccx::KK;
  info[3] = eccx::UB<eccx::C>::KLAZY;
  info[4] = eccx::XOP_COUNT;
  info[5] = (int)eccx::C::A24;
  info[6] = eccx::KS;
  return 0;
}

// ops[8 op .. 8 op + 7] = what, K1, V1, K2, V2 (0, 0: no second operand), words per row of a, b, out
int x448check_ops(int* ops) {
  using namespace eccx;
  for (int i = 0; i < XOP_COUNT; ++i) {
    const XOp o = OPS[i];
    const int row[8] = {o.what, o.k1, o.v1, o.k2, o.v2, o.aw, o.bw, o.ow};
    for (int j = 0; j < 8; ++j) ops[8 * i + j] = row[j];
  }
  return 0;
}

// runs one operation over n >= 1 rows (host pointers); vbound[0], vbound[1] = the limb bound K and the value bound V of
// the result's type (0, 0 where the result is words or bytes); returns 0 or a hipError_t
int x448check_run(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int* vbound, size_t n) {
  if (op < 0 || op >= eccx::XOP_COUNT || n == 0) return -1;
  static_assert(eccx::XOP_COUNT == 14, "k_x448_check has one case per operation");
  const eccx::XOp o = eccx::OPS[op];
  const size_t bytes[3] = {n * o.aw * sizeof(uint32_t), n * o.bw * sizeof(uint32_t), n * o.ow * sizeof(uint32_t)};
  uint32_t* dev[3] = {nullptr, nullptr, nullptr};
  int* dkv = nullptr;
  const uint32_t* host[2] = {a, b};
  hipError_t e = hipSuccess;
  for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipMalloc(&dev[k], bytes[k]);
  for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipMemcpy(dev[k], host[k], bytes[k], hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&dkv, 2 * sizeof(int));
  if (e == hipSuccess) e = hipMemset(dev[2], 0, bytes[2]);
  if (e == hipSuccess) e = hipMemset(dkv, 0, 2 * sizeof(int));
  if (e == hipSuccess) {
    const int wg = 64;
    hipLaunchKernelGGL(eccx::k_x448_check, dim3((unsigned)((n + wg - 1) / wg)), dim3(wg), 0, 0, op, dev[0], dev[1], dev[2], dkv, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dev[2], bytes[2], hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(vbound, dkv, 2 * sizeof(int), hipMemcpyDeviceToHost);
  for (int k = 0; k < 3; ++k)
    if (dev[k]) (void)hipFree(dev[k]);
  if (dkv) (void)hipFree(dkv);
  return (int)e;
}
}
