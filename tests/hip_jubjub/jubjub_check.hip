// Test-only library: the unsaturated field JUBJUBU (ufe.hpp, general Montgomery, 9 limbs of 29 bits, R = 2^261) run on
// raw limb arrays at the largest limb and value bounds the operand types admit, one doubling and one addition of the
// Edwards ladder (kernels_unsat.hpp) and the Tonelli-Shanks root (kernels_jubjub.hpp), so that
// tests/test_jubjub_field_gpu.py can compare with Python integers and check the bounds each result's type claims.  Not
// part of the product; built by __graft_entry__.build() into tests/hip_jubjub/libjubjubcheck.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_jubjub.hpp"

namespace eccx {

using C = JUBJUBU;
using CS = JUBJUB;
constexpr int N = C::N;
static_assert(UB<C>::KKMAX == 6 && UB<C>::KMAX == 7 && C::RP == 70, "the budget the row layouts of the Edwards kernels were sized for");

// operations; rows are N = 9 words per element unless said otherwise
enum {
  OP_MUL_5_1 = 0,   // u_mul(U<5, 10>, U<1, 3>)
  OP_MUL_3_2 = 1,   // u_mul(U<3, 6>, U<2, 4>): K1 K2 = KKMAX
  OP_SQR_2 = 2,     // u_sqr(U<2, 6>): the laziest square
  OP_ADD = 3,       // u_add(U<3, 8>, U<3, 8>)
  OP_SUB = 4,       // u_sub(U<3, 8>, U<1, 3>)
  OP_REDUCE = 5,    // u_reduce(U<7, 448>): limbs as lazy as a register allows (448 q is what a top limb below 7 * 2^29 can hold)
  OP_CANONICAL = 6, // u_to_canonical(U<3, 8>) -> 8 saturated words (in a row of 9)
  OP_DBL = 7,       // ued_dbl<true>: (x, y, z, t) -> (x, y, z, t), rows of 36 words
  OP_ADD_PT = 8,    // ued_add<true>(p, ued_cache(q)): rows of 36 words
  OP_SQRT = 9,      // 8 plain words (row of 9) -> root candidate as 8 plain words, word 8 = 1 where its square is the input
  OP_COUNT = 10
};

template <int K, int V>
__device__ U<C, K, V> load_l(const uint32_t* p) {
  U<C, K, V> r;
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = p[i];
  return r;
}
template <int K, int V>
__device__ void store_l(uint32_t* p, const U<C, K, V>& a, int* kv) {
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = a.v[i];
  kv[0] = K;
  kv[1] = V;
}
__device__ void load_pt(UEd<C>& p, const uint32_t* r) {
  p.x = load_l<1, 3>(r);
  p.y = load_l<1, 3>(r + N);
  p.z = load_l<1, 3>(r + 2 * N);
  p.t = load_l<1, 3>(r + 3 * N);
}
__device__ void store_pt(uint32_t* r, const UEd<C>& p, int* kv) {
  store_l(r, p.x, kv);
  store_l(r + N, p.y, kv);
  store_l(r + 2 * N, p.z, kv);
  store_l(r + 3 * N, p.t, kv);
}

// kv: the limb and value bounds (K, V) of the result's type, written by lane 0 (0, 0 where the result is no U<>)
__global__ void __launch_bounds__(64) k_check(int op, size_t n, int words, const uint32_t* a, const uint32_t* b, uint32_t* out, int* kv) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t *pa = a + i * words, *pb = b + i * words;
  uint32_t* po = out + i * words;
  int lkv[2] = {0, 0};
  switch (op) {
    // no operand may be reduced on the way in: the types must admit each operation as it stands
    case OP_MUL_5_1:
      static_assert(UB<C>::kk_ok(5, 1) && UB<C>::vout(10, 3) <= 3, "admitted as it is");
      store_l(po, u_mul(load_l<5, 10>(pa), load_l<1, 3>(pb)), lkv);
      break;
    case OP_MUL_3_2:
      static_assert(UB<C>::kk_ok(3, 2) && !UB<C>::kk_ok(4, 2) && UB<C>::vout(6, 4) <= 3, "at the column budget");
      store_l(po, u_mul(load_l<3, 6>(pa), load_l<2, 4>(pb)), lkv);
      break;
    case OP_SQR_2:
      static_assert(UB<C>::ksq_ok(2) && !UB<C>::ksq_ok(3) && UB<C>::vout(6, 6) <= 3, "the laziest square");
      store_l(po, u_sqr(load_l<2, 6>(pa)), lkv);
      break;
    case OP_ADD:
      store_l(po, u_add(load_l<3, 8>(pa), load_l<3, 8>(pb)), lkv);
      break;
    case OP_SUB:
      store_l(po, u_sub(load_l<3, 8>(pa), load_l<1, 3>(pb)), lkv);
      break;
    case OP_REDUCE:
      store_l(po, u_reduce(load_l<7, 448>(pa)), lkv);
      break;
    case OP_CANONICAL: {
      Fe<CS::L> c;
      u_to_canonical<C>(c, load_l<3, 8>(pa));
#pragma unroll
      for (int k = 0; k < N; ++k) po[k] = k < CS::L ? c.v[k] : 0u;
      break;
    }
    case OP_DBL: {
      UEd<C> p, r;
      load_pt(p, pa);
      ued_dbl<C, true>(r, p);
      store_pt(po, r, lkv);
      break;
    }
    case OP_ADD_PT: {
      UEd<C> p, q, r;
      load_pt(p, pa);
      load_pt(q, pb);
      UEdCached<C> c;
      ued_cache<C>(c, q);
      ued_add<C, true>(r, p, c, false);
      store_pt(po, r, lkv);
      break;
    }
    case OP_SQRT: {
      Fe<CS::L> plain, c;
#pragma unroll
      for (int k = 0; k < CS::L; ++k) plain.v[k] = pa[k];
      const UT<C> x = u_as<1, 3>(u_to_mont<C>(plain));
      const UT<C> r = ut_sqrt_ts<C>(x);
      u_to_canonical<C>(c, r);
#pragma unroll
      for (int k = 0; k < CS::L; ++k) po[k] = c.v[k];
      po[CS::L] = ut_equal(u_sqr(r), x) ? 1u : 0u;
      break;
    }
    default: break;
  }
  if (i == 0) { kv[0] = lkv[0]; kv[1] = lkv[1]; }
}

}  // namespace eccx

// words: 9 or 36 per row (OP_DBL, OP_ADD_PT).  Returns 0, or a negative number for a HIP error / bad argument.
extern "C" int jubjub_check(int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out, int* kv) {
  using namespace eccx;
  if (op < 0 || op >= OP_COUNT || !a || !b || !out || !kv) return -2;
  if (n == 0) return 0;
  const int words = (op == OP_DBL || op == OP_ADD_PT) ? 4 * N : N;
  const size_t bytes = n * (size_t)words * sizeof(uint32_t);
  uint32_t *da = nullptr, *db = nullptr, *dout = nullptr;
  int* dkv = nullptr;
  int rc = -3;
  if (hipMalloc(&da, bytes) == hipSuccess && hipMalloc(&db, bytes) == hipSuccess && hipMalloc(&dout, bytes) == hipSuccess &&
      hipMalloc(&dkv, 2 * sizeof(int)) == hipSuccess && hipMemcpy(da, a, bytes, hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(db, b, bytes, hipMemcpyHostToDevice) == hipSuccess && hipMemset(dout, 0, bytes) == hipSuccess) {
    hipLaunchKernelGGL(k_check, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, op, n, words, da, db, dout, dkv);
    if (hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
        hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(kv, dkv, 2 * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess)
      rc = 0;
  }
  (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout); (void)hipFree(dkv);
  return rc;
}
