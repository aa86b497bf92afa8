// Test-only library: the single operations of the saturated field layer (eccoxide_amd/csrc/fe.hpp, inv_gcd.hpp's
// fe_inv_fast, and the three integer helpers of kernels_codec.hpp) for the eight FIELD classes of curve_consts.inc, over
// whole batches of chosen operands, so that tests/test_sat_layer_gpu.py can compare every word with Python integers
// (tests/sat_ref.py) at the carry and fold boundaries no scalar multiplication reaches.  Three entry points: arithmetic
// on raw limb arrays, predicates and selects, and the byte I/O at chosen alignments.  Not part of the product; built by
// __graft_entry__.build() into tests/hip_sat/libsatcheck.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fe.hpp"
#include "inv_gcd.hpp"
#include "kernels_codec.hpp"

namespace eccx {

// arithmetic ops of satcheck_op; the OP_MUL_K_* multiply by the class's own constant through fe_mul_k, whose second
// factor goes through the mac*_k chunks (wave-uniform operands) where fe_mul's goes through mac*_v
enum {
  OP_ADD = 0, OP_SUB = 1, OP_NEG = 2, OP_MUL = 3, OP_SQR = 4, OP_TO_MONT = 5, OP_FROM_MONT = 6, OP_INV = 7,
  OP_MUL_K_R2 = 8, OP_MUL_K_ONE = 9, OP_MUL_K_B = 10, OP_MUL_K_B3 = 11, OP_MUL_K_D2 = 12, OP_COUNT = 13
};
// ops of satcheck_pred: one byte per row, except the two selects and fe_neg_canonical (4 L bytes per row: a limb array)
enum {
  PR_IS_CANONICAL = 0, PR_IS_ZERO = 1, PR_EQ = 2, PR_SELECT_EVEN = 3, PR_SELECT_ODD = 4, PR_NEG_CANONICAL = 5,
  PR_GREATER = 6, PR_ALL_ZERO = 7, PR_COUNT = 8
};

template <class C, class = void> struct has_B : std::false_type {};
template <class C> struct has_B<C, std::void_t<decltype(C::B)>> : std::true_type {};
template <class C, class = void> struct has_B3 : std::false_type {};
template <class C> struct has_B3<C, std::void_t<decltype(C::B3)>> : std::true_type {};
template <class C, class = void> struct has_D2 : std::false_type {};
template <class C> struct has_D2<C, std::void_t<decltype(C::D2)>> : std::true_type {};

// CURVE448 carries R2 = ONE = 1 and N0, PP1 of a Montgomery modulus: fe_mul_impl would run a Montgomery reduction on it
// while fe_to_mont multiplies by 1, so its product, square, conversions and fe_inv_fast mean nothing, and the library
// instantiates none of them (X448 computes on CURVE448U; the saturated twin does byte I/O, fe_is_canonical and the
// normalisation's integer steps only).  It gets add, sub, neg, the predicates and the I/O here.
template <class C> constexpr bool has_product = !std::is_same_v<C, CURVE448>;

template <class C> constexpr bool op_ok(int op) {
  if (op == OP_ADD || op == OP_SUB || op == OP_NEG) return true;
  if (!has_product<C>) return false;
  if (op == OP_MUL_K_B) return has_B<C>::value;
  if (op == OP_MUL_K_B3) return has_B3<C>::value;
  if (op == OP_MUL_K_D2) return has_D2<C>::value;
  return op >= 0 && op < OP_COUNT;
}
constexpr bool op_binary(int op) { return op == OP_ADD || op == OP_SUB || op == OP_MUL; }

template <class C, int OP>
__global__ void __launch_bounds__(WG) k_sat_op(size_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                               uint32_t* __restrict__ out) {
  constexpr int L = C::L;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    Fe<L> x, y, r;
#pragma unroll
    for (int k = 0; k < L; ++k) x.v[k] = a[i * L + k];
    if constexpr (op_binary(OP)) {
#pragma unroll
      for (int k = 0; k < L; ++k) y.v[k] = b[i * L + k];
    }
    if constexpr (OP == OP_ADD) fe_add<C>(r, x, y);
    else if constexpr (OP == OP_SUB) fe_sub<C>(r, x, y);
    else if constexpr (OP == OP_NEG) fe_neg<C>(r, x);
    else if constexpr (OP == OP_MUL) fe_mul<C>(r, x, y);
    else if constexpr (OP == OP_SQR) fe_sqr<C>(r, x);
    else if constexpr (OP == OP_TO_MONT) fe_to_mont<C>(r, x);
    else if constexpr (OP == OP_FROM_MONT) fe_from_mont<C>(r, x);
    else if constexpr (OP == OP_INV) fe_inv_fast<C>(r, x);
    else if constexpr (OP == OP_MUL_K_R2) fe_mul_k<C>(r, x, C::R2);
    else if constexpr (OP == OP_MUL_K_ONE) fe_mul_k<C>(r, x, C::ONE);
    else if constexpr (OP == OP_MUL_K_B) fe_mul_k<C>(r, x, C::B);
    else if constexpr (OP == OP_MUL_K_B3) fe_mul_k<C>(r, x, C::B3);
    else fe_mul_k<C>(r, x, C::D2);
#pragma unroll
    for (int k = 0; k < L; ++k) out[i * L + k] = r.v[k];
  }
}

constexpr bool pred_binary(int op) { return op == PR_EQ || op == PR_SELECT_EVEN || op == PR_SELECT_ODD || op == PR_GREATER; }
constexpr bool pred_wide(int op) { return op == PR_SELECT_EVEN || op == PR_SELECT_ODD || op == PR_NEG_CANONICAL; }

template <class C, int OP>
__global__ void __launch_bounds__(WG) k_sat_pred(size_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                 uint8_t* __restrict__ out) {
  constexpr int L = C::L;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    Fe<L> x, y, r;
#pragma unroll
    for (int k = 0; k < L; ++k) x.v[k] = a[i * L + k];
    if constexpr (pred_binary(OP)) {
#pragma unroll
      for (int k = 0; k < L; ++k) y.v[k] = b[i * L + k];
    }
    if constexpr (pred_wide(OP)) {
      // the selects take a from the even rows (PR_SELECT_EVEN) or from the odd ones: both senses within every wavefront
      if constexpr (OP == PR_SELECT_EVEN) fe_select<C>(r, (i & 1u) == 0, x, y);
      else if constexpr (OP == PR_SELECT_ODD) fe_select<C>(r, (i & 1u) != 0, x, y);
      else fe_neg_canonical<C>(r, x);
      uint32_t* o = reinterpret_cast<uint32_t*>(out) + i * L;
#pragma unroll
      for (int k = 0; k < L; ++k) o[k] = r.v[k];
    } else {
      bool v;
      if constexpr (OP == PR_IS_CANONICAL) v = fe_is_canonical<C>(x);
      else if constexpr (OP == PR_IS_ZERO) v = fe_is_zero<C>(x);
      else if constexpr (OP == PR_EQ) v = fe_eq<C>(x, y);
      else if constexpr (OP == PR_GREATER) v = fe_greater<L>(x, y);
      else v = fe_all_zero<L>(x);
      out[i] = v ? 1u : 0u;
    }
  }
}

// BE: fe_load_be then fe_store_le; otherwise fe_load_le then fe_store_be.  Both templates compile for every class.
template <class C, bool BE>
__global__ void __launch_bounds__(WG) k_sat_io(size_t n, const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    Fe<C::L> x;
    if constexpr (BE) {
      fe_load_be<C>(x, in + i * (size_t)C::FB);
      fe_store_le<C>(out + i * (size_t)C::FB, x);
    } else {
      fe_load_le<C>(x, in + i * (size_t)C::FB);
      fe_store_be<C>(out + i * (size_t)C::FB, x);
    }
  }
}

}  // namespace eccx

namespace {
using namespace eccx;

struct Dev {
  void* p[3] = {nullptr, nullptr, nullptr};
  hipError_t e = hipSuccess;
  // device buffer k of `bytes` bytes, filled with `fill`, then from `src` (src_bytes of it, off bytes in) where src is given
  uint8_t* get(int k, size_t bytes, const void* src, size_t src_bytes, size_t off = 0, int fill = 0) {
    if (e) return nullptr;
    e = hipMalloc(&p[k], bytes ? bytes : 1);
    if (!e && bytes) e = hipMemset(p[k], fill, bytes);
    if (!e && src && src_bytes) e = hipMemcpy((uint8_t*)p[k] + off, src, src_bytes, hipMemcpyHostToDevice);
    return (uint8_t*)p[k];
  }
  void back(void* dst, int k, size_t bytes) {
    if (!e && bytes) e = hipMemcpy(dst, p[k], bytes, hipMemcpyDeviceToHost);
  }
  ~Dev() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  }
};

// a grid below the batch: every batch of more than WG rows takes several turns of the kernels' grid-stride loops
unsigned small_grid(size_t n) { return n > 3 * (size_t)WG ? 3u : 1u; }

template <class C, int OP>
int launch_op(size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if constexpr (!op_ok<C>(OP)) {
    return (int)hipErrorInvalidValue;
  } else {
    const size_t bytes = n * C::L * sizeof(uint32_t);
    if (!a || !out || (op_binary(OP) && !b)) return (int)hipErrorInvalidValue;
    Dev d;
    const uint32_t* da = (const uint32_t*)d.get(0, bytes, a, bytes);
    const uint32_t* db = op_binary(OP) ? (const uint32_t*)d.get(1, bytes, b, bytes) : nullptr;
    uint32_t* dout = (uint32_t*)d.get(2, bytes, nullptr, 0, 0, 0xA5);
    if (d.e) return (int)d.e;
    hipLaunchKernelGGL((k_sat_op<C, OP>), dim3(small_grid(n)), dim3(WG), 0, 0, n, da, db, dout);
    d.e = hipGetLastError();
    d.back(out, 2, bytes);
    return (int)d.e;
  }
}

template <class C>
int op_(int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  switch (op) {
#define SATCHECK_OP(o) case o: return launch_op<C, o>(n, a, b, out);
    SATCHECK_OP(OP_ADD) SATCHECK_OP(OP_SUB) SATCHECK_OP(OP_NEG) SATCHECK_OP(OP_MUL) SATCHECK_OP(OP_SQR)
    SATCHECK_OP(OP_TO_MONT) SATCHECK_OP(OP_FROM_MONT) SATCHECK_OP(OP_INV) SATCHECK_OP(OP_MUL_K_R2)
    SATCHECK_OP(OP_MUL_K_ONE) SATCHECK_OP(OP_MUL_K_B) SATCHECK_OP(OP_MUL_K_B3) SATCHECK_OP(OP_MUL_K_D2)
#undef SATCHECK_OP
    default: return (int)hipErrorInvalidValue;
  }
}

template <class C, int OP>
int launch_pred(size_t n, const uint32_t* a, const uint32_t* b, uint8_t* out) {
  const size_t bytes = n * C::L * sizeof(uint32_t);
  const size_t out_bytes = pred_wide(OP) ? bytes : n;
  if (!a || !out || (pred_binary(OP) && !b)) return (int)hipErrorInvalidValue;
  Dev d;
  const uint32_t* da = (const uint32_t*)d.get(0, bytes, a, bytes);
  const uint32_t* db = pred_binary(OP) ? (const uint32_t*)d.get(1, bytes, b, bytes) : nullptr;
  uint8_t* dout = d.get(2, out_bytes, nullptr, 0, 0, 0xA5);
  if (d.e) return (int)d.e;
  hipLaunchKernelGGL((k_sat_pred<C, OP>), dim3(small_grid(n)), dim3(WG), 0, 0, n, da, db, dout);
  d.e = hipGetLastError();
  d.back(out, 2, out_bytes);
  return (int)d.e;
}

template <class C>
int pred_(int op, size_t n, const uint32_t* a, const uint32_t* b, uint8_t* out) {
  switch (op) {
#define SATCHECK_PR(o) case o: return launch_pred<C, o>(n, a, b, out);
    SATCHECK_PR(PR_IS_CANONICAL) SATCHECK_PR(PR_IS_ZERO) SATCHECK_PR(PR_EQ) SATCHECK_PR(PR_SELECT_EVEN)
    SATCHECK_PR(PR_SELECT_ODD) SATCHECK_PR(PR_NEG_CANONICAL) SATCHECK_PR(PR_GREATER) SATCHECK_PR(PR_ALL_ZERO)
#undef SATCHECK_PR
    default: return (int)hipErrorInvalidValue;
  }
}

constexpr size_t IO_SLACK = 64;    // the output buffer is n FB + IO_SLACK bytes
constexpr int IO_MAX_OFF = 32;     // so at least 32 bytes of fill follow the last record

template <class C>
int io_(int be, size_t n, int in_off, int out_off, const uint8_t* in, uint8_t* out) {
  const size_t bytes = n * (size_t)C::FB;
  if (!in || !out || in_off < 0 || in_off > IO_MAX_OFF || out_off < 0 || out_off > IO_MAX_OFF) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* din = d.get(0, bytes + (size_t)in_off, in, bytes, (size_t)in_off);
  uint8_t* dout = d.get(2, bytes + IO_SLACK, nullptr, 0, 0, 0xA5);
  if (d.e) return (int)d.e;
  if (be) hipLaunchKernelGGL((k_sat_io<C, true>), dim3(small_grid(n)), dim3(WG), 0, 0, n, din + in_off, dout + out_off);
  else hipLaunchKernelGGL((k_sat_io<C, false>), dim3(small_grid(n)), dim3(WG), 0, 0, n, din + in_off, dout + out_off);
  d.e = hipGetLastError();
  d.back(out, 2, bytes + IO_SLACK);
  return (int)d.e;
}

// class indices of tests/sat_ref.py (the order of the field classes in curve_consts.inc)
#define SATCHECK_DISPATCH(cls, fn, ...)          \
  switch (cls) {                                 \
    case 0: return fn<P256>(__VA_ARGS__);        \
    case 1: return fn<P384>(__VA_ARGS__);        \
    case 2: return fn<P521>(__VA_ARGS__);        \
    case 3: return fn<BLS12_381>(__VA_ARGS__);   \
    case 4: return fn<ED25519>(__VA_ARGS__);     \
    case 5: return fn<P256K1>(__VA_ARGS__);      \
    case 6: return fn<CURVE448>(__VA_ARGS__);    \
    case 7: return fn<JUBJUB>(__VA_ARGS__);      \
    default: return (int)hipErrorInvalidValue;   \
  }
}  // namespace

// a, b (binary ops only), out: n x L little-endian uint32 words, no byte I/O on this path.  Returns the HIP error code;
// hipErrorInvalidValue for an op the class does not have (a constant it does not own, CURVE448's products).
extern "C" int satcheck_op(int cls, int op, size_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (n == 0) return 0;
  SATCHECK_DISPATCH(cls, op_, op, n, a, b, out);
}

// a, b as for satcheck_op; out_bytes: n bytes (0 or 1), or n x 4 L bytes for the selects and fe_neg_canonical
extern "C" int satcheck_pred(int cls, int op, size_t n, const uint32_t* a, const uint32_t* b, uint8_t* out_bytes) {
  if (n == 0) return 0;
  SATCHECK_DISPATCH(cls, pred_, op, n, a, b, out_bytes);
}

// in: n x FB bytes, placed in_off bytes into a hipMalloc'ed buffer; out: the whole output buffer, n FB + 64 bytes,
// pre-filled with 0xA5, the records written from out_off on.  be != 0: fe_load_be then fe_store_le, else the reverse.
extern "C" int satcheck_io(int cls, int be, size_t n, int in_off, int out_off, const uint8_t* in, uint8_t* out) {
  if (n == 0) return 0;
  SATCHECK_DISPATCH(cls, io_, be, n, in_off, out_off, in, out);
}
