// Test-only library: ECDSA verification's two kernels (eccoxide_amd/csrc/kernels_ecdsa.hpp: k_ecdsa_prepare and
// k_ecdsa_finish, launched unchanged for the four group-order structs) and the single operations they are made of
// (inv_gcd.hpp's inversion, fe.hpp's general Montgomery product modulo n), over whole batches, so that
// tests/test_ecdsa_primitives.py can compare u1, u2, the pre-verdicts and the verdicts with Python integers.  Not part
// of the product; built by __graft_entry__.build() into tests/hip_ecdsa/libecdsacheck.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_ecdsa.hpp"

namespace eccx {

// out[i] = a[i]^-1 mod n (plain in, plain out; 0 gives 0), SB-byte big-endian records
template <class O>
__global__ void __launch_bounds__(WG) k_ord_inv_check(size_t n, const uint8_t* __restrict__ a, uint8_t* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    Fe<O::L> x, r;
    fe_load_be<O>(x, a + i * (size_t)O::SB);
    fe_inv_gcd<O>(r, x);
    fe_store_be<O>(out + i * (size_t)O::SB, r);
  }
}

// out[i] = a[i] b[i] R^-1 mod n (to_mont == false), or a[i] R mod n by the product with the constant R^2 (b unread)
template <class O>
__global__ void __launch_bounds__(WG) k_ord_mul_check(size_t n, bool to_mont, const uint8_t* __restrict__ a,
                                                      const uint8_t* __restrict__ b, uint8_t* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    Fe<O::L> x, y, r;
    fe_load_be<O>(x, a + i * (size_t)O::SB);
    if (to_mont) {
      fe_mul_k<O>(r, x, O::R2);
    } else {
      fe_load_be<O>(y, b + i * (size_t)O::SB);
      fe_mul<O>(r, x, y);
    }
    fe_store_be<O>(out + i * (size_t)O::SB, r);
  }
}

}  // namespace eccx

namespace {
using namespace eccx;

struct Dev {
  void* p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipError_t e = hipSuccess;
  // device buffer k of `bytes` bytes, filled from `src` (or with `fill` where src is null)
  uint8_t* get(int k, size_t bytes, const void* src, int fill = 0) {
    if (e) return nullptr;
    e = hipMalloc(&p[k], bytes ? bytes : 1);
    if (!e && bytes) e = src ? hipMemcpy(p[k], src, bytes, hipMemcpyHostToDevice) : hipMemset(p[k], fill, bytes);
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

// a grid below the batch: every batch of more than WG lanes takes several turns of the kernels' grid-stride loops
unsigned small_grid(size_t n) { return n > 3 * (size_t)WG ? 3u : 1u; }

enum { OP_INV = 0, OP_MUL = 1, OP_TO_MONT = 2 };

template <class O>
int prepare_(size_t n, const uint8_t* digests, int digest_bytes, const uint8_t* sigs, const uint8_t* key_flags, int alias,
             uint8_t* u1_out, uint8_t* u2_out, uint8_t* verdicts_out) {
  constexpr size_t SB = O::SB;
  if (digest_bytes < 0 || digest_bytes > 2 * (int)SB || (alias && !key_flags)) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* dg = d.get(0, n * (digest_bytes ? (size_t)digest_bytes : SB), digests);
  const uint8_t* sg = d.get(1, n * 2 * SB, sigs);
  uint8_t* u1 = d.get(2, n * SB, nullptr, 0xA5);
  uint8_t* u2 = d.get(3, n * SB, nullptr, 0xA5);
  uint8_t* vd = d.get(4, n, alias ? key_flags : nullptr, 0xEE);
  const uint8_t* kf = alias ? vd : (key_flags ? d.get(5, n, key_flags) : nullptr);
  if (d.e) return (int)d.e;
  hipLaunchKernelGGL(k_ecdsa_prepare<O>, dim3(small_grid(n)), dim3(WG), 0, 0, n, dg, digest_bytes, sg, kf, u1, u2, vd);
  d.e = hipGetLastError();
  d.back(u1_out, 2, n * SB);
  d.back(u2_out, 3, n * SB);
  d.back(verdicts_out, 4, n);
  return (int)d.e;
}

template <class O>
int finish_(size_t n, const uint8_t* sigs, const uint8_t* xs, const uint8_t* lflags, uint8_t* verdicts) {
  constexpr size_t SB = O::SB;
  Dev d;
  const uint8_t* sg = d.get(0, n * 2 * SB, sigs);
  const uint8_t* x = d.get(1, n * SB, xs);
  const uint8_t* lf = d.get(2, n, lflags);
  uint8_t* vd = d.get(3, n, verdicts);
  if (d.e) return (int)d.e;
  hipLaunchKernelGGL(k_ecdsa_finish<O>, dim3(small_grid(n)), dim3(WG), 0, 0, n, sg, x, lf, vd);
  d.e = hipGetLastError();
  d.back(verdicts, 3, n);
  return (int)d.e;
}

template <class O>
int op_(int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  constexpr size_t SB = O::SB;
  if (op < OP_INV || op > OP_TO_MONT || (op == OP_MUL && !b)) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* da = d.get(0, n * SB, a);
  const uint8_t* db = op == OP_MUL ? d.get(1, n * SB, b) : nullptr;
  uint8_t* dout = d.get(2, n * SB, nullptr, 0xA5);
  if (d.e) return (int)d.e;
  if (op == OP_INV) hipLaunchKernelGGL(k_ord_inv_check<O>, dim3(small_grid(n)), dim3(WG), 0, 0, n, da, dout);
  else hipLaunchKernelGGL(k_ord_mul_check<O>, dim3(small_grid(n)), dim3(WG), 0, 0, n, op == OP_TO_MONT, da, db, dout);
  d.e = hipGetLastError();
  d.back(out, 2, n * SB);
  return (int)d.e;
}

// curve ids as in include/eccx.h
#define ECDSACHECK_DISPATCH(curve, fn, ...)            \
  switch (curve) {                                     \
    case 0: return fn<P256_ORD>(__VA_ARGS__);          \
    case 1: return fn<P384_ORD>(__VA_ARGS__);          \
    case 2: return fn<P521_ORD>(__VA_ARGS__);          \
    case 5: return fn<P256K1_ORD>(__VA_ARGS__);        \
    default: return (int)hipErrorInvalidValue;         \
  }
}  // namespace

// digests: n x digest_bytes (0: n x SB scalars); sigs: n x 2 SB; key_flags: null or n bytes; alias_flags != 0: the verdict
// buffer itself, pre-filled from key_flags, is passed as the kernel's key_flags (eccx_ecdsa_verify_dev under
// ECCX_PUBKEY_SEC1).  u1_out, u2_out: n x SB; verdicts_out: n pre-verdicts.  Returns the HIP error code.
extern "C" int ecdsacheck_prepare(int curve, size_t n, const uint8_t* digests, int digest_bytes, const uint8_t* sigs,
                                  const uint8_t* key_flags, int alias_flags, uint8_t* u1_out, uint8_t* u2_out,
                                  uint8_t* verdicts_out) {
  if (n == 0) return 0;
  ECDSACHECK_DISPATCH(curve, prepare_, n, digests, digest_bytes, sigs, key_flags, alias_flags, u1_out, u2_out, verdicts_out);
}

// sigs: n x 2 SB; xs: n x SB x-coordinates; lflags: n ladder flags; verdicts: n pre-verdicts in, verdicts out
extern "C" int ecdsacheck_finish(int curve, size_t n, const uint8_t* sigs, const uint8_t* xs, const uint8_t* lflags,
                                 uint8_t* verdicts_inout) {
  if (n == 0) return 0;
  ECDSACHECK_DISPATCH(curve, finish_, n, sigs, xs, lflags, verdicts_inout);
}

// op 0: out = a^-1 mod n; 1: out = a b R^-1 mod n; 2: out = a R mod n (R = 2^(32 L)); n x SB big-endian records, values < n
extern "C" int ecdsacheck_op(int curve, int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  if (n == 0) return 0;
  ECDSACHECK_DISPATCH(curve, op_, op, n, a, b, out);
}
