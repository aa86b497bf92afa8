// Test-only library: ECDSA signing's finishing kernel (eccoxide_amd/csrc/kernels_ecdsa_sign.hpp: k_ecdsa_sign_finish,
// launched unchanged for the four group-order structs on x-coordinates and flags the test makes up) and the secret-data
// helpers it is made of (the range test, ord_add_ct, ord_cond_sub_ct, ord_select_ct), over whole batches, so that
// tests/test_ecdsa_sign_primitives.py can compare them with Python integers.  The helpers take whole 4 L-byte
// big-endian words, so that values up to 2^(32 L) - 1 reach them.  Not part of the product; built by
// __graft_entry__.build() into tests/hip_ecdsa_sign/libecdsasigncheck.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_ecdsa_sign.hpp"

namespace eccx {

// 4 L big-endian bytes <-> L words
template <int L>
__device__ __forceinline__ void load_full(Fe<L>& r, const uint8_t* in) {
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const uint8_t* p = in + 4 * (L - 1 - i);
    r.v[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
  }
}
template <int L>
__device__ __forceinline__ void store_full(uint8_t* out, const Fe<L>& a) {
#pragma unroll
  for (int i = 0; i < L; ++i) {
    uint8_t* p = out + 4 * (L - 1 - i);
    p[0] = (uint8_t)(a.v[i] >> 24); p[1] = (uint8_t)(a.v[i] >> 16); p[2] = (uint8_t)(a.v[i] >> 8); p[3] = (uint8_t)a.v[i];
  }
}

enum { OP_RANGE = 0, OP_ADD = 1, OP_COND_SUB = 2, OP_SELECT = 3 };

// a, b: n x 4 L bytes; c: n bytes (the carry of OP_COND_SUB, the choice of OP_SELECT); out: n x 4 L bytes, or n bytes for
// OP_RANGE
template <class O, int OP>
__global__ void __launch_bounds__(WG) k_ord_ct_check(size_t n, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                     const uint8_t* __restrict__ c, uint8_t* __restrict__ out) {
  constexpr int L = O::L;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    Fe<L> x, y, r;
    load_full<L>(x, a + i * (size_t)(4 * L));
    if constexpr (OP == OP_RANGE) {
      out[i] = ord_in_range_ct<O>(x) ? 1 : 0;
    } else {
      if constexpr (OP == OP_ADD || OP == OP_SELECT) load_full<L>(y, b + i * (size_t)(4 * L));
      if constexpr (OP == OP_ADD) ord_add_ct<O>(r, x, y);
      if constexpr (OP == OP_COND_SUB) ord_cond_sub_ct<O>(r, x.v, (uint32_t)c[i]);
      if constexpr (OP == OP_SELECT) ord_select_ct<L>(r, ct_mask(c[i] != 0), x, y);
      store_full<L>(out + i * (size_t)(4 * L), r);
    }
  }
}

}  // namespace eccx

namespace {
using namespace eccx;

struct Dev {
  void* p[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
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

template <class O>
int op_(int op, size_t n, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* out) {
  constexpr size_t W = 4 * O::L;
  if (op < OP_RANGE || op > OP_SELECT) return (int)hipErrorInvalidValue;
  if (((op == OP_ADD || op == OP_SELECT) && !b) || ((op == OP_COND_SUB || op == OP_SELECT) && !c)) return (int)hipErrorInvalidValue;
  Dev d;
  const size_t ob = op == OP_RANGE ? n : n * W;
  const uint8_t* da = d.get(0, n * W, a);
  const uint8_t* db = b ? d.get(1, n * W, b) : nullptr;
  const uint8_t* dc = c ? d.get(2, n, c) : nullptr;
  uint8_t* dout = d.get(3, ob, nullptr, 0xA5);
  if (d.e) return (int)d.e;
  const dim3 g(small_grid(n)), w(WG);
  if (op == OP_RANGE) hipLaunchKernelGGL((k_ord_ct_check<O, OP_RANGE>), g, w, 0, 0, n, da, db, dc, dout);
  else if (op == OP_ADD) hipLaunchKernelGGL((k_ord_ct_check<O, OP_ADD>), g, w, 0, 0, n, da, db, dc, dout);
  else if (op == OP_COND_SUB) hipLaunchKernelGGL((k_ord_ct_check<O, OP_COND_SUB>), g, w, 0, 0, n, da, db, dc, dout);
  else hipLaunchKernelGGL((k_ord_ct_check<O, OP_SELECT>), g, w, 0, 0, n, da, db, dc, dout);
  d.e = hipGetLastError();
  d.back(out, 3, ob);
  return (int)d.e;
}

template <class O>
int finish_(size_t n, const uint8_t* digests, int digest_bytes, const uint8_t* secrets, const uint8_t* nonces, const uint8_t* xs,
            const uint8_t* lflags, uint8_t* sigs_out, uint8_t* status_out) {
  constexpr size_t SB = O::SB;
  if (digest_bytes < 0 || digest_bytes > 2 * (int)SB) return (int)hipErrorInvalidValue;
  Dev d;
  const uint8_t* dg = d.get(0, n * (digest_bytes ? (size_t)digest_bytes : SB), digests);
  const uint8_t* ds = d.get(1, n * SB, secrets);
  const uint8_t* dk = d.get(2, n * SB, nonces);
  const uint8_t* dx = d.get(3, n * SB, xs);
  const uint8_t* df = d.get(4, n, lflags);
  uint8_t* sg = d.get(5, n * 2 * SB, nullptr, 0xA5);
  uint8_t* st = d.get(6, n, nullptr, 0xEE);
  if (d.e) return (int)d.e;
  hipLaunchKernelGGL(k_ecdsa_sign_finish<O>, dim3(small_grid(n)), dim3(WG), 0, 0, n, dg, digest_bytes, ds, dk, dx, df, sg, st);
  d.e = hipGetLastError();
  d.back(sigs_out, 5, n * 2 * SB);
  d.back(status_out, 6, n);
  return (int)d.e;
}

// curve ids as in include/eccx.h
#define ECDSASIGNCHECK_DISPATCH(curve, fn, ...)        \
  switch (curve) {                                     \
    case 0: return fn<P256_ORD>(__VA_ARGS__);          \
    case 1: return fn<P384_ORD>(__VA_ARGS__);          \
    case 2: return fn<P521_ORD>(__VA_ARGS__);          \
    case 5: return fn<P256K1_ORD>(__VA_ARGS__);        \
    default: return (int)hipErrorInvalidValue;         \
  }
}  // namespace

// Records of 4 L big-endian bytes (L = 8, 12, 17, 8 words).  op 0: out[i] = 0 < a < n (n bytes); 1: ord_add_ct(a, b);
// 2: ord_cond_sub_ct(a, carry c[i]); 3: c[i] ? a : b by ord_select_ct.  Returns the HIP error code.
extern "C" int ecdsasigncheck_op(int curve, int op, size_t n, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* out) {
  if (n == 0) return 0;
  ECDSASIGNCHECK_DISPATCH(curve, op_, op, n, a, b, c, out);
}

// k_ecdsa_sign_finish on given rows: digests n x digest_bytes (0: n x SB scalars), secrets, nonces, xs n x SB, lflags n
// bytes; sigs_out n x 2 SB, status_out n bytes
extern "C" int ecdsasigncheck_finish(int curve, size_t n, const uint8_t* digests, int digest_bytes, const uint8_t* secrets,
                                     const uint8_t* nonces, const uint8_t* xs, const uint8_t* lflags, uint8_t* sigs_out,
                                     uint8_t* status_out) {
  if (n == 0) return 0;
  ECDSASIGNCHECK_DISPATCH(curve, finish_, n, digests, digest_bytes, secrets, nonces, xs, lflags, sigs_out, status_out);
}
