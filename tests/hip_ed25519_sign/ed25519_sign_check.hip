// Test-only library: the device functions of Ed25519 signing (eccoxide_amd/csrc/kernels_ed25519_sign.hpp) over whole
// batches, so that tests/test_ed25519_sign_primitives.py can compare them with hashlib and Python integers: the
// SHA-512 entry with a 32-byte prefix, the reduction of a secret 64-byte little-endian value mod l, the clamped secret
// scalar, and S = r + k a mod l.  Not part of the product; built by __graft_entry__.build() into
// tests/hip_ed25519_sign/libed25519signcheck.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_ed25519_sign.hpp"

namespace eccx {

// out[i] = SHA-512(pre[i] || msgs[offsets[i] - offsets[0] .. offsets[i + 1] - offsets[0])), pre: n x 32 bytes
__global__ void k_sha512_32_check(size_t n, const uint8_t* __restrict__ pre, const uint8_t* __restrict__ msgs,
                                  const uint64_t* __restrict__ offsets, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t p[4], h[8];
  ed_load_words_be<ED25519_ORD>(p, pre + i * 32);
  sha512_prefixed32(h, p, msgs + (offsets[i] - offsets[0]), offsets[i + 1] - offsets[i]);
  for (int j = 0; j < 8; ++j)
    for (int b = 0; b < 8; ++b) out[i * 64 + 8 * j + b] = (uint8_t)(h[j] >> (56 - 8 * b));
}

__device__ __forceinline__ void load_digest(uint64_t (&h)[8], const uint8_t* in) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {  // the digest's big-endian words
    uint64_t w = 0;
    for (int b = 0; b < 8; ++b) w = (w << 8) | in[8 * j + b];
    h[j] = w;
  }
}

// out[i] = (64 bytes at in + 64 i, little-endian) mod l, 32 bytes little-endian
__global__ void k_reduce_wide_ct_check(size_t n, const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t h[8];
  load_digest(h, in + i * 64);
  Fe<8> r;
  ord_from_wide_le_ct<ED25519_ORD>(r, h);
  fe_store_le<ED25519_ORD>(out + i * 32, r);
}

// out[i] = clamp(first 32 of the 64 bytes at in + 64 i) mod l, 32 bytes little-endian
__global__ void k_secret_scalar_check(size_t n, const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t h[8];
  load_digest(h, in + i * 64);
  Fe<8> a;
  ed_secret_scalar_ct<ED25519_ORD>(a, h);
  fe_store_le<ED25519_ORD>(out + i * 32, a);
}

// out[i] = r[i] + k[i] a[i] mod l; all n x 32 little-endian, inputs below l
__global__ void k_muladd_check(size_t n, const uint8_t* __restrict__ r, const uint8_t* __restrict__ k, const uint8_t* __restrict__ a,
                               uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fe<8> fr, fk, fa, s;
  fe_load_le<ED25519_ORD>(fr, r + i * 32);
  fe_load_le<ED25519_ORD>(fk, k + i * 32);
  fe_load_le<ED25519_ORD>(fa, a + i * 32);
  ord_muladd_ct<ED25519_ORD>(s, fr, fk, fa);
  fe_store_le<ED25519_ORD>(out + i * 32, s);
}

}  // namespace eccx

namespace {
struct Dev {
  void* p[4] = {nullptr, nullptr, nullptr, nullptr};
  ~Dev() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  }
};
unsigned blocks(size_t n) { return (unsigned)((n + 127) / 128); }
}  // namespace

// lead: the messages are placed `lead` bytes into their device buffer (a hipMalloc'ed buffer is aligned), so that the
// same batch can be hashed at every misalignment of the message pointer
extern "C" int ed25519signcheck_sha512_32(size_t n, const uint8_t* pre, const uint8_t* msgs, size_t msg_bytes, const uint64_t* offsets,
                                          size_t lead, uint8_t* out) {
  Dev d;
  hipError_t e = hipMalloc(&d.p[0], n * 32);
  if (!e) e = hipMalloc(&d.p[1], msg_bytes + lead + 1);
  if (!e) e = hipMalloc(&d.p[2], (n + 1) * 8);
  if (!e) e = hipMalloc(&d.p[3], n * 64);
  if (!e) e = hipMemcpy(d.p[0], pre, n * 32, hipMemcpyHostToDevice);
  if (!e && msg_bytes) e = hipMemcpy((uint8_t*)d.p[1] + lead, msgs, msg_bytes, hipMemcpyHostToDevice);
  if (!e) e = hipMemcpy(d.p[2], offsets, (n + 1) * 8, hipMemcpyHostToDevice);
  if (e) return (int)e;
  hipLaunchKernelGGL(eccx::k_sha512_32_check, dim3(blocks(n)), dim3(128), 0, 0, n, (const uint8_t*)d.p[0],
                     (const uint8_t*)d.p[1] + lead, (const uint64_t*)d.p[2], (uint8_t*)d.p[3]);
  e = hipGetLastError();
  if (!e) e = hipMemcpy(out, d.p[3], n * 64, hipMemcpyDeviceToHost);
  return (int)e;
}

static int wide_to_32(size_t n, const uint8_t* in, uint8_t* out, bool clamp) {
  Dev d;
  hipError_t e = hipMalloc(&d.p[0], n * 64);
  if (!e) e = hipMalloc(&d.p[1], n * 32);
  if (!e) e = hipMemcpy(d.p[0], in, n * 64, hipMemcpyHostToDevice);
  if (e) return (int)e;
  if (clamp) hipLaunchKernelGGL(eccx::k_secret_scalar_check, dim3(blocks(n)), dim3(128), 0, 0, n, (const uint8_t*)d.p[0], (uint8_t*)d.p[1]);
  else hipLaunchKernelGGL(eccx::k_reduce_wide_ct_check, dim3(blocks(n)), dim3(128), 0, 0, n, (const uint8_t*)d.p[0], (uint8_t*)d.p[1]);
  e = hipGetLastError();
  if (!e) e = hipMemcpy(out, d.p[1], n * 32, hipMemcpyDeviceToHost);
  return (int)e;
}

extern "C" int ed25519signcheck_reduce_wide_ct(size_t n, const uint8_t* in, uint8_t* out) { return wide_to_32(n, in, out, false); }
extern "C" int ed25519signcheck_secret_scalar(size_t n, const uint8_t* in, uint8_t* out) { return wide_to_32(n, in, out, true); }

extern "C" int ed25519signcheck_muladd(size_t n, const uint8_t* r, const uint8_t* k, const uint8_t* a, uint8_t* out) {
  Dev d;
  hipError_t e = hipSuccess;
  const uint8_t* src[3] = {r, k, a};
  for (int j = 0; j < 4 && !e; ++j) e = hipMalloc(&d.p[j], n * 32);
  for (int j = 0; j < 3 && !e; ++j) e = hipMemcpy(d.p[j], src[j], n * 32, hipMemcpyHostToDevice);
  if (e) return (int)e;
  hipLaunchKernelGGL(eccx::k_muladd_check, dim3(blocks(n)), dim3(128), 0, 0, n, (const uint8_t*)d.p[0], (const uint8_t*)d.p[1],
                     (const uint8_t*)d.p[2], (uint8_t*)d.p[3]);
  e = hipGetLastError();
  if (!e) e = hipMemcpy(out, d.p[3], n * 32, hipMemcpyDeviceToHost);
  return (int)e;
}
