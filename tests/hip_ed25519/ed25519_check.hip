// Test-only library: the device functions of Ed25519 verification (eccoxide_amd/csrc/sha512.hpp, and the reduction of
// a 64-byte little-endian value mod l in kernels_ed25519_verify.hpp) over whole batches, so that
// tests/test_ed25519_primitives.py can compare them with hashlib and Python integers.  Not part of the product; built
// by __graft_entry__.build() into tests/hip_ed25519/libed25519check.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_ed25519_verify.hpp"

namespace eccx {

// out[i] = SHA-512(pre[i] || msgs[offsets[i] - offsets[0] .. offsets[i + 1] - offsets[0])), pre: n x 64 bytes
__global__ void k_sha512_check(size_t n, const uint8_t* __restrict__ pre, const uint8_t* __restrict__ msgs,
                               const uint64_t* __restrict__ offsets, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t p[8], h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    uint64_t w = 0;
    for (int b = 0; b < 8; ++b) w = (w << 8) | pre[i * 64 + 8 * j + b];
    p[j] = w;
  }
  sha512_prefixed(h, p, msgs + (offsets[i] - offsets[0]), offsets[i + 1] - offsets[i]);
  for (int j = 0; j < 8; ++j)
    for (int b = 0; b < 8; ++b) out[i * 64 + 8 * j + b] = (uint8_t)(h[j] >> (56 - 8 * b));
}

// out[i] = (64 bytes at in + 64 i, little-endian) mod l, 32 bytes little-endian
__global__ void k_reduce_wide_check(size_t n, const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {  // the digest's big-endian words
    uint64_t w = 0;
    for (int b = 0; b < 8; ++b) w = (w << 8) | in[i * 64 + 8 * j + b];
    h[j] = w;
  }
  Fe<8> r;
  ord_from_wide_le<ED25519_ORD>(r, h);
  fe_store_le<ED25519_ORD>(out + i * 32, r);
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
}  // namespace

extern "C" int ed25519check_sha512(size_t n, const uint8_t* pre, const uint8_t* msgs, size_t msg_bytes, const uint64_t* offsets,
                                   uint8_t* out) {
  Dev d;
  hipError_t e = hipMalloc(&d.p[0], n * 64);
  if (!e) e = hipMalloc(&d.p[1], msg_bytes ? msg_bytes : 1);
  if (!e) e = hipMalloc(&d.p[2], (n + 1) * 8);
  if (!e) e = hipMalloc(&d.p[3], n * 64);
  if (!e) e = hipMemcpy(d.p[0], pre, n * 64, hipMemcpyHostToDevice);
  if (!e && msg_bytes) e = hipMemcpy(d.p[1], msgs, msg_bytes, hipMemcpyHostToDevice);
  if (!e) e = hipMemcpy(d.p[2], offsets, (n + 1) * 8, hipMemcpyHostToDevice);
  if (e) return (int)e;
  hipLaunchKernelGGL(eccx::k_sha512_check, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, 0, n, (const uint8_t*)d.p[0],
                     (const uint8_t*)d.p[1], (const uint64_t*)d.p[2], (uint8_t*)d.p[3]);
  e = hipGetLastError();
  if (!e) e = hipMemcpy(out, d.p[3], n * 64, hipMemcpyDeviceToHost);
  return (int)e;
}

extern "C" int ed25519check_reduce_wide(size_t n, const uint8_t* in, uint8_t* out) {
  Dev d;
  hipError_t e = hipMalloc(&d.p[0], n * 64);
  if (!e) e = hipMalloc(&d.p[1], n * 32);
  if (!e) e = hipMemcpy(d.p[0], in, n * 64, hipMemcpyHostToDevice);
  if (e) return (int)e;
  hipLaunchKernelGGL(eccx::k_reduce_wide_check, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, 0, n, (const uint8_t*)d.p[0],
                     (uint8_t*)d.p[1]);
  e = hipGetLastError();
  if (!e) e = hipMemcpy(out, d.p[1], n * 32, hipMemcpyDeviceToHost);
  return (int)e;
}
