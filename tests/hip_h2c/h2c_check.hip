// Test-only library: the device functions of hashing to BLS12-381 G1 (eccoxide_amd/csrc/sha256.hpp, kernels_h2c.hpp) over
// whole batches, each in a small kernel launched with at most two workgroups so that the stride loops run, for
// tests/test_h2c_primitives.py to compare with hashlib and the Python model.  Not part of the product; built by
// __graft_entry__.build() into tests/hip_h2c/libh2ccheck.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_h2c.hpp"

namespace eccx {
using CU = BLS12_381U;
using CS = BLS12_381;
using HC = BLS12_381_H2C;
constexpr int W3 = urow3_words<CU>();

ECCX_DEV void store_words_be(uint8_t* out, const uint32_t* w, int words) {
  for (int j = 0; j < words; ++j)
    for (int b = 0; b < 4; ++b) out[4 * j + b] = (uint8_t)(w[j] >> (24 - 8 * b));
}

// out[i] = SHA-256(msgs[offsets[i] - offsets[0] .. offsets[i + 1] - offsets[0]))
__global__ void __launch_bounds__(WG) k_sha256_check(size_t n, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offsets,
                                                     uint8_t* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    uint32_t h[8];
    sha256_msg(h, msgs + (offsets[i] - offsets[0]), offsets[i + 1] - offsets[i]);
    store_words_be(out + i * 32, h, 8);
  }
}

// out[i] = expand_message_xmd(msg i, tag, 32 ELL)
template <int ELL>
__global__ void __launch_bounds__(WG) k_expand_check(size_t n, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offsets,
                                                     const H2cTag tag, uint8_t* __restrict__ out) {
  __shared__ uint32_t s_tail[H2cTag::B0_WORDS];
  h2c_stage_tail(s_tail, tag);
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    uint32_t w[8 * ELL];
    expand_message_xmd<ELL>(w, msgs + (offsets[i] - offsets[0]), offsets[i + 1] - offsets[i], tag, s_tail);
    store_words_be(out + i * 32 * ELL, w, 8 * ELL);
  }
}

// out[i] = (64 big-endian bytes at in + 64 i) mod p, 48 bytes big-endian
__global__ void __launch_bounds__(WG) k_fp_from_uniform_check(size_t n, const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    uint32_t w[16];
    for (int j = 0; j < 16; ++j) {
      uint32_t x = 0;
      for (int b = 0; b < 4; ++b) x = (x << 8) | in[i * 64 + 4 * j + b];
      w[j] = x;
    }
    Fe<CS::L> c;
    u_to_canonical<CU>(c, h2c_fp_from_uniform<CU, HC>(w));
    fe_store_be<CS>(out + i * 48, c);
  }
}

ECCX_DEV UT<CU> load_element(const uint8_t* p) {
  Fe<CS::L> c;
  fe_load_be<CS>(c, p);
  return u_as<1, 3>(u_to_mont<CU>(c));
}

// rows[i] = h2c_map_to_curve_g1(u[i]), u: n x 48 bytes big-endian, canonical
__global__ void __launch_bounds__(WG, unsat_occupancy<CU>()) k_map_check(size_t n, const uint8_t* __restrict__ u, uint32_t* __restrict__ rows,
                                                                       uint8_t* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    UJac<CU> q;
    h2c_map_to_curve_g1<CU, HC>(q, load_element(u + i * 48));
    u3_store<CU>(rows + i * (size_t)W3, q.x, q.y, u_reduce(q.z));
    flags[i] = 0;
  }
}

// the rows k_h2c_map_finish takes, from given field elements: u is n x COUNT x 48 bytes
template <int COUNT>
__global__ void __launch_bounds__(WG) k_park_check(size_t n, const uint8_t* __restrict__ u, uint32_t* __restrict__ rows,
                                                   uint8_t* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const UT<CU> u0 = load_element(u + i * 48 * COUNT);
    UT<CU> u1 = u0;
    if constexpr (COUNT == 2) u1 = load_element(u + i * 96 + 48);
    h2c_store_u<CU>(rows + i * (size_t)W3, u0, u1);
    flags[i] = 0;
  }
}
}  // namespace eccx

namespace {
using namespace eccx;
struct Dev {
  void* p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~Dev() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  }
  hipError_t up(int k, const void* host, size_t bytes) {
    hipError_t e = hipMalloc(&p[k], bytes ? bytes : 1);
    if (e == hipSuccess && bytes) e = hipMemcpy(p[k], host, bytes, hipMemcpyHostToDevice);
    return e;
  }
  hipError_t room(int k, size_t bytes) { return hipMalloc(&p[k], bytes ? bytes : 1); }
};
int grid_of(size_t n) { return n > (size_t)WG ? 2 : 1; }
#define TRY(call)                      \
  do {                                 \
    hipError_t e_ = (call);            \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

// rows -> x || y and flags through the product's normalisation
int normalise(Dev& d, int rows, int out, int flags, size_t n, uint8_t* h_out, uint8_t* h_flags) {
  hipLaunchKernelGGL((k_batch_to_affine_unsat<CU, NORM_JACOBIAN, 8>), dim3(1), dim3(WG), 0, nullptr, n, (const uint32_t*)d.p[rows],
                     (uint8_t*)d.p[out], (uint8_t*)d.p[flags]);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(h_out, d.p[out], n * 96, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(h_flags, d.p[flags], n, hipMemcpyDeviceToHost));
  return 0;
}
}  // namespace

extern "C" int h2ccheck_sha256(size_t n, const uint8_t* msgs, size_t msg_bytes, const uint64_t* offsets, uint8_t* out) {
  Dev d;
  TRY(d.up(0, msgs, msg_bytes));
  TRY(d.up(1, offsets, (n + 1) * 8));
  TRY(d.room(2, n * 32));
  hipLaunchKernelGGL(k_sha256_check, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, (const uint8_t*)d.p[0], (const uint64_t*)d.p[1], (uint8_t*)d.p[2]);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(out, d.p[2], n * 32, hipMemcpyDeviceToHost));
  return 0;
}

// ell in {1, 2, 4}: 32 ell bytes per message
extern "C" int h2ccheck_expand(int ell, size_t n, const uint8_t* msgs, size_t msg_bytes, const uint64_t* offsets, const uint8_t* dst,
                               size_t dst_len, uint8_t* out) {
  if (ell != 1 && ell != 2 && ell != 4) return -1;
  H2cTag tag;
  h2c_host::pack_tag(tag, dst, dst_len, 32u * (uint32_t)ell);
  Dev d;
  TRY(d.up(0, msgs, msg_bytes));
  TRY(d.up(1, offsets, (n + 1) * 8));
  TRY(d.room(2, n * 32 * (size_t)ell));
  const uint8_t* m = (const uint8_t*)d.p[0];
  const uint64_t* o = (const uint64_t*)d.p[1];
  uint8_t* r = (uint8_t*)d.p[2];
  if (ell == 1) hipLaunchKernelGGL(k_expand_check<1>, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, m, o, tag, r);
  if (ell == 2) hipLaunchKernelGGL(k_expand_check<2>, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, m, o, tag, r);
  if (ell == 4) hipLaunchKernelGGL(k_expand_check<4>, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, m, o, tag, r);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(out, d.p[2], n * 32 * (size_t)ell, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int h2ccheck_fp_from_uniform(size_t n, const uint8_t* in, uint8_t* out) {
  Dev d;
  TRY(d.up(0, in, n * 64));
  TRY(d.room(1, n * 48));
  hipLaunchKernelGGL(k_fp_from_uniform_check, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, (const uint8_t*)d.p[0], (uint8_t*)d.p[1]);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(out, d.p[1], n * 48, hipMemcpyDeviceToHost));
  return 0;
}

// u: n x 48 -> the mapped points (before the cofactor is cleared), x || y and flags
extern "C" int h2ccheck_map(size_t n, const uint8_t* u, uint8_t* out, uint8_t* flags) {
  Dev d;
  TRY(d.up(0, u, n * 48));
  TRY(d.room(1, n * (size_t)W3 * 4));
  TRY(d.room(2, n * 96));
  TRY(d.room(3, n));
  hipLaunchKernelGGL(k_map_check, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, (const uint8_t*)d.p[0], (uint32_t*)d.p[1], (uint8_t*)d.p[3]);
  TRY(hipGetLastError());
  return normalise(d, 1, 2, 3, n, out, flags);
}

// u: n x count x 48 -> the product's second kernel (both maps, h2c_g1_finish) from given field elements
extern "C" int h2ccheck_finish(int count, size_t n, const uint8_t* u, uint8_t* out, uint8_t* flags) {
  if (count != 1 && count != 2) return -1;
  Dev d;
  TRY(d.up(0, u, n * 48 * (size_t)count));
  TRY(d.room(1, n * (size_t)W3 * 4));
  TRY(d.room(2, n * 96));
  TRY(d.room(3, n));
  const uint8_t* du = (const uint8_t*)d.p[0];
  uint32_t* rows = (uint32_t*)d.p[1];
  if (count == 2) {
    hipLaunchKernelGGL(k_park_check<2>, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, du, rows, (uint8_t*)d.p[3]);
    hipLaunchKernelGGL((k_h2c_map_finish<CU, HC, BLS12_381_GLV, 2>), dim3(grid_of(n)), dim3(WG), 0, nullptr, n, rows);
  } else {
    hipLaunchKernelGGL(k_park_check<1>, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, du, rows, (uint8_t*)d.p[3]);
    hipLaunchKernelGGL((k_h2c_map_finish<CU, HC, BLS12_381_GLV, 1>), dim3(grid_of(n)), dim3(WG), 0, nullptr, n, rows);
  }
  TRY(hipGetLastError());
  return normalise(d, 1, 2, 3, n, out, flags);
}
