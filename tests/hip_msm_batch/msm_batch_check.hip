// Test-only library: the launch sequence of the batched multi-scalar multiplication over shared points
// (eccoxide_amd/csrc/kernels_msm_batch.hpp) at a window width of the CALLER's choosing -- the product always runs
// eccx_msm_batch_window_bits(n, m) -- on BLS12-381 G1 (g2 == 0) and G2 (g2 != 0), for tests/test_msm_batch_stages_gpu.py to
// compare with the Python model at every width and for tools/bench_msm_batch.py to sweep the widths:
//   msmbcheck_bytes   the workspace of one (n, m, c)
//   msmbcheck_dev     the whole schedule and the curve's normalisation on DEVICE buffers and a stream, without synchronising
//   msmbcheck_host    the same on host buffers (it allocates, copies and synchronises)
//   msmbcheck_host_cus  msmbcheck_host with the grid caps of a card of the caller's compute-unit count
// Not part of the product; built by __graft_entry__.build().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_msm_batch.hpp"
#include "msm_policy_g2.hpp"

namespace eccx {
using CU = BLS12_381U;
using G1P = MsmWeierstrassA0<CU>;
using G2P = MsmG2<CU, BLS12_381_G2>;

// the limit rule of the product (launch.hpp), restated: this library includes no launch interface
bool fits(size_t n, size_t m, int c) {
  if (n == 0 || m == 0 || c < MSM_MIN_BITS || c > MSM_MAX_BITS) return false;
  if (m > MSM_MAX_N || n > MSM_MAX_N / m) return false;
  const uint64_t W = (uint64_t)msm_windows(c), B = msm_buckets(c), lim = 0xFFFFF000ull;
  return W * m * n <= lim && W * B * m <= lim;
}

hipError_t run(int g2, hipStream_t s, int cus, size_t n, size_t m, int c, const uint8_t* k, const uint8_t* p, const uint8_t* inf,
               uint8_t* ws, uint8_t* out, uint8_t* flags) {
  uint32_t* rows = nullptr;
  const int grid = (int)((m + WG - 1) / WG);
  if (g2) {
    const hipError_t e = msmb_launch<G2P>(s, cus, n, m, c, k, p, inf, ws, &rows, flags, false);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_g2_to_affine<CU>, dim3(grid), dim3(WG), 0, s, m, rows, out, flags);
  } else {
    const hipError_t e = msmb_launch<G1P>(s, cus, n, m, c, k, p, inf, ws, &rows, flags, false);
    if (e != hipSuccess) return e;
    constexpr int UN = 8;
    const int g = (int)((m + (size_t)WG * UN - 1) / ((size_t)WG * UN));
    hipLaunchKernelGGL((k_batch_to_affine_unsat<CU, NORM_HOMOGENEOUS, UN>), dim3(g), dim3(WG), 0, s, m, rows, out, flags);
  }
  return hipGetLastError();
}

int cus_of_device() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  return cus;
}
}  // namespace eccx

// Functions that launch return a hipError_t, or -1 for a bad argument.

extern "C" int msmbcheck_windows(int c) { return eccx::msm_windows(c); }

extern "C" size_t msmbcheck_bytes(int g2, size_t n, size_t m, int c) {
  using namespace eccx;
  if (!fits(n, m, c)) return 0;
  return g2 ? msmb_layout<G2P>(n, m, c).bytes : msmb_layout<G1P>(n, m, c).bytes;
}

// d_scalars: m x n x 32; d_points: n records (96 / 192 bytes); d_inf: null or n; d_ws: msmbcheck_bytes(g2, n, m, c) bytes,
// 256-byte aligned; d_out: m records; d_flags: m bytes
extern "C" int msmbcheck_dev(int g2, size_t n, size_t m, int c, const void* d_scalars, const void* d_points, const void* d_inf, void* d_ws,
                             void* d_out, void* d_flags, void* stream) {
  using namespace eccx;
  if (!fits(n, m, c) || !d_scalars || !d_points || !d_ws || !d_out || !d_flags) return -1;
  const int cus = cus_of_device();
  if (cus <= 0) return -1;
  return (int)run(g2, static_cast<hipStream_t>(stream), cus, n, m, c, static_cast<const uint8_t*>(d_scalars),
                  static_cast<const uint8_t*>(d_points), static_cast<const uint8_t*>(d_inf), static_cast<uint8_t*>(d_ws),
                  static_cast<uint8_t*>(d_out), static_cast<uint8_t*>(d_flags));
}

// msmbcheck_host_cus: the grids capped as on a card of `cus` compute units (cus = 1: the prepare passes run 8 workgroups,
// 2048 lanes, and Horner 8 workgroups of 64 lanes), so that small batches walk the grid-stride loops more than once
extern "C" int msmbcheck_host_cus(int g2, int cus, size_t n, size_t m, int c, const uint8_t* scalars, const uint8_t* points, uint8_t* out,
                                  uint8_t* flags) {
  using namespace eccx;
  if (!fits(n, m, c) || !scalars || !points || !out || !flags) return -1;
  if (cus <= 0) return -1;
  const size_t pb = g2 ? G2P::POINT_BYTES : G1P::POINT_BYTES, bytes = msmbcheck_bytes(g2, n, m, c);
  uint8_t *d_k = nullptr, *d_p = nullptr, *d_ws = nullptr, *d_o = nullptr, *d_f = nullptr;
  hipError_t e = hipMalloc(&d_k, m * n * 32);
  if (e == hipSuccess) e = hipMalloc(&d_p, n * pb);
  if (e == hipSuccess) e = hipMalloc(&d_ws, bytes);
  if (e == hipSuccess) e = hipMalloc(&d_o, m * pb);
  if (e == hipSuccess) e = hipMalloc(&d_f, m);
  if (e == hipSuccess) e = hipMemcpy(d_k, scalars, m * n * 32, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_p, points, n * pb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_ws, 0xA5, bytes);  // junk wherever the schedule does not write first
  if (e == hipSuccess) e = run(g2, nullptr, cus, n, m, c, d_k, d_p, nullptr, d_ws, d_o, d_f);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_o, m * pb, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(flags, d_f, m, hipMemcpyDeviceToHost);
  for (void* q : {(void*)d_k, (void*)d_p, (void*)d_ws, (void*)d_o, (void*)d_f}) (void)hipFree(q);
  return (int)e;
}

extern "C" int msmbcheck_host(int g2, size_t n, size_t m, int c, const uint8_t* scalars, const uint8_t* points, uint8_t* out, uint8_t* flags) {
  return msmbcheck_host_cus(g2, eccx::cus_of_device(), n, m, c, scalars, points, out, flags);
}
