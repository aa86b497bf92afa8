// Test-only library: the device functions of hashing to BLS12-381 G2 (eccoxide_amd/csrc/kernels_h2c_g2.hpp) over whole
// batches, each in a small kernel launched with at most two workgroups so that the stride loops run, for
// tests/test_h2c_g2_primitives.py to compare with the Python model.  The product's kernels run through the slots of
// ops_BLS12_381_G2().  Not part of the product; built by __graft_entry__.build() into tests/hip_h2c_g2/libh2cg2check.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels_h2c_g2.hpp"
#include "launch.hpp"

namespace eccx {
using CU = BLS12_381U;
using CS = BLS12_381;
using HC = BLS12_381_G2_H2C;
constexpr int FB2 = 2 * CS::FB;  // an Fp2 element: c1 || c0

ECCX_DEV F2<CU> load_f2(const uint8_t* p) {
  Fe<CS::L> c0, c1;
  (void)f2_load_be<CS>(c0, c1, p);
  return f2_to_mont<CU>(c0, c1);
}
ECCX_DEV void store_f2(uint8_t* p, const F2<CU>& a) {
  Fe<CS::L> c0, c1;
  f2_to_canonical<CU>(c0, c1, a);
  f2_store_be<CS>(p, c0, c1);
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
    for (int j = 0; j < 8 * ELL; ++j)
      for (int b = 0; b < 4; ++b) out[i * 32 * ELL + 4 * j + b] = (uint8_t)(w[j] >> (24 - 8 * b));
  }
}

// the elements k_h2c_g2_hash_to_field parked in the rows, as bytes: out is n x count x 96
__global__ void __launch_bounds__(WG) k_unpark_check(size_t n, int count, const uint32_t* __restrict__ rows, uint8_t* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    F2<CU> u0, u1;
    h2c_g2_load_u<CU>(u0, u1, rows + i * (size_t)G2_PT_WORDS);
    store_f2(out + i * (size_t)count * FB2, u0);
    if (count == 2) store_f2(out + i * 2 * FB2 + FB2, u1);
  }
}
// ... and the rows k_h2c_g2_map takes, from given field elements: u is n x count x 96
__global__ void __launch_bounds__(WG) k_park_check(size_t n, int count, const uint8_t* __restrict__ u, uint32_t* __restrict__ rows,
                                                   uint8_t* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const F2<CU> u0 = load_f2(u + i * (size_t)count * FB2);
    const F2<CU> u1 = count == 2 ? load_f2(u + i * 2 * FB2 + FB2) : u0;
    const UT<CU> e[4] = {u0.c0, u0.c1, u1.c0, u1.c1};
    h2c_g2_store_u<CU>(rows + i * (size_t)G2_PT_WORDS, e);
    flags[i] = 0;
  }
}

__global__ void __launch_bounds__(WG) k_sgn0_check(size_t n, const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG)
    out[i] = (uint8_t)h2c_g2_sgn0<CU>(load_f2(in + i * FB2));
}

// (verdict[i], y[i]) = sqrt_ratio(u[i], v[i])
__global__ void __launch_bounds__(WG, 1) k_sqrt_ratio_check(size_t n, const uint8_t* __restrict__ u, const uint8_t* __restrict__ v,
                                                            uint8_t* __restrict__ y, uint8_t* __restrict__ verdict) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    F2<CU> r;
    const bool qr = h2c_g2_sqrt_ratio<CU, HC>(r, load_f2(u + i * FB2), load_f2(v + i * FB2));
    store_f2(y + i * FB2, r);
    verdict[i] = qr ? 1 : 0;
  }
}

// rows[i] = the isogeny on (xn[i] / xd[i], y[i])
__global__ void __launch_bounds__(WG, 1) k_iso_check(size_t n, const uint8_t* __restrict__ xn, const uint8_t* __restrict__ xd,
                                                     const uint8_t* __restrict__ y, uint32_t* __restrict__ rows, uint8_t* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    G2Pt<CU> q;
    h2c_g2_iso<CU, HC>(q, load_f2(xn + i * FB2), load_f2(xd + i * FB2), load_f2(y + i * FB2));
    g2_row_store<CU>(rows + i * (size_t)G2_PT_WORDS, q);
    flags[i] = 0;
  }
}

// rows[i] = the affine point pts[i], or infinity where inf[i] == 1
__global__ void __launch_bounds__(WG) k_rows_of_points(size_t n, const uint8_t* __restrict__ pts, const uint8_t* __restrict__ inf,
                                                       uint32_t* __restrict__ rows, uint8_t* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    G2Aff<CU> a;
    (void)g2_load_affine<CU>(a, pts + i * 2 * FB2);
    G2Pt<CU> q;
    q.x = a.x; q.y = a.y; q.z = f2_one<CU>();
    if (inf[i] == 1) g2_set_infinity<CU>(q);
    g2_row_store<CU>(rows + i * (size_t)G2_PT_WORDS, q);
    flags[i] = 0;
  }
}
}  // namespace eccx

namespace {
using namespace eccx;
struct Dev {
  void* p[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
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
constexpr size_t ROW_BYTES = (size_t)G2_PT_WORDS * 4;
#define TRY(call)                         \
  do {                                    \
    hipError_t e_ = (call);               \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

// rows -> x || y and flags through the product's normalisation
int normalise(Dev& d, int rows, int out, int flags, size_t n, uint8_t* h_out, uint8_t* h_flags) {
  TRY(ops_BLS12_381_G2().to_affine_var(1, nullptr, n, (const uint32_t*)d.p[rows], (uint8_t*)d.p[out], (uint8_t*)d.p[flags]));
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(h_out, d.p[out], n * 2 * FB2, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(h_flags, d.p[flags], n, hipMemcpyDeviceToHost));
  return 0;
}
}  // namespace

// ell in {4, 8}: 32 ell bytes per message
extern "C" int h2cg2check_expand(int ell, size_t n, const uint8_t* msgs, size_t msg_bytes, const uint64_t* offsets, const uint8_t* dst,
                                 size_t dst_len, uint8_t* out) {
  if (ell != 4 && ell != 8) return -1;
  H2cTag tag;
  h2c_host::pack_tag(tag, dst, dst_len, 32u * (uint32_t)ell);
  Dev d;
  TRY(d.up(0, msgs, msg_bytes));
  TRY(d.up(1, offsets, (n + 1) * 8));
  TRY(d.room(2, n * 32 * (size_t)ell));
  const uint8_t* m = (const uint8_t*)d.p[0];
  const uint64_t* o = (const uint64_t*)d.p[1];
  uint8_t* r = (uint8_t*)d.p[2];
  if (ell == 4) hipLaunchKernelGGL(k_expand_check<4>, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, m, o, tag, r);
  if (ell == 8) hipLaunchKernelGGL(k_expand_check<8>, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, m, o, tag, r);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(out, d.p[2], n * 32 * (size_t)ell, hipMemcpyDeviceToHost));
  return 0;
}

// the product's hash_to_field kernel: out is n x count x 96 (each element c1 || c0), flags n
extern "C" int h2cg2check_hash_to_field(int count, size_t n, const uint8_t* msgs, size_t msg_bytes, const uint64_t* offsets,
                                        const uint8_t* dst, size_t dst_len, uint8_t* out, uint8_t* flags) {
  if (count != 1 && count != 2) return -1;
  H2cTag tag;
  h2c_host::pack_tag(tag, dst, dst_len, 128u * (uint32_t)count);
  Dev d;
  TRY(d.up(0, msgs, msg_bytes));
  TRY(d.up(1, offsets, (n + 1) * 8));
  TRY(d.room(2, n * ROW_BYTES));
  TRY(d.room(3, n * (size_t)count * FB2));
  TRY(d.room(4, n));
  TRY(ops_BLS12_381_G2().h2c_hash_to_field(grid_of(n), nullptr, n, (const uint8_t*)d.p[0], (const uint64_t*)d.p[1], tag, count,
                                           (uint32_t*)d.p[2], (uint8_t*)d.p[4]));
  hipLaunchKernelGGL(k_unpark_check, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, count, (const uint32_t*)d.p[2], (uint8_t*)d.p[3]);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(out, d.p[3], n * (size_t)count * FB2, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(flags, d.p[4], n, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int h2cg2check_sgn0(size_t n, const uint8_t* in, uint8_t* out) {
  Dev d;
  TRY(d.up(0, in, n * FB2));
  TRY(d.room(1, n));
  hipLaunchKernelGGL(k_sgn0_check, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, (const uint8_t*)d.p[0], (uint8_t*)d.p[1]);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(out, d.p[1], n, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int h2cg2check_sqrt_ratio(size_t n, const uint8_t* u, const uint8_t* v, uint8_t* y, uint8_t* verdict) {
  Dev d;
  TRY(d.up(0, u, n * FB2));
  TRY(d.up(1, v, n * FB2));
  TRY(d.room(2, n * FB2));
  TRY(d.room(3, n));
  hipLaunchKernelGGL(k_sqrt_ratio_check, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, (const uint8_t*)d.p[0], (const uint8_t*)d.p[1],
                     (uint8_t*)d.p[2], (uint8_t*)d.p[3]);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(y, d.p[2], n * FB2, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(verdict, d.p[3], n, hipMemcpyDeviceToHost));
  return 0;
}

// xn, xd, y: n x 96 each -> the isogeny's image of (xn / xd, y), x || y and flags
extern "C" int h2cg2check_iso(size_t n, const uint8_t* xn, const uint8_t* xd, const uint8_t* y, uint8_t* out, uint8_t* flags) {
  Dev d;
  TRY(d.up(0, xn, n * FB2));
  TRY(d.up(1, xd, n * FB2));
  TRY(d.up(2, y, n * FB2));
  TRY(d.room(3, n * ROW_BYTES));
  TRY(d.room(4, n * 2 * FB2));
  TRY(d.room(5, n));
  hipLaunchKernelGGL(k_iso_check, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, (const uint8_t*)d.p[0], (const uint8_t*)d.p[1],
                     (const uint8_t*)d.p[2], (uint32_t*)d.p[3], (uint8_t*)d.p[5]);
  TRY(hipGetLastError());
  return normalise(d, 3, 4, 5, n, out, flags);
}

// u: n x count x 96 -> the product's map kernel from given field elements (count = 1: the mapped point itself, count = 2:
// Q0 + Q1), and with clear != 0 its cofactor kernel behind it; x || y and flags
extern "C" int h2cg2check_map(int count, int clear, size_t n, const uint8_t* u, uint8_t* out, uint8_t* flags) {
  if (count != 1 && count != 2) return -1;
  const CurveOps& ops = ops_BLS12_381_G2();
  Dev d;
  TRY(d.up(0, u, n * (size_t)count * FB2));
  TRY(d.room(1, 2 * n * ROW_BYTES));
  TRY(d.room(2, n * 2 * FB2));
  TRY(d.room(3, n));
  uint32_t* rows = (uint32_t*)d.p[1];
  hipLaunchKernelGGL(k_park_check, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, count, (const uint8_t*)d.p[0], rows, (uint8_t*)d.p[3]);
  TRY(hipGetLastError());
  TRY(ops.h2c_map_finish(grid_of(n), nullptr, n, count, rows));
  if (clear) TRY(ops.h2c_clear(grid_of(n), nullptr, n, rows));
  return normalise(d, 1, 2, 3, n, out, flags);
}

// pts: n x 192 affine with inf flags (1: the identity) -> the product's cofactor kernel; x || y and flags
extern "C" int h2cg2check_clear(size_t n, const uint8_t* pts, const uint8_t* inf, uint8_t* out, uint8_t* flags) {
  const CurveOps& ops = ops_BLS12_381_G2();
  Dev d;
  TRY(d.up(0, pts, n * 2 * FB2));
  TRY(d.up(1, inf, n));
  TRY(d.room(2, 2 * n * ROW_BYTES));
  TRY(d.room(3, n * 2 * FB2));
  TRY(d.room(4, n));
  uint32_t* rows = (uint32_t*)d.p[2];
  hipLaunchKernelGGL(k_rows_of_points, dim3(grid_of(n)), dim3(WG), 0, nullptr, n, (const uint8_t*)d.p[0], (const uint8_t*)d.p[1], rows,
                     (uint8_t*)d.p[4]);
  TRY(hipGetLastError());
  TRY(ops.h2c_clear(grid_of(n), nullptr, n, rows));
  return normalise(d, 2, 3, 4, n, out, flags);
}

// One launch of the product's pipeline on DEVICE buffers, enqueued on `stream` without synchronising, with the grids the
// C ABI gives it (tools/bench_h2c_g2.py times each on its own): stage 0 hash_to_field (hash_to_curve: two elements),
// 1 the maps and the addition, 2 the cofactor chain, 3 the normalisation.  d_rows: 2 n rows.
extern "C" int h2cg2check_stage(int stage, size_t n, const void* d_msgs, const void* d_offsets, const uint8_t* dst, size_t dst_len,
                                void* d_rows, void* d_out, void* d_flags, void* stream) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    TRY(hipGetDevice(&dev));
    TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  }
  const CurveOps& ops = ops_BLS12_381_G2();
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t* rows = static_cast<uint32_t*>(d_rows);
  uint8_t* flags = static_cast<uint8_t*>(d_flags);
  auto capped = [](size_t units, size_t cap) { return (int)std::max<size_t>(1, std::min((units + WG - 1) / WG, cap)); };
  if (stage == 0) {
    H2cTag tag;
    h2c_host::pack_tag(tag, dst, dst_len, 256);
    TRY(ops.h2c_hash_to_field(capped(n, (size_t)cus * 8), s, n, static_cast<const uint8_t*>(d_msgs), static_cast<const uint64_t*>(d_offsets),
                              tag, 2, rows, flags));
  } else if (stage == 1) {
    TRY(ops.h2c_map_finish(ops.h2c_map_grid(cus, n), s, n, 2, rows));
  } else if (stage == 2) {
    TRY(ops.h2c_clear(ops.h2c_clear_grid(cus, n), s, n, rows));
  } else if (stage == 3) {
    TRY(ops.to_affine_var(capped((n + 7) / 8, (size_t)cus * 4), s, n, rows, static_cast<uint8_t*>(d_out), flags));
  } else {
    return -1;
  }
  return 0;
}
