// Test-only library: the stages of the multi-scalar multiplication (eccoxide_amd/csrc/kernels_msm.hpp), each launched on
// inputs the test makes up, for tests/test_msm_stages_gpu.py to compare with the Python model (tests/msm_ref.py):
//   msmcheck_recode   the recoding kernel: n scalars -> n x ceil(257 / c) signed digits
//   msmcheck_segsum   the segmented sum over a grouped list (key, term | sign << 31) it is given: the converted terms come
//                     from the product's own conversion kernel; every bucket row comes back normalised
//   msmcheck_reduce   the window reduction sum_j j B_j on bucket rows it is given (affine points, present or not), one
//                     normalised point per window
//   msmcheck_msm_host the whole schedule on host buffers with the grid caps of a card of the caller's compute-unit count
// Bucket rows and window sums go through the product's batched normalisation.  Not part of the product; built by
// __graft_entry__.build().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kernels_msm.hpp"

namespace eccx {
using CU = BLS12_381U;
using G = MsmWeierstrassA0<CU>;
constexpr int RW = G::ROW_WORDS;

// bucket rows from affine records: present[i] == 0 leaves the row alone (the reduction must not read it)
__global__ void __launch_bounds__(WG) k_rows_from_affine(size_t m, const uint8_t* __restrict__ xy, const uint8_t* __restrict__ present,
                                                         uint32_t* __restrict__ scratch_entries, uint32_t* __restrict__ rows) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < m; i += (size_t)gridDim.x * WG) {
    if (!present[i]) continue;
    uint32_t* e = scratch_entries + i * (size_t)G::ENTRY_WORDS;
    G::convert(e, xy + i * (size_t)G::POINT_BYTES, false);
    G::Pt p;
    G::load_entry(p, e, false);
    G::store_row(rows + i * (size_t)RW, p);
  }
}
// the Y half of the reduction's last pairs, one row per window
__global__ void k_take_y(int windows, const uint32_t* __restrict__ pairs, uint32_t* __restrict__ rows) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= windows * RW) return;
  const int w = t / RW, j = t % RW;
  rows[t] = pairs[(2 * (size_t)w + 1) * RW + j];
}

struct Dev {
  std::vector<void*> all;
  hipError_t e = hipSuccess;
  template <class T>
  T* get(size_t bytes, const void* from = nullptr, bool zero = false) {
    void* p = nullptr;
    if (e == hipSuccess) e = hipMalloc(&p, bytes ? bytes : 1);
    if (p) all.push_back(p);
    if (e == hipSuccess && from) e = hipMemcpy(p, from, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && zero) e = hipMemset(p, 0, bytes ? bytes : 1);
    return static_cast<T*>(p);
  }
  ~Dev() {
    for (void* p : all) (void)hipFree(p);
  }
};

// rows (count x RW words, device) -> count x 96 bytes and flags (0 point, 1 infinity) on the host
hipError_t normalise(Dev& d, size_t count, const uint32_t* d_rows, uint8_t* out, uint8_t* flags) {
  uint8_t* d_out = d.get<uint8_t>(count * G::POINT_BYTES);
  uint8_t* d_fl = d.get<uint8_t>(count, nullptr, true);
  if (d.e != hipSuccess) return d.e;
  constexpr int UN = 8;
  const int grid = (int)((count + (size_t)WG * UN - 1) / ((size_t)WG * UN));
  hipLaunchKernelGGL((k_batch_to_affine_unsat<CU, NORM_HOMOGENEOUS, UN>), dim3(grid), dim3(WG), 0, nullptr, count, d_rows, d_out, d_fl);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, count * G::POINT_BYTES, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(flags, d_fl, count, hipMemcpyDeviceToHost);
  return e;
}
}  // namespace eccx

// Every function returns a hipError_t, or -1 for a bad argument.  All buffers are host buffers.

extern "C" int msmcheck_windows(int c) { return eccx::msm_windows(c); }

// digits: n x msm_windows(c) int32
extern "C" int msmcheck_recode(size_t n, int c, const uint8_t* scalars, int32_t* digits) {
  using namespace eccx;
  if (n == 0 || c < MSM_MIN_BITS || c > MSM_MAX_BITS || !scalars || !digits) return -1;
  Dev d;
  const size_t out_bytes = n * (size_t)msm_windows(c) * sizeof(int32_t);
  uint8_t* d_k = d.get<uint8_t>(n * 32, scalars);
  int32_t* d_d = d.get<int32_t>(out_bytes);
  if (d.e != hipSuccess) return (int)d.e;
  hipLaunchKernelGGL(k_msm_recode, dim3(msm_grid(n, 2)), dim3(WG), 0, nullptr, n, c, d_k, d_d);  // two workgroups: the stride loop runs
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(digits, d_d, out_bytes, hipMemcpyDeviceToHost);
  return (int)e;
}

// The grouped list of `len` entries (keys non-decreasing, each below c's windows x buckets; terms: index | sign << 31 into
// the n points) summed per key.  out: m x 96 bytes and m flags for the m = windows x buckets keys; a key without entries
// comes back as infinity (its row is never written: the rows start zeroed here).
extern "C" int msmcheck_segsum(size_t n, int c, const uint8_t* points, size_t len, const uint32_t* keys, const uint32_t* terms,
                               uint8_t* out, uint8_t* flags) {
  using namespace eccx;
  if (n == 0 || c < MSM_MIN_BITS || c > MSM_MAX_BITS || !points || !out || !flags || (len && (!keys || !terms))) return -1;
  const size_t W = (size_t)msm_windows(c), m = W * msm_buckets(c);
  if (len > W * n) return -1;  // the workspace is laid out for at most one entry per term and window
  for (size_t i = 0; i < len; ++i)
    if (keys[i] >= m || (terms[i] & 0x7fffffffu) >= n || (i && keys[i] < keys[i - 1])) return -1;
  const MsmLayout L = msm_layout<G>(n, c);
  Dev d;
  uint8_t* ws = d.get<uint8_t>(L.bytes, nullptr, true);
  uint8_t* d_pts = d.get<uint8_t>(n * G::POINT_BYTES, points);
  uint8_t* d_zero = d.get<uint8_t>(n * 32, nullptr, true);  // scalars 0: the conversion pass files nothing
  if (d.e != hipSuccess) return (int)d.e;
  auto u32 = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
  hipLaunchKernelGGL((k_msm_prepare<G, false>), dim3(msm_grid(n, 2)), dim3(WG), 0, nullptr, n, c, d_zero, d_pts, nullptr, u32(L.entries),
                     u32(L.ctr), u32(L.rejected), nullptr, nullptr, 0u);
  hipError_t e = hipGetLastError();
  const uint32_t total = (uint32_t)len;
  if (e == hipSuccess && len) e = hipMemcpy(ws + L.list_keys, keys, len * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && len) e = hipMemcpy(ws + L.list_terms, terms, len * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ws + L.total, &total, 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = msm_launch_segsum<G>(nullptr, W * n, ws, L);
  if (e == hipSuccess) e = normalise(d, m, u32(L.bucket_rows), out, flags);
  return (int)e;
}

// Bucket rows for m = windows x buckets keys from affine points (present[i] == 0: the bucket is empty and its row holds
// junk), reduced to sum_j j B_j per window.  out: windows x 96 bytes and flags.
extern "C" int msmcheck_reduce(int c, const uint8_t* bucket_points, const uint8_t* present, uint8_t* out, uint8_t* flags) {
  using namespace eccx;
  if (c < MSM_MIN_BITS || c > MSM_MAX_BITS || !bucket_points || !present || !out || !flags) return -1;
  const int W = msm_windows(c);
  const size_t m = (size_t)W * msm_buckets(c);
  const MsmLayout L = msm_layout<G>(1, c);
  Dev d;
  uint8_t* ws = d.get<uint8_t>(L.bytes);
  if (d.e == hipSuccess) d.e = hipMemset(ws, 0xA5, L.bytes);  // junk in every row that is not given
  uint8_t* d_pts = d.get<uint8_t>(m * G::POINT_BYTES, bucket_points);
  uint8_t* d_present = d.get<uint8_t>(m, present);
  uint32_t* d_scratch = d.get<uint32_t>(m * (size_t)G::ENTRY_WORDS * 4);
  uint32_t* d_rows = d.get<uint32_t>((size_t)W * RW * 4);
  if (d.e != hipSuccess) return (int)d.e;
  // the counters as the scatter leaves them: each key's END offset
  std::vector<uint32_t> ends(m);
  uint32_t run = 0;
  for (size_t i = 0; i < m; ++i) ends[i] = run += present[i] ? 1u + (uint32_t)(i % 3) : 0u;
  hipError_t e = hipMemcpy(ws + L.ctr, ends.data(), m * 4, hipMemcpyHostToDevice);
  auto u32 = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_rows_from_affine, dim3(msm_grid(m, 64)), dim3(WG), 0, nullptr, m, d_pts, d_present, d_scratch, u32(L.bucket_rows));
    e = hipGetLastError();
  }
  int last = 0;
  if (e == hipSuccess) e = msm_launch_reduce<G>(nullptr, c, ws, L, &last);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_take_y, dim3((W * RW + 255) / 256), dim3(256), 0, nullptr, W, u32(L.pairs[last]), d_rows);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = normalise(d, (size_t)W, d_rows, out, flags);
  return (int)e;
}

// The whole schedule at a window width of the caller's choosing (the product always runs eccx_msm_window_bits(n)), on
// DEVICE buffers and a stream, without synchronising: what tools/bench_msm.py times to choose that function.  d_ws:
// msmcheck_msm_bytes(n, c) bytes, 256-byte aligned; d_out: 96 bytes; d_flag: 1 byte.
extern "C" size_t msmcheck_msm_bytes(size_t n, int c) {
  using namespace eccx;
  if (n == 0 || n > MSM_MAX_N || c < MSM_MIN_BITS || c > MSM_MAX_BITS) return 0;
  return msm_layout<G>(n, c).bytes;
}
extern "C" int msmcheck_msm_dev(size_t n, int c, const void* d_scalars, const void* d_points, void* d_ws, void* d_out, void* d_flag,
                                void* stream) {
  using namespace eccx;
  if (n == 0 || n > MSM_MAX_N || c < MSM_MIN_BITS || c > MSM_MAX_BITS || !d_scalars || !d_points || !d_ws || !d_out || !d_flag) return -1;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int cus = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
  uint32_t* row = nullptr;
  hipError_t e = msm_launch<G>(s, cus, n, c, static_cast<const uint8_t*>(d_scalars), static_cast<const uint8_t*>(d_points), nullptr,
                               static_cast<uint8_t*>(d_ws), &row, static_cast<uint8_t*>(d_flag), false);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((k_batch_to_affine_unsat<CU, NORM_HOMOGENEOUS, 8>), dim3(1), dim3(WG), 0, s, (size_t)1, row, static_cast<uint8_t*>(d_out),
                     static_cast<uint8_t*>(d_flag));
  return (int)hipGetLastError();
}

// The whole schedule on HOST buffers with the prepare and scatter grids capped as on a card of `cus` compute units
// (msm_grid(n, cus * 8): with cus = 1, 8 workgroups, 2048 lanes), so that a few thousand terms walk the grid-stride loop
// more than once.  inf: null or n flags; out: 96 bytes; flag: 1 byte.  It allocates, copies and synchronises.
extern "C" int msmcheck_msm_host(int cus, size_t n, int c, const uint8_t* scalars, const uint8_t* points, const uint8_t* inf, uint8_t* out,
                                 uint8_t* flag) {
  using namespace eccx;
  if (cus < 1 || n == 0 || n > MSM_MAX_N || c < MSM_MIN_BITS || c > MSM_MAX_BITS || !scalars || !points || !out || !flag) return -1;
  const size_t bytes = msm_layout<G>(n, c).bytes;
  Dev d;
  uint8_t* d_k = d.get<uint8_t>(n * 32, scalars);
  uint8_t* d_p = d.get<uint8_t>(n * G::POINT_BYTES, points);
  uint8_t* d_inf = inf ? d.get<uint8_t>(n, inf) : nullptr;
  uint8_t* ws = d.get<uint8_t>(bytes);
  uint8_t* d_out = d.get<uint8_t>(G::POINT_BYTES);
  uint8_t* d_fl = d.get<uint8_t>(1);
  if (d.e == hipSuccess) d.e = hipMemset(ws, 0xA5, bytes);  // junk wherever the schedule does not write first
  if (d.e != hipSuccess) return (int)d.e;
  uint32_t* row = nullptr;
  hipError_t e = msm_launch<G>(nullptr, cus, n, c, d_k, d_p, d_inf, ws, &row, d_fl, false);
  if (e == hipSuccess) {
    hipLaunchKernelGGL((k_batch_to_affine_unsat<CU, NORM_HOMOGENEOUS, 8>), dim3(1), dim3(WG), 0, nullptr, (size_t)1, row, d_out, d_fl);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, G::POINT_BYTES, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(flag, d_fl, 1, hipMemcpyDeviceToHost);
  return (int)e;
}
